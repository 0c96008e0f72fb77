// Test-time augmentation and confidence maps for whole-image inference on the device (no counterpart in the reference: its
// UNet/inference.py forwards every tile once and keeps the arg-max only).  Per tile and per transform t of the square's dihedral group
//   unet_image_tile_gather_tta  writes the transform of unet_image_tile_gather's tile straight into the network's [1][C][th'][tw'] input
//   unet_prob_accumulate        brings the softmax of the transformed tile back to tile coordinates and stores / adds it into the accumulator
// and after the last transform
//   unet_argmax_paste_conf      unet_argmax_paste plus the winning probability and, on request, every class's probability.
// A permutation, a fixed-order fp32 sum, a power-of-two scale and a comparison: a host loop reproduces all three bit for bit.
//
// Transform code t (include/unet_hip.h): bit 2 = transpose the spatial axes, then bit 1 = flip rows, then bit 0 = flip columns.  With
// G the plain [C][th][tw] tile and X the transformed one:
//   t & 4 == 0:  X[c][a][b] = G[c][t & 2 ? th - 1 - a : a][t & 1 ? tw - 1 - b : b]           X is [C][th][tw]
//   t & 4 != 0:  X[c][a][b] = G[c][t & 1 ? th - 1 - b : b][t & 2 ? tw - 1 - a : a]           X is [C][tw][th]
// Flips are involutions, so the same two formulas read backwards are the inverse that unet_prob_accumulate applies.
//
// The transposing codes go through LDS in blocks of 32 x 32 pixels with a pitch of 33 floats: the block is read with the lanes along the
// source's fastest axis and written with the lanes along the destination's, so neither side of HBM sees a stride of one row per lane, and
// both the row-wise store (lane = column, stride 1) and the column-wise load (lane = row, stride 33) touch 32 different banks per half-wave.
// No allocation, no globals, no environment.
#include "common.h"

extern "C" int unet_image_tile_gather(const void* img, int dtype, int H, int W, int C, const float* mean, const float* stddev,
                                      int y0, int x0, int th, int tw, float* out, void* stream);

namespace {

constexpr int TS = 32;          // edge of a staged block, in pixels
constexpr int TP = TS + 1;      // its pitch in LDS
constexpr int CH = 4;           // channels (gather) / classes (accumulate) staged per pass: 4 * 32 * 33 floats = 16.5 KiB of LDS

// np.pad(mode="reflect") index, as in inference.hip: period 2(n - 1), any number of reflections; n >= 2 wherever i >= n (launcher)
__device__ __forceinline__ int reflect_index(int i, int n) {
    if (i < n) return i;
    const int p = 2 * (n - 1);
    const int m = i % p;
    return m < n ? m : p - m;
}

int grid_rows(long total, int cap) { long b = (total + 255) / 256; if (b > cap) b = cap; if (b < 1) b = 1; return (int)b; }
int grid_blocks(long blocks, int cap) { if (blocks > cap) blocks = cap; if (blocks < 1) blocks = 1; return (int)blocks; }

// Codes 1..3.  tile_gather_kernel's thread shape -- one thread per (OUTPUT row, 4 output columns), all channels, one f32x4 store per channel
// plane -- with the source row mirrored (fy) and the four source columns taken in descending order (fx): where they are plain source
// columns the thread still reads one contiguous run of 4 * C elements and reverses it in registers.
template <class T, int CT>
__global__ __launch_bounds__(256) void tile_gather_flip_kernel(const T* __restrict__ img, int H, int W, int C, const float* __restrict__ mean,
        const float* __restrict__ sd, int y0, int x0, int th, int tw, int fy, int fx, float* __restrict__ out, int vec) {
    const int nq = (tw + 3) / 4;
    const long total = (long)th * nq, stride = (long)gridDim.x * 256;
    const size_t plane = (size_t)th * tw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int y = (int)(i / nq), x = (int)(i - (long)y * nq) * 4;
        const int sy = reflect_index(y0 + (fy ? th - 1 - y : y), H);
        const T* row = img + (size_t)sy * W * C;
        const bool full = x + 4 <= tw;
        const int gx = x0 + (fx ? tw - 4 - x : x);                               // lowest of the four tile columns (>= x0 when full)
        if (CT > 0 && full && gx + 4 <= W) {
            T e[CT > 0 ? 4 * CT : 1];
            __builtin_memcpy(e, row + (size_t)gx * CT, sizeof(T) * 4 * CT);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float m = mean[c], s = sd[c];
                f32x4 r;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn((float)(fx ? e[(3 - k) * CT + c] : e[k * CT + c]) - m, s);
                float* o = out + (size_t)c * plane + (size_t)y * tw + x;
                if (vec) *reinterpret_cast<f32x4*>(o) = r;
                else { o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; }
            }
            continue;
        }
        const int nk = full ? 4 : tw - x;
        int sx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xk = x + (k < nk ? k : 0);
            sx[k] = reflect_index(x0 + (fx ? tw - 1 - xk : xk), W);
        }
        for (int c = 0; c < C; ++c) {
            const float m = mean[c], s = sd[c];
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn((float)row[(size_t)sx[k] * C + c] - m, s);
            float* o = out + (size_t)c * plane + (size_t)y * tw + x;
            if (vec && full) *reinterpret_cast<f32x4*>(o) = r;
            else for (int k = 0; k < nk; ++k) o[k] = r[k];
        }
    }
}

// Codes 4..7.  One block per 32 x 32 pixels of the plain tile (grid-stride over the blocks), up to CH channels per pass.  Load: lane = tile
// column, so a half-wave reads 32 consecutive source pixels (32 * C elements, one run where nothing reflects).  Store: lane = tile row =
// output column, so a half-wave writes 32 consecutive floats of one output row (in descending lane order under fb: the same 128 bytes).
template <class T>
__global__ __launch_bounds__(256) void tile_gather_transpose_kernel(const T* __restrict__ img, int H, int W, int C, const float* __restrict__ mean,
        const float* __restrict__ sd, int y0, int x0, int th, int tw, int fa, int fb, float* __restrict__ out) {
    __shared__ float lds[CH][TS][TP];
    const int nbx = (tw + TS - 1) / TS, nby = (th + TS - 1) / TS;
    const long nblk = (long)nbx * nby;
    const size_t plane = (size_t)th * tw;
    const int l = threadIdx.x & (TS - 1), q = threadIdx.x >> 5;                  // lane within a half-wave, 8 quarter-rows per pass
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int gy0 = (int)(blk / nbx) * TS, gx0 = (int)(blk - (long)(blk / nbx) * nbx) * TS;
        for (int c0 = 0; c0 < C; c0 += CH) {
            const int nc = C - c0 < CH ? C - c0 : CH;
#pragma unroll
            for (int i = 0; i < TS / 8; ++i) {
                const int r = q + 8 * i, gy = gy0 + r, gx = gx0 + l;
                if (gy < th && gx < tw) {
                    const T* src = img + ((size_t)reflect_index(y0 + gy, H) * W + reflect_index(x0 + gx, W)) * C + c0;
                    for (int c = 0; c < nc; ++c) lds[c][r][l] = __fdiv_rn((float)src[c] - mean[c0 + c], sd[c0 + c]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < TS / 8; ++i) {
                const int r = q + 8 * i, gy = gy0 + l, gx = gx0 + r;              // r = tile column (output row), l = tile row (output column)
                if (gy < th && gx < tw) {
                    const int a = fa ? tw - 1 - gx : gx, b = fb ? th - 1 - gy : gy;
                    float* o = out + (size_t)c0 * plane + (size_t)a * th + b;
                    for (int c = 0; c < nc; ++c) o[(size_t)c * plane] = lds[c][l][r];
                }
            }
            __syncthreads();
        }
    }
}

// Codes 0..3: one thread per accumulator pixel, which owns its K floats; the source pixel is the mirrored one, so the lanes of a wave
// read one contiguous run backwards.  KT = 2 / 4: K == ldp == lda == KT and both tensors aligned, one 8- / 16-byte access per tensor.
template <int KT>
__global__ __launch_bounds__(256) void prob_accumulate_kernel(const float* __restrict__ p, int ldp, int th, int tw, int K, int fy, int fx, int first,
        float* __restrict__ acc, int lda) {
    const long total = (long)th * tw, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int y = (int)(i / tw), x = (int)(i - (long)y * tw);
        const int sy = fy ? th - 1 - y : y, sx = fx ? tw - 1 - x : x;
        const float* s = p + ((size_t)sy * tw + sx) * ldp;
        float* d = acc + (size_t)i * lda;
        if (KT > 0) {
            typedef float V __attribute__((ext_vector_type(KT > 0 ? KT : 1)));
            V v = *reinterpret_cast<const V*>(s);
            if (!first) v = *reinterpret_cast<const V*>(d) + v;
            *reinterpret_cast<V*>(d) = v;
        } else if (first) {
            for (int k = 0; k < K; ++k) d[k] = s[k];
        } else {
            for (int k = 0; k < K; ++k) d[k] = d[k] + s[k];
        }
    }
}

// Codes 4..7: prob is [tw][th] pixels, acc [th][tw].  32 x 32 pixels and up to CH classes per pass.  Load: lane = prob column, each lane
// the pixel's (up to) CH consecutive floats.  Store: lane = prob row = accumulator column, again the pixel's consecutive floats.
__global__ __launch_bounds__(256) void prob_accumulate_transpose_kernel(const float* __restrict__ p, int ldp, int th, int tw, int K, int fa, int fb,
        int first, float* __restrict__ acc, int lda) {
    __shared__ float lds[CH][TS][TP];
    const int nbb = (th + TS - 1) / TS, nba = (tw + TS - 1) / TS;                 // prob: rows a in [0, tw), columns b in [0, th)
    const long nblk = (long)nba * nbb;
    const int l = threadIdx.x & (TS - 1), q = threadIdx.x >> 5;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int a0 = (int)(blk / nbb) * TS, b0 = (int)(blk - (long)(blk / nbb) * nbb) * TS;
        for (int k0 = 0; k0 < K; k0 += CH) {
            const int nk = K - k0 < CH ? K - k0 : CH;
#pragma unroll
            for (int i = 0; i < TS / 8; ++i) {
                const int r = q + 8 * i, a = a0 + r, b = b0 + l;
                if (a < tw && b < th) {
                    const float* s = p + ((size_t)a * th + b) * ldp + k0;
                    for (int k = 0; k < nk; ++k) lds[k][r][l] = s[k];
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < TS / 8; ++i) {
                const int r = q + 8 * i, a = a0 + l, b = b0 + r;
                if (a < tw && b < th) {
                    const int y = fb ? th - 1 - b : b, x = fa ? tw - 1 - a : a;
                    float* d = acc + ((size_t)y * tw + x) * lda + k0;
                    if (first) for (int k = 0; k < nk; ++k) d[k] = lds[k][l][r];
                    else       for (int k = 0; k < nk; ++k) d[k] = d[k] + lds[k][l][r];
                }
            }
            __syncthreads();
        }
    }
}

// argmax_paste_kernel's thread shape, zone and clipping (inference.hip) and its comparison -- start at class 0, replace on v > m, on the
// UNSCALED values -- so the mask is that kernel's; conf receives m * scale, prob_out every class's value * scale.
template <class M>
__global__ __launch_bounds__(256) void argmax_paste_conf_kernel(const float* __restrict__ p, int ldp, int tw, int K, float scale, int oy, int ox,
        int zh, int zw, M* __restrict__ mask, long pitch, int my, int mx, int hm, int wm, float* __restrict__ conf, long conf_pitch,
        float* __restrict__ prob_out) {
    const int nq = (zw + 3) / 4;
    const long total = (long)zh * nq, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int r = (int)(i / nq), c = (int)(i - (long)r * nq) * 4;
        if (my + r >= hm || mx + c >= wm) continue;
        int nk = zw - c; if (nk > 4) nk = 4;
        if (nk > wm - (mx + c)) nk = wm - (mx + c);
        const float* zp = p + ((size_t)(oy + r) * tw + (ox + c)) * ldp;
        M am[4] = {0, 0, 0, 0};
        float cf[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nk) break;
            const float* z = zp + (size_t)k * ldp;
            float m = z[0]; int a = 0;
            for (int j = 1; j < K; ++j) { const float v = z[j]; if (v > m) { m = v; a = j; } }
            am[k] = (M)a;
            cf[k] = m * scale;
            if (prob_out) {
                float* po = prob_out + ((size_t)(my + r) * wm + (mx + c + k)) * K;
                for (int j = 0; j < K; ++j) po[j] = z[j] * scale;
            }
        }
        M* o = mask + (size_t)(my + r) * pitch + (mx + c);
        typedef M MV __attribute__((ext_vector_type(4)));
        if (nk == 4 && (reinterpret_cast<uintptr_t>(o) & (sizeof(MV) - 1)) == 0) {
            MV v; v[0] = am[0]; v[1] = am[1]; v[2] = am[2]; v[3] = am[3];
            *reinterpret_cast<MV*>(o) = v;
        } else {
            for (int k = 0; k < nk; ++k) o[k] = am[k];
        }
        if (conf) {
            float* co = conf + (size_t)(my + r) * conf_pitch + (mx + c);
            if (nk == 4 && (reinterpret_cast<uintptr_t>(co) & 15u) == 0) { f32x4 v; v[0] = cf[0]; v[1] = cf[1]; v[2] = cf[2]; v[3] = cf[3]; *reinterpret_cast<f32x4*>(co) = v; }
            else for (int k = 0; k < nk; ++k) co[k] = cf[k];
        }
    }
}

template <class T>
int launch_gather_tta(const void* img, int H, int W, int C, const float* mean, const float* sd, int y0, int x0, int th, int tw, int t, float* out,
                      hipStream_t st) {
    const T* p = (const T*)img;
    if (t & 4) {
        const int g = grid_blocks((long)((th + TS - 1) / TS) * ((tw + TS - 1) / TS), 8192);
        tile_gather_transpose_kernel<T><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, (t >> 1) & 1, t & 1, out);
        return UNET_LAUNCH_STATUS();
    }
    const int vec = (tw % 4 == 0 && unet_aligned16(out)) ? 1 : 0;
    const int g = grid_rows((long)th * ((tw + 3) / 4), 8192);
    const int fy = (t >> 1) & 1, fx = t & 1;
    if (C == 1)      tile_gather_flip_kernel<T, 1><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, fy, fx, out, vec);
    else if (C == 3) tile_gather_flip_kernel<T, 3><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, fy, fx, out, vec);
    else             tile_gather_flip_kernel<T, 0><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, fy, fx, out, vec);
    return UNET_LAUNCH_STATUS();
}

template <class M>
int launch_paste_conf(const float* acc, int lda, int tw, int K, float scale, int oy, int ox, int zh, int zw, void* mask, long pitch, int my, int mx,
                      int hm, int wm, float* conf, long conf_pitch, float* prob_out, hipStream_t st) {
    const int g = grid_rows((long)zh * ((zw + 3) / 4), 8192);
    argmax_paste_conf_kernel<M><<<g, 256, 0, st>>>(acc, lda, tw, K, scale, oy, ox, zh, zw, (M*)mask, pitch, my, mx, hm, wm, conf, conf_pitch, prob_out);
    return UNET_LAUNCH_STATUS();
}

}  // namespace

extern "C" int unet_image_tile_gather_tta(const void* img, int dtype, int H, int W, int C, const float* mean, const float* stddev,
                                          int y0, int x0, int th, int tw, int transform, float* out, void* stream) {
    UNET_CHECK_ARG(transform >= 0 && transform <= 7);
    if (transform == 0) return unet_image_tile_gather(img, dtype, H, W, C, mean, stddev, y0, x0, th, tw, out, stream);
    UNET_CHECK_ARG(img && mean && stddev && out && (const void*)out != img && H > 0 && W > 0 && C > 0 && dtype >= 0 && dtype <= 2);
    UNET_CHECK_ARG(y0 >= 0 && x0 >= 0 && th > 0 && tw > 0 && (long)y0 + th <= 0x7fffffffL && (long)x0 + tw <= 0x7fffffffL);
    UNET_CHECK_ARG((H > 1 || y0 + th <= H) && (W > 1 || x0 + tw <= W));
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(img) & (dtype == 2 ? 3u : dtype == 1 ? 1u : 0u)) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) return launch_gather_tta<uint8_t>(img, H, W, C, mean, stddev, y0, x0, th, tw, transform, out, st);
    if (dtype == 1) return launch_gather_tta<uint16_t>(img, H, W, C, mean, stddev, y0, x0, th, tw, transform, out, st);
    return launch_gather_tta<float>(img, H, W, C, mean, stddev, y0, x0, th, tw, transform, out, st);
}

extern "C" int unet_prob_accumulate(const float* prob, int ldp, int th, int tw, int K, int transform, int first, float* acc, int lda, void* stream) {
    UNET_CHECK_ARG(prob && acc && th > 0 && tw > 0 && K >= 1 && ldp >= K && lda >= K && transform >= 0 && transform <= 7);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(prob) & 3u) == 0 && (reinterpret_cast<uintptr_t>(acc) & 3u) == 0);
    const size_t px = (size_t)th * tw;
    const float* pe = prob + (px - 1) * (size_t)ldp + K;                          // one past the last float either side touches
    const float* ae = acc + (px - 1) * (size_t)lda + K;
    UNET_CHECK_ARG(reinterpret_cast<uintptr_t>(pe) <= reinterpret_cast<uintptr_t>(acc) || reinterpret_cast<uintptr_t>(ae) <= reinterpret_cast<uintptr_t>(prob));
    hipStream_t st = (hipStream_t)stream;
    const int f1 = (transform >> 1) & 1, f0 = transform & 1;
    if (transform & 4) {
        const int g = grid_blocks((long)((th + TS - 1) / TS) * ((tw + TS - 1) / TS), 8192);
        prob_accumulate_transpose_kernel<<<g, 256, 0, st>>>(prob, ldp, th, tw, K, f1, f0, first ? 1 : 0, acc, lda);
        return UNET_LAUNCH_STATUS();
    }
    const int g = grid_rows((long)px, 8192);
    const bool dense = ldp == K && lda == K;
    const uintptr_t both = reinterpret_cast<uintptr_t>(prob) | reinterpret_cast<uintptr_t>(acc);
    if (dense && K == 2 && (both & 7u) == 0)       prob_accumulate_kernel<2><<<g, 256, 0, st>>>(prob, ldp, th, tw, K, f1, f0, first ? 1 : 0, acc, lda);
    else if (dense && K == 4 && (both & 15u) == 0) prob_accumulate_kernel<4><<<g, 256, 0, st>>>(prob, ldp, th, tw, K, f1, f0, first ? 1 : 0, acc, lda);
    else                                           prob_accumulate_kernel<0><<<g, 256, 0, st>>>(prob, ldp, th, tw, K, f1, f0, first ? 1 : 0, acc, lda);
    return UNET_LAUNCH_STATUS();
}

extern "C" int unet_argmax_paste_conf(const float* acc, int lda, int th, int tw, int K, float scale, int oy, int ox, int zh, int zw,
                                      void* mask, int elem_size, long pitch, int my, int mx, int Hm, int Wm,
                                      float* conf, long conf_pitch, float* prob_out, void* stream) {
    UNET_CHECK_ARG(acc && mask && th > 0 && tw > 0 && K > 0 && lda >= K && (elem_size == 1 || elem_size == 4) && (elem_size == 4 || K <= 256));
    UNET_CHECK_ARG((conf || prob_out) && (!conf || conf_pitch >= Wm));
    UNET_CHECK_ARG(oy >= 0 && ox >= 0 && zh > 0 && zw > 0 && (long)oy + zh <= th && (long)ox + zw <= tw);
    UNET_CHECK_ARG(my >= 0 && mx >= 0 && Hm > 0 && Wm > 0 && pitch >= Wm && (long)my + zh <= 0x7fffffffL && (long)mx + zw <= 0x7fffffffL);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(acc) & 3u) == 0 && (elem_size == 1 || (reinterpret_cast<uintptr_t>(mask) & 3u) == 0));
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(conf) & 3u) == 0 && (reinterpret_cast<uintptr_t>(prob_out) & 3u) == 0);
    if (my >= Hm || mx >= Wm) return UNET_OK;                                    // the zone lies in the padding: nothing to write
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 1) return launch_paste_conf<uint8_t>(acc, lda, tw, K, scale, oy, ox, zh, zw, mask, pitch, my, mx, Hm, Wm, conf, conf_pitch, prob_out, st);
    return launch_paste_conf<int>(acc, lda, tw, K, scale, oy, ox, zh, zw, mask, pitch, my, mx, Hm, Wm, conf, conf_pitch, prob_out, st);
}
