// Whole-image inference on the device (reference UNet/inference.py:27-173, 201-206): the image is uploaded once in its raw dtype; per tile
//   unet_image_tile_gather  cuts the tile out of the (virtually) reflect-padded image, z-scores it and writes the network's [1][C][th][tw] input
//   unet_argmax_paste       takes the first maximum over the classes of the tile's softmax and writes the zone of responsibility into the mask
// so that nothing of a tile crosses the bus and no launch waits for the host.  No allocation, no globals, no environment.
#include "common.h"

namespace {

// np.pad(mode="reflect") index of padded coordinate i (>= 0) on an axis of n source elements: period 2(n - 1), the edge is not repeated
// (UNet/inference.py:46,156).  The periodic form, not a single fold: an axis shorter than the padding reflects more than once.  n >= 2 wherever
// i >= n (checked by the launcher).
__device__ __forceinline__ int reflect_index(int i, int n) {
    if (i < n) return i;
    const int p = 2 * (n - 1);
    const int m = i % p;
    return m < n ? m : p - m;
}

// One thread per (row, 4 columns) of the tile, all C channels: where the four columns are source columns (no reflection) the thread reads
// 4 * C consecutive source elements, so a wave reads one contiguous run of W*C; it writes one f32x4 per channel plane, contiguous along tw.
// (x - mean) / std as numpy evaluates it in float32 (UNet/imagereader.py:33-49): one subtraction, one correctly rounded division.
template <class T, int CT>
__global__ __launch_bounds__(256) void tile_gather_kernel(const T* __restrict__ img, int H, int W, int C, const float* __restrict__ mean,
        const float* __restrict__ sd, int y0, int x0, int th, int tw, float* __restrict__ out, int vec) {
    const int nq = (tw + 3) / 4;
    const long total = (long)th * nq, stride = (long)gridDim.x * 256;
    const size_t plane = (size_t)th * tw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int y = (int)(i / nq), x = (int)(i - (long)y * nq) * 4;
        const int sy = reflect_index(y0 + y, H);
        const T* row = img + (size_t)sy * W * C;
        const int gx = x0 + x;
        const bool full = x + 4 <= tw;
        if (CT > 0 && full && gx + 4 <= W) {
            T e[CT > 0 ? 4 * CT : 1];                                            // 4 pixels x CT channels, pixel-major: one contiguous run
            __builtin_memcpy(e, row + (size_t)gx * CT, sizeof(T) * 4 * CT);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float m = mean[c], s = sd[c];
                f32x4 r;
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = __fdiv_rn((float)e[k * CT + c] - m, s);
                float* o = out + (size_t)c * plane + (size_t)y * tw + x;
                if (vec) *reinterpret_cast<f32x4*>(o) = r;
                else { o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; }
            }
            continue;
        }
        const int nk = full ? 4 : tw - x;
        int sx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) sx[k] = reflect_index(gx + (k < nk ? k : 0), W);
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

// One thread per (zone row, 4 zone columns).  The comparison is argmax_kernel's (misc.hip): start at class 0, replace on v > m, so the FIRST
// maximum wins (np.argmax, UNet/inference.py:107,166).  K2: two classes stored densely, one 8-byte load per pixel.  Only zone pixels inside the
// mask extent are written: the halo and the reflect padding never are.
template <class M, int K2>
__global__ __launch_bounds__(256) void argmax_paste_kernel(const float* __restrict__ p, int ldp, int tw, int K, int oy, int ox, int zh, int zw,
        M* __restrict__ mask, long pitch, int my, int mx, int hm, int wm) {
    const int nq = (zw + 3) / 4;
    const long total = (long)zh * nq, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int r = (int)(i / nq), c = (int)(i - (long)r * nq) * 4;
        if (my + r >= hm || mx + c >= wm) continue;
        int nk = zw - c; if (nk > 4) nk = 4;
        if (nk > wm - (mx + c)) nk = wm - (mx + c);
        const float* zp = p + ((size_t)(oy + r) * tw + (ox + c)) * ldp;
        M am[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nk) break;
            const float* z = zp + (size_t)k * ldp;
            if (K2) {
                const f32x2 v = *reinterpret_cast<const f32x2*>(z);
                am[k] = (M)(v[1] > v[0] ? 1 : 0);
            } else {
                float m = z[0]; int a = 0;
                for (int j = 1; j < K; ++j) { const float v = z[j]; if (v > m) { m = v; a = j; } }
                am[k] = (M)a;
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
    }
}

int grid_rows(long total, int cap) { long b = (total + 255) / 256; if (b > cap) b = cap; if (b < 1) b = 1; return (int)b; }

template <class T>
int launch_gather(const void* img, int H, int W, int C, const float* mean, const float* sd, int y0, int x0, int th, int tw, float* out, hipStream_t st) {
    const int vec = (tw % 4 == 0 && unet_aligned16(out)) ? 1 : 0;
    const int g = grid_rows((long)th * ((tw + 3) / 4), 8192);
    const T* p = (const T*)img;
    if (C == 1)      tile_gather_kernel<T, 1><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, out, vec);
    else if (C == 3) tile_gather_kernel<T, 3><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, out, vec);
    else             tile_gather_kernel<T, 0><<<g, 256, 0, st>>>(p, H, W, C, mean, sd, y0, x0, th, tw, out, vec);
    return UNET_LAUNCH_STATUS();
}

template <class M>
int launch_paste(const float* prob, int ldp, int tw, int K, int oy, int ox, int zh, int zw, void* mask, long pitch, int my, int mx, int hm, int wm,
                 hipStream_t st) {
    const int g = grid_rows((long)zh * ((zw + 3) / 4), 8192);
    const bool k2 = K == 2 && ldp == 2 && (reinterpret_cast<uintptr_t>(prob) & 7u) == 0;
    if (k2) argmax_paste_kernel<M, 1><<<g, 256, 0, st>>>(prob, ldp, tw, K, oy, ox, zh, zw, (M*)mask, pitch, my, mx, hm, wm);
    else    argmax_paste_kernel<M, 0><<<g, 256, 0, st>>>(prob, ldp, tw, K, oy, ox, zh, zw, (M*)mask, pitch, my, mx, hm, wm);
    return UNET_LAUNCH_STATUS();
}

}  // namespace

// dtype: 0 = uint8, 1 = uint16, 2 = fp32 (include/unet_hip.h).  An axis of one element has no reflection (np.pad raises): refused.
extern "C" int unet_image_tile_gather(const void* img, int dtype, int H, int W, int C, const float* mean, const float* stddev,
                                      int y0, int x0, int th, int tw, float* out, void* stream) {
    UNET_CHECK_ARG(img && mean && stddev && out && (const void*)out != img && H > 0 && W > 0 && C > 0 && dtype >= 0 && dtype <= 2);
    UNET_CHECK_ARG(y0 >= 0 && x0 >= 0 && th > 0 && tw > 0 && (long)y0 + th <= 0x7fffffffL && (long)x0 + tw <= 0x7fffffffL);
    UNET_CHECK_ARG((H > 1 || y0 + th <= H) && (W > 1 || x0 + tw <= W));
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(img) & (dtype == 2 ? 3u : dtype == 1 ? 1u : 0u)) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) return launch_gather<uint8_t>(img, H, W, C, mean, stddev, y0, x0, th, tw, out, st);
    if (dtype == 1) return launch_gather<uint16_t>(img, H, W, C, mean, stddev, y0, x0, th, tw, out, st);
    return launch_gather<float>(img, H, W, C, mean, stddev, y0, x0, th, tw, out, st);
}

extern "C" int unet_argmax_paste(const float* prob, int ldp, int th, int tw, int K, int oy, int ox, int zh, int zw,
                                 void* mask, int elem_size, long pitch, int my, int mx, int Hm, int Wm, void* stream) {
    UNET_CHECK_ARG(prob && mask && th > 0 && tw > 0 && K > 0 && ldp >= K && (elem_size == 1 || elem_size == 4) && (elem_size == 4 || K <= 256));
    UNET_CHECK_ARG(oy >= 0 && ox >= 0 && zh > 0 && zw > 0 && (long)oy + zh <= th && (long)ox + zw <= tw);
    UNET_CHECK_ARG(my >= 0 && mx >= 0 && Hm > 0 && Wm > 0 && pitch >= Wm && (long)my + zh <= 0x7fffffffL && (long)mx + zw <= 0x7fffffffL);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(prob) & 3u) == 0 && (elem_size == 1 || (reinterpret_cast<uintptr_t>(mask) & 3u) == 0));
    if (my >= Hm || mx >= Wm) return UNET_OK;                                    // the zone lies in the padding: nothing to write
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 1) return launch_paste<uint8_t>(prob, ldp, tw, K, oy, ox, zh, zw, mask, pitch, my, mx, Hm, Wm, st);
    return launch_paste<int>(prob, ldp, tw, K, oy, ox, zh, zw, mask, pitch, my, mx, Hm, Wm, st);
}
