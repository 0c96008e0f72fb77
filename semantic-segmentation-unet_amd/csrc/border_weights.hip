// Border-distance loss weights (the U-Net recipe's per-pixel weight map, single-transform form), per image, from the step's own one-hot labels:
//   c(p)  = first maximum of pixel p's one-hot row (the loop of unet_softmax_ce_weighted); a row with no positive entry is UNLABELED
//   B     = labeled pixels with a labeled 4-neighbour inside the image of another class (both sides of a class border; the image edge is no
//           border; unlabeled pixels are never in B and put no neighbour in it)
//   d2(p) = exact squared Euclidean distance in pixels from p to the nearest pixel of B (int32; 0 on B; UNET_BORDER_NONE = INT32_MAX when
//           the image has no border pixel)
//   w(p)  = (1 + w0 * exp(d2(p) * neg_inv_2sigma2)) * m(p), the term exactly 0 when d2 == UNET_BORDER_NONE; m = pixel_weight_in or 1;
//           evaluated in double from the fp32 arguments and rounded to fp32 ONCE.  Not expf in fp32: a map that differs from the exact one in
//           its last bit is harmless to the loss, but the first Adam step moves a parameter by lr g / (|g| + 1e-7), which turns last-bit
//           differences of the gradient into 1e-3 of a tensor's magnitude where g is near zero (measured: two explicit maps one ulp apart).
//           Rounded once from double, the device's map is the fp32 rounding of the definition itself, so a step with it is the step with
//           that map handed in as pixel_weights, bit for bit.  2 M double exponentials are a few microseconds.
// An exact Euclidean distance transform, separable: the squared distance is min over x' of (x - x')^2 + g(x')^2 with g the vertical distance
// to the nearest B pixel of column x'.  Four launches, all integer until the final exponential:
//   1. class_kernel   one-hot -> one class byte per pixel (255 = unlabeled).  The only pass over the 4 K bytes per pixel; K in {2, 4} with a
//                     16-byte aligned label tensor: a lane owns 4 pixels, 16-byte loads, one packed 4-byte store.
//   2. mask_kernel    a lane owns 32 rows of one column (a "chunk"): border flag of each from the class bytes of the pixel and its four
//                     neighbours, packed into one 32-bit mask (bit i = row 32 chunk + i).  The flags never reach memory as bytes.
//   3. column_kernel  a lane owns a chunk again: nearest set bit above and below it (a walk over the column's other masks, at most H / 32 of
//                     them each way), then per row the nearest bit of its own mask by clz / ctz; stores g^2, or NONE for a column without B.
//   4. row_kernel     one workgroup per image row: g^2 of the row staged in LDS; a lane owns an x and searches outward, x - r and x + r, until
//                     r^2 reaches its running minimum (every later candidate is >= r^2: exact; at most W - 1 trips).  Lanes of a wave read
//                     consecutive LDS words: no bank conflict.  A row whose columns all hold NONE (an image without border) skips the search.
//                     The exponential, the multiply by pixel_weight_in and both stores are fused here.
// No atomics, no floating-point sums, no loop bound other than H, W (or H / 32): the same bits run after run, d2 exact by construction.
// NONE is never added to: a candidate is formed only from a finite g^2 <= 16383^2, plus r^2 <= 16383^2, < 2^29.
#include "common.h"
#include <math.h>

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WG = 256;
constexpr int CHUNK = 32;                        // rows per mask word
constexpr int NONE = 0x7fffffff;                 // UNET_BORDER_NONE
constexpr unsigned UNLABELED = 255u;
constexpr int MAX_SIDE = 16384;                  // H^2 + W^2 < 2^31; a row of W int32 is at most 64 KiB of LDS

// first maximum of a one-hot row; no positive entry: unlabeled
template <int KT>
__device__ __forceinline__ unsigned class_of(const int* lp, int Krt) {
    const int K = KT ? KT : Krt;
    int best = lp[0], al = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) { const int li = lp[k]; if (li > best) { best = li; al = k; } }
    return best > 0 ? (unsigned)al : UNLABELED;
}

// K in {2, 4}, labels 16-byte aligned: 4 pixels per lane
template <int K>
__global__ __launch_bounds__(WG) void class_dense_kernel(const int* __restrict__ lab, uint8_t* __restrict__ cls, long P) {
    const long nq = P >> 2, stride = (long)gridDim.x * WG;
    for (long q = (long)blockIdx.x * WG + threadIdx.x; q < nq; q += stride) {
        int lv[4 * K];
#pragma unroll
        for (int v = 0; v < K; ++v) {
            const i32x4 t = *reinterpret_cast<const i32x4*>(lab + (size_t)q * 4 * K + 4 * v);
#pragma unroll
            for (int e = 0; e < 4; ++e) lv[4 * v + e] = t[e];
        }
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) packed |= class_of<K>(lv + j * K, K) << (8 * j);
        *reinterpret_cast<unsigned*>(cls + (size_t)q * 4) = packed;
    }
    const long tail = (nq << 2) + (long)blockIdx.x * WG + threadIdx.x;          // the last P % 4 pixels
    if (tail < P) cls[tail] = (uint8_t)class_of<K>(lab + (size_t)tail * K, K);
}

__global__ __launch_bounds__(WG) void class_generic_kernel(const int* __restrict__ lab, uint8_t* __restrict__ cls, long P, int K) {
    const long stride = (long)gridDim.x * WG;
    for (long p = (long)blockIdx.x * WG + threadIdx.x; p < P; p += stride) cls[p] = (uint8_t)class_of<0>(lab + (size_t)p * K, K);
}

// lane = (image n, chunk c, column x), x fastest: neighbouring lanes read neighbouring class bytes
__global__ __launch_bounds__(WG) void mask_kernel(const uint8_t* __restrict__ cls, unsigned* __restrict__ masks, int N, int H, int W, int nch) {
    const long total = (long)N * nch * W, stride = (long)gridDim.x * WG;
    for (long t = (long)blockIdx.x * WG + threadIdx.x; t < total; t += stride) {
        const int x = (int)(t % W); const long nc = t / W;
        const int c = (int)(nc % nch); const long n = nc / nch;
        const uint8_t* col = cls + (size_t)n * H * W + x;
        const int y0 = c * CHUNK, y1 = y0 + CHUNK < H ? y0 + CHUNK : H;
        unsigned up = y0 > 0 ? col[(size_t)(y0 - 1) * W] : UNLABELED, cur = col[(size_t)y0 * W], m = 0;
        for (int y = y0; y < y1; ++y) {
            const uint8_t* px = col + (size_t)y * W;
            const unsigned down = y + 1 < H ? px[W] : UNLABELED;
            const unsigned left = x > 0 ? px[-1] : UNLABELED, right = x + 1 < W ? px[1] : UNLABELED;
            // a neighbour outside the image or unlabeled never differs; an unlabeled pixel is never a border
            const bool differs = (up != UNLABELED && up != cur) || (down != UNLABELED && down != cur) ||
                                 (left != UNLABELED && left != cur) || (right != UNLABELED && right != cur);
            if (cur != UNLABELED && differs) m |= 1u << (y - y0);
            up = cur; cur = down;
        }
        masks[t] = m;
    }
}

__global__ __launch_bounds__(WG) void column_kernel(const unsigned* __restrict__ masks, int* __restrict__ gsq, int N, int H, int W, int nch) {
    const long total = (long)N * nch * W, stride = (long)gridDim.x * WG;
    for (long t = (long)blockIdx.x * WG + threadIdx.x; t < total; t += stride) {
        const int x = (int)(t % W); const long nc = t / W;
        const int c = (int)(nc % nch); const long n = nc / nch;
        const unsigned* cm = masks + (size_t)n * nch * W + x;       // this column's masks, W words apart
        const unsigned m = cm[(size_t)c * W];
        int above = -1, below = -1;                                  // row of the nearest B pixel outside this chunk; -1: none
        for (int cc = c - 1; cc >= 0; --cc) {
            const unsigned mm = cm[(size_t)cc * W];
            if (mm) { above = cc * CHUNK + 31 - __clz((int)mm); break; }
        }
        for (int cc = c + 1; cc < nch; ++cc) {
            const unsigned mm = cm[(size_t)cc * W];
            if (mm) { below = cc * CHUNK + __ffs((int)mm) - 1; break; }
        }
        const int y0 = c * CHUNK, y1 = y0 + CHUNK < H ? y0 + CHUNK : H;
        int* out = gsq + (size_t)n * H * W + x;
        for (int y = y0; y < y1; ++y) {
            const int i = y - y0;
            const unsigned lo = m & (0xffffffffu >> (31 - i)), hi = m >> i;      // bits at or above the row / at or below it
            int g = NONE;
            if (lo) g = i - (31 - __clz((int)lo)); else if (above >= 0) g = y - above;
            int gd = NONE;
            if (hi) gd = __ffs((int)hi) - 1; else if (below >= 0) gd = below - y;
            if (gd < g) g = gd;
            out[(size_t)y * W] = g == NONE ? NONE : g * g;
        }
    }
}

// one workgroup per row (n, y); dynamic LDS: W int32
__global__ __launch_bounds__(WG) void row_kernel(const int* __restrict__ gsq, const float* __restrict__ pw, float w0, float c, float* __restrict__ wout,
                                                 int* __restrict__ d2out, int W) {
    extern __shared__ int row[];
    const size_t base = (size_t)blockIdx.x * W;
    int any = 0;
    for (int x = threadIdx.x; x < W; x += blockDim.x) { const int v = gsq[base + x]; row[x] = v; any |= v != NONE; }
    any = __syncthreads_or(any);                                     // (also the barrier behind the staging stores)
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        int best = row[x];
        if (any) {
            for (int r = 1; r < W; ++r) {
                const int r2 = r * r;
                if (r2 >= best) break;
                if (x - r >= 0) { const int v = row[x - r]; if (v != NONE && v + r2 < best) best = v + r2; }
                if (x + r < W) { const int v = row[x + r]; if (v != NONE && v + r2 < best) best = v + r2; }
            }
        }
        // in double, rounded to fp32 once: the stored weight is the fp32 rounding of the definition's exact value (see the header of this file)
        const double term = best == NONE ? 0.0 : (double)w0 * exp((double)best * (double)c);
        double w = 1.0 + term;
        if (pw) w = w * (double)pw[base + x];
        wout[base + x] = (float)w;
        if (d2out) d2out[base + x] = best;
    }
}

int grid_for(long total, int cap) { long b = (total + WG - 1) / WG; if (b > cap) b = cap; if (b < 1) b = 1; return (int)b; }

struct Layout { size_t gsq, masks, cls, bytes; int nch; };
Layout layout_of(int N, int H, int W) {
    Layout l;
    const size_t P = (size_t)N * H * W;
    l.nch = (H + CHUNK - 1) / CHUNK;
    l.gsq = 0;
    l.masks = P * 4;
    l.cls = l.masks + (size_t)N * l.nch * W * 4;
    l.bytes = l.cls + ((P + 3) & ~(size_t)3);
    return l;
}
bool shape_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE && (long)N * H <= 0x7fffffffL; }

}  // namespace

extern "C" size_t unet_border_weights_workspace(int N, int H, int W) { return shape_ok(N, H, W) ? layout_of(N, H, W).bytes : 0; }

extern "C" int unet_border_weights(const int* labels_onehot, int K, const float* pixel_weight_in, float w0, float neg_inv_2sigma2,
                                   float* weights_out, int* d2_out, int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    UNET_CHECK_ARG(labels_onehot && weights_out && ws && shape_ok(N, H, W));
    UNET_CHECK_ARG(K >= 1 && K <= 255);                                              // one class byte per pixel, 255 = unlabeled
    UNET_CHECK_ARG(isfinite(w0) && w0 >= 0.f && isfinite(neg_inv_2sigma2) && neg_inv_2sigma2 < 0.f);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 3u) == 0);
    const Layout l = layout_of(N, H, W);
    if (ws_bytes < l.bytes) return UNET_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    int* gsq = reinterpret_cast<int*>((char*)ws + l.gsq);
    unsigned* masks = reinterpret_cast<unsigned*>((char*)ws + l.masks);
    uint8_t* cls = reinterpret_cast<uint8_t*>((char*)ws + l.cls);
    const long P = (long)N * H * W;
    if ((K == 2 || K == 4) && unet_aligned16(labels_onehot)) {
        const int nblk = grid_for(P >> 2, 4096);                                     // (never empty: the first lanes also take the tail)
        if (K == 2) class_dense_kernel<2><<<nblk, WG, 0, st>>>(labels_onehot, cls, P);
        else class_dense_kernel<4><<<nblk, WG, 0, st>>>(labels_onehot, cls, P);
    } else {
        class_generic_kernel<<<grid_for(P, 4096), WG, 0, st>>>(labels_onehot, cls, P, K);
    }
    int rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    const int nblk = grid_for((long)N * l.nch * W, 4096);
    mask_kernel<<<nblk, WG, 0, st>>>(cls, masks, N, H, W, l.nch);
    rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    column_kernel<<<nblk, WG, 0, st>>>(masks, gsq, N, H, W, l.nch);
    rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    const int threads = W >= WG ? WG : ((W + 63) / 64) * 64;
    row_kernel<<<N * H, threads, (size_t)W * sizeof(int), st>>>(gsq, pixel_weight_in, w0, neg_inv_2sigma2, weights_out, d2_out, W);
    return UNET_LAUNCH_STATUS();
}
