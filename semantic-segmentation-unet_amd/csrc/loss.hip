// Weighted training loss: Softmax + CategoricalCrossentropy as unet_softmax_ce (misc.hip) computes them, with a weight per pixel
//   w_p = class_weight[t_p] * pixel_weight[p]        (t_p = first maximum of the one-hot row; a NULL factor is 1; one fp32 multiply)
//   loss = loss_scale * sum_p w_p * l_p,   dlogits[p][k] = (the unweighted value, grad_scale included) * w_p
// (Keras: loss_fn(labels, softmax, sample_weight=w), UNet/model.py:211; the reduction stays "sum / G, mean over H, W": NOT divided by the
// weight sum, which is reported instead) and, with ignore_empty, pixels whose one-hot row has no positive entry left out: no loss, a
// dlogits row of +0.0 (stored, the buffer is reused), not counted as correct or valid; their prob row is still written.
//
// HBM-bound: 32 B per pixel at K = 2 (+ 4 B with a pixel-weight map).  One grid-stride pass, at most 1024 workgroups:
//   dense    K in {2, 4}, ldz == lddz == K, logits / labels / prob / dlogits all 16-byte aligned: one 16-byte load or store per tensor and
//            lane (two pixels at K = 2, one at K = 4), the exponentials taken once and kept in registers;
//   generic  every other K, leading dimension, alignment or missing output: one pixel per lane, the loops of softmax_ce_kernel.
// Both run ce_pixel below, which is softmax_ce_kernel's arithmetic operation for operation: with all weights 1 prob and dlogits are that
// kernel's bits.  Reductions: per lane in double / integers, per wave by shuffles, per workgroup one partial of each (double loss, double
// weight sum, 64-bit correct, 64-bit valid) in the workspace; a one-workgroup kernel adds the partials in a fixed order.  No floating-point
// atomics: the result does not depend on launch order.
// Companions: unet_labels_onehot_ignore (class map -> one-hot with an unlabeled value).
#include "common.h"

namespace {

typedef unsigned long long u64;
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WG = 256;

__device__ __forceinline__ float smoothed(int li, float ls, int K) {
    float y = (float)li;
    if (ls > 0.f) y = y * (1.f - ls) + ls / (float)K;
    return y;
}

struct Sums { double loss, weight; unsigned correct, valid; };

// One pixel.  zp / lp: its K logits and one-hot entries (registers on the dense path, memory on the generic one; lp may be null: then no
// loss, no gradient); pp / dp: where its prob / dlogits rows go (each may be null).  KT > 0: K at compile time, exponentials kept.
template <int KT>
__device__ __forceinline__ void ce_pixel(const float* zp, const int* lp, int Krt, const float* __restrict__ cw, float pwv, int ignore_empty,
        float* pp, float* dp, float ls, float grad_scale, float clip_eps, Sums& acc) {
    const int K = KT ? KT : Krt;
    float e[KT ? KT : 1];
    float m = zp[0]; int am = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) { const float v = zp[k]; if (v > m) { m = v; am = k; } }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { const float ek = expf(zp[k] - m); if constexpr (KT != 0) e[k] = ek; se += ek; }
    const float lse = logf(se), inv = 1.f / se;
    auto p_of = [&](int k) { if constexpr (KT != 0) return e[k] * inv; else return expf(zp[k] - m) * inv; };
    float ysum = 0.f, ell = 0.f; int al = 0, lbest = 0;
    if (lp) {
        lbest = lp[0];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int li = lp[k];
            if (li > lbest) { lbest = li; al = k; }
            const float y = smoothed(li, ls, K);
            ysum += y;
            if (clip_eps > 0.f) ell -= y * logf(fminf(fmaxf(p_of(k), clip_eps), 1.f - clip_eps));     // Keras' clipped-probability path
            else ell -= y * ((zp[k] - m) - lse);
        }
    }
    const bool labeled = !(ignore_empty && lbest <= 0);
    const float w = (cw ? cw[al] : 1.f) * pwv;
    float gdot = 0.f;                            // clip path: sum_j g_j p_j with g_j = -y_j / q_j inside the clip range
    if (dp && clip_eps > 0.f) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float pk = p_of(k);
            if (pk >= clip_eps && pk <= 1.f - clip_eps) gdot -= smoothed(lp[k], ls, K);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float pk = p_of(k);
        if (pp) pp[k] = pk;
        if (dp) {
            float g = 0.f;                       // an unlabeled pixel: +0.0, stored, not 0 * x
            if (labeled) {
                const float y = smoothed(lp[k], ls, K);
                if (clip_eps > 0.f) {
                    const float gp = (pk >= clip_eps && pk <= 1.f - clip_eps) ? -y : 0.f;
                    g = (gp - pk * gdot) * grad_scale;
                } else {
                    g = (pk * ysum - y) * grad_scale;
                }
                g = g * w;
            }
            dp[k] = g;
        }
    }
    if (lp && labeled) {
        acc.loss += (double)w * (double)ell;
        acc.weight += (double)w;
        acc.valid += 1u;
        acc.correct += al == am ? 1u : 0u;
    }
}

// the four per-workgroup partials of workgroup b live at part[b], part[nblk + b], part[2 nblk + b], part[3 nblk + b] (8 bytes each)
__device__ __forceinline__ void write_partials(const Sums& acc, void* part) {
    __shared__ double sL[WG / 64], sW[WG / 64];
    __shared__ u64 sC[WG / 64], sV[WG / 64];
    double l = acc.loss, w = acc.weight; u64 c = acc.correct, v = acc.valid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { l += __shfl_xor(l, o); w += __shfl_xor(w, o); c += __shfl_xor(c, o); v += __shfl_xor(v, o); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sL[wave] = l; sW[wave] = w; sC[wave] = c; sV[wave] = v; }
    __syncthreads();
    if (threadIdx.x == 0) {
        l = sL[0]; w = sW[0]; c = sC[0]; v = sV[0];
#pragma unroll
        for (int i = 1; i < WG / 64; ++i) { l += sL[i]; w += sW[i]; c += sC[i]; v += sV[i]; }
        const size_t nblk = gridDim.x, b = blockIdx.x;
        ((double*)part)[b] = l; ((double*)part)[nblk + b] = w;
        ((u64*)part)[2 * nblk + b] = c; ((u64*)part)[3 * nblk + b] = v;
    }
}

// K in {2, 4}, everything dense and 16-byte aligned: a lane owns 4 / K consecutive pixels = one 16-byte vector of every tensor
template <int K>
__global__ __launch_bounds__(WG) void ce_weighted_dense_kernel(const float* __restrict__ z, const int* __restrict__ lab,
        const float* __restrict__ cw, const float* __restrict__ pw, int ignore_empty, float* __restrict__ prob, float* __restrict__ dz,
        long P, float label_smoothing, float grad_scale, float clip_eps, void* __restrict__ part) {
    constexpr int PPT = 4 / K;
    Sums acc = {0.0, 0.0, 0u, 0u};
    const long nq = (P + PPT - 1) / PPT, stride = (long)gridDim.x * WG;
    const bool pw_pair = PPT == 2 && pw && (reinterpret_cast<uintptr_t>(pw) & 7u) == 0;
    for (long q = (long)blockIdx.x * WG + threadIdx.x; q < nq; q += stride) {
        const long pix0 = q * PPT;
        float zv[4], pv[4], dv[4], wv[PPT]; int lv[4];
        const bool full = pix0 + PPT <= P;                    // false only for the last pixel of an odd P at K = 2
        if (full) {
            const f32x4 fz = *reinterpret_cast<const f32x4*>(z + (size_t)pix0 * K);
            const i32x4 il = *reinterpret_cast<const i32x4*>(lab + (size_t)pix0 * K);
#pragma unroll
            for (int e = 0; e < 4; ++e) { zv[e] = fz[e]; lv[e] = il[e]; }
            if (pw_pair) {
                const f32x2 t = *reinterpret_cast<const f32x2*>(pw + pix0);
                wv[0] = t[0]; wv[PPT - 1] = t[PPT - 1];
            } else {
#pragma unroll
                for (int j = 0; j < PPT; ++j) wv[j] = pw ? pw[pix0 + j] : 1.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { zv[e] = e < K ? z[(size_t)pix0 * K + e] : 0.f; lv[e] = e < K ? lab[(size_t)pix0 * K + e] : 0; }
#pragma unroll
            for (int j = 0; j < PPT; ++j) wv[j] = (j == 0 && pw) ? pw[pix0] : 1.f;
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j)
            if (j == 0 || full)
                ce_pixel<K>(zv + j * K, lv + j * K, K, cw, wv[j], ignore_empty, pv + j * K, dv + j * K, label_smoothing, grad_scale, clip_eps, acc);
        if (full) {
            f32x4 op, od;
#pragma unroll
            for (int e = 0; e < 4; ++e) { op[e] = pv[e]; od[e] = dv[e]; }
            *reinterpret_cast<f32x4*>(prob + (size_t)pix0 * K) = op;
            *reinterpret_cast<f32x4*>(dz + (size_t)pix0 * K) = od;
        } else {
#pragma unroll
            for (int e = 0; e < K; ++e) { prob[(size_t)pix0 * K + e] = pv[e]; dz[(size_t)pix0 * K + e] = dv[e]; }
        }
    }
    write_partials(acc, part);
}

__global__ __launch_bounds__(WG) void ce_weighted_generic_kernel(const float* __restrict__ z, int ldz, const int* __restrict__ lab,
        const float* __restrict__ cw, const float* __restrict__ pw, int ignore_empty, float* __restrict__ prob, float* __restrict__ dz, int lddz,
        long P, int K, float label_smoothing, float grad_scale, float clip_eps, void* __restrict__ part) {
    Sums acc = {0.0, 0.0, 0u, 0u};
    const long stride = (long)gridDim.x * WG;
    for (long pix = (long)blockIdx.x * WG + threadIdx.x; pix < P; pix += stride)
        ce_pixel<0>(z + (size_t)pix * ldz, lab ? lab + (size_t)pix * K : nullptr, K, cw, pw ? pw[pix] : 1.f, ignore_empty,
                    prob ? prob + (size_t)pix * K : nullptr, dz ? dz + (size_t)pix * lddz : nullptr, label_smoothing, grad_scale, clip_eps, acc);
    write_partials(acc, part);
}

// one wave: lane i adds the partials [i * chunk, (i + 1) * chunk) in index order, then neighbouring lanes combine (1, 2, 4, .. 32 apart): a
// fixed order for a given nblk.  out = [loss, correct, valid, weight_sum]
__global__ __launch_bounds__(64) void ce_weighted_finalize_kernel(const void* __restrict__ part, int nblk, float loss_scale, float* __restrict__ out) {
    const double *pl = (const double*)part, *pw = pl + nblk;
    const u64 *pc = (const u64*)part + 2 * (size_t)nblk, *pv = pc + nblk;
    const int chunk = (nblk + 63) / 64, b0 = threadIdx.x * chunk, b1 = b0 + chunk < nblk ? b0 + chunk : nblk;
    double l = 0.0, w = 0.0; u64 c = 0, v = 0;
    for (int b = b0; b < b1; ++b) { l += pl[b]; w += pw[b]; c += pc[b]; v += pv[b]; }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { l += __shfl_xor(l, o); w += __shfl_xor(w, o); c += __shfl_xor(c, o); v += __shfl_xor(v, o); }
    if (threadIdx.x == 0) {
        out[0] = (float)(l * (double)loss_scale);
        out[1] = (float)c; out[2] = (float)v; out[3] = (float)w;
    }
}

// unet_labels_onehot's kernel (misc.hip) with one class-map value that means "unlabeled": a zero row, not counted as out of range
__global__ __launch_bounds__(WG) void onehot_ignore_kernel(const uint8_t* __restrict__ cls, int* __restrict__ onehot, long P, int K, int ignore_label,
                                                           unsigned* __restrict__ bad) {
    const long total = P * K, stride = (long)gridDim.x * WG;
    unsigned nbad = 0;
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i < total; i += stride) {
        const long px = i / K; const int k = (int)(i - px * K);
        const int c = cls[px];
        const bool ignored = c == ignore_label;
        onehot[i] = (c == k && !ignored) ? 1 : 0;
        if (k == 0 && c >= K && !ignored) ++nbad;
    }
    if (nbad && bad) atomicAdd(bad, nbad);
}

int grid_for(long total, int cap) { long b = (total + WG - 1) / WG; if (b > cap) b = cap; if (b < 1) b = 1; return (int)b; }

}  // namespace

// room for the 4 x 8-byte partials of every workgroup of the widest grid (the generic path's)
extern "C" size_t unet_softmax_ce_weighted_workspace(long P) { return (size_t)grid_for(P, 1024) * 32; }

// labels_onehot, prob, dlogits, class_weight, pixel_weight and stats_out may each be null; weights and ignore_empty need the labels
extern "C" int unet_softmax_ce_weighted(const float* logits, int ldz, const int* labels_onehot, const float* class_weight,
        const float* pixel_weight, int ignore_empty, float* prob, float* dlogits, int lddz, long P, int K, float label_smoothing,
        float loss_scale, float grad_scale, float ce_clip_eps, float* stats_out, void* ws, size_t ws_bytes, void* stream) {
    UNET_CHECK_ARG(logits && ws && P > 0 && K > 0 && ldz >= K && (!dlogits || (labels_onehot && lddz >= K)));
    UNET_CHECK_ARG(ce_clip_eps >= 0.f && ce_clip_eps < 0.5f);
    UNET_CHECK_ARG(!stats_out || labels_onehot);
    UNET_CHECK_ARG((!class_weight && !pixel_weight && !ignore_empty) || labels_onehot);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0);
    if (ws_bytes < unet_softmax_ce_weighted_workspace(P)) return UNET_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const bool dense = (K == 2 || K == 4) && ldz == K && lddz == K && labels_onehot && prob && dlogits && unet_aligned16(logits) &&
                       unet_aligned16(labels_onehot) && unet_aligned16(prob) && unet_aligned16(dlogits);
    int nblk;
    if (dense && K == 2) {
        nblk = grid_for((P + 1) / 2, 1024);
        ce_weighted_dense_kernel<2><<<nblk, WG, 0, st>>>(logits, labels_onehot, class_weight, pixel_weight, ignore_empty, prob, dlogits, P,
                                                        label_smoothing, grad_scale, ce_clip_eps, ws);
    } else if (dense) {
        nblk = grid_for(P, 1024);
        ce_weighted_dense_kernel<4><<<nblk, WG, 0, st>>>(logits, labels_onehot, class_weight, pixel_weight, ignore_empty, prob, dlogits, P,
                                                        label_smoothing, grad_scale, ce_clip_eps, ws);
    } else {
        nblk = grid_for(P, 1024);
        ce_weighted_generic_kernel<<<nblk, WG, 0, st>>>(logits, ldz, labels_onehot, class_weight, pixel_weight, ignore_empty, prob, dlogits, lddz,
                                                       P, K, label_smoothing, grad_scale, ce_clip_eps, ws);
    }
    int rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    if (stats_out) {
        ce_weighted_finalize_kernel<<<1, 64, 0, st>>>(ws, nblk, loss_scale, stats_out);
        rc = UNET_LAUNCH_STATUS();
    }
    return rc;
}

extern "C" int unet_labels_onehot_ignore(const uint8_t* classmap, int* onehot, long P, int K, int ignore_label, unsigned* out_of_range,
                                         void* stream) {
    UNET_CHECK_ARG(classmap && onehot && P > 0 && K > 0 && K <= 256);
    onehot_ignore_kernel<<<grid_for(P * K, 4096), WG, 0, (hipStream_t)stream>>>(classmap, onehot, P, K, ignore_label, out_of_range);
    return UNET_LAUNCH_STATUS();
}
