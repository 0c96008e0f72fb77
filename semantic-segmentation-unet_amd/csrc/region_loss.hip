// Region term of the training loss: soft Tversky index per image and class (alpha = beta = 0.5: soft Dice), added to the cross-entropy that
// unet_softmax_ce / unet_softmax_ce_weighted computed.  With p = the softmax those kernels wrote, y = the hard one-hot row (first maximum of
// the label row; an all-zero row is class 0, or with ignore_empty an unlabeled pixel that enters nothing) and the sums over the labeled
// pixels of image n only:
//   I_nk = sum p_k y_k,  S_nk = sum p_k,  Y_nk = sum y_k,   D_nk = (1 - a - b) I_nk + a S_nk + b Y_nk + s,   T_nk = (I_nk + s) / D_nk
//   region = scale * sum_n sum_k c~_k (1 - T_nk),            c~_k = class_weight[k] / sum_j class_weight[j]  (NULL: 1 / K)
//   d region / d p_pk = coef[n][k][0] * y_pk + coef[n][k][1],  coef = (-scale c~_k A_nk, -scale c~_k B_nk),
//       A_nk = 1 / D - (I + s)(1 - a - b) / D^2,   B_nk = -a (I + s) / D^2
//   dlogits[p][j] += p_j (g_j - sum_k p_k g_k)             (unlabeled rows are not touched: they stay the +0.0 the CE kernel stored)
//
// HBM-bound.  unet_region_loss_sums: one pass over prob and labels (16 B per pixel at K = 2), then a one-workgroup finalize launch;
// unet_region_loss_bwd: one read-modify-write pass over dlogits (32 B per pixel at K = 2).  Paths, as in loss.hip:
//   dense    K in {2, 4}, ldp == (lddz ==) K, every image's first row 16-byte aligned in every tensor: one 16-byte access per tensor and lane
//            (two pixels at K = 2 -- HW must be even, which also keeps every image's first row aligned --, one at K = 4);
//   generic  every other K <= REGION_MAX_K, leading dimension or alignment: one pixel per lane.
// Work is cut into SLOTS: slot (n, b) is the b-th of bpi = min(ceil(units per image / 256), 256) workgroup shares of image n, so a workgroup
// never straddles two images and bpi -- hence the grouping of every sum -- depends on the image size alone, not on N: an image's sums, and
// with them its dlogits rows, are the same bits whichever batch it arrives in.  The grid is min(N * bpi, 1024) workgroups that stride over
// the slots.  Reductions: per lane in double, per wave by shuffles, per workgroup through LDS in wave order; one partial triple per slot and
// class in the workspace; the finalize kernel adds a (n, k) pair's partials in a fixed order with one wave.  No floating-point atomics:
// the result does not depend on launch order and is the same bits run after run.
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WG = 256;
constexpr int MAX_BPI = 256;          // workgroup shares per image
constexpr int MAX_GRID = 1024;
constexpr int REGION_MAX_K = 32;      // the generic sums kernel keeps 2 doubles + 1 count per class and lane: 160 VGPRs at 32, no scratch

template <int KC> struct Acc { double I[KC], S[KC]; unsigned Y[KC]; };

// first maximum of the one-hot row; false: the pixel is unlabeled and ignored
template <int KC>
__device__ __forceinline__ bool truth_of(const int* lp, int K, int ignore_empty, int& t) {
    int lbest = lp[0]; t = 0;
#pragma unroll
    for (int k = 1; k < KC; ++k)
        if (k < K) { const int li = lp[k]; if (li > lbest) { lbest = li; t = k; } }
    return !(ignore_empty && lbest <= 0);
}

// KC = 0: K at run time, no unrolled form (the generic backward)
template <>
__device__ __forceinline__ bool truth_of<0>(const int* lp, int K, int ignore_empty, int& t) {
    int lbest = lp[0]; t = 0;
    for (int k = 1; k < K; ++k) { const int li = lp[k]; if (li > lbest) { lbest = li; t = k; } }
    return !(ignore_empty && lbest <= 0);
}

template <int KC>
__device__ __forceinline__ void sum_pixel(const float* pp, const int* lp, int K, int ignore_empty, Acc<KC>& a) {
    int t;
    if (!truth_of<KC>(lp, K, ignore_empty, t)) return;
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if (k < K) {
            const double pk = (double)pp[k];
            a.S[k] += pk;
            if (k == t) { a.I[k] += pk; a.Y[k] += 1u; }
        }
}

// the partial triple of slot (n, b) and class k lives at part[((n K + k) 3 + c) bpi + b], c = 0 (I), 1 (S), 2 (Y); all doubles (counts are
// exact in a double)
template <int KC>
__device__ __forceinline__ void write_partials(const Acc<KC>& a, int K, double* __restrict__ part, int n, int b, int bpi) {
    __shared__ double sh[WG / 64][KC * 3];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if (k < K) {
            double i = a.I[k], s = a.S[k], y = (double)a.Y[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { i += __shfl_xor(i, o); s += __shfl_xor(s, o); y += __shfl_xor(y, o); }
            if ((threadIdx.x & 63) == 0) { sh[wave][k * 3] = i; sh[wave][k * 3 + 1] = s; sh[wave][k * 3 + 2] = y; }
        }
    __syncthreads();
    if ((int)threadIdx.x < K * 3) {
        double v = sh[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WG / 64; ++w) v += sh[w][threadIdx.x];
        part[((size_t)n * K * 3 + threadIdx.x) * bpi + b] = v;
    }
    __syncthreads();                 // sh is written again by the workgroup's next slot
}

template <int K>
__global__ __launch_bounds__(WG) void region_sums_dense_kernel(const float* __restrict__ prob, const int* __restrict__ lab, int ignore_empty,
        int N, long HW, int bpi, double* __restrict__ part) {
    constexpr int PPT = 4 / K;
    const long units = HW / PPT, nslot = (long)N * bpi;
    for (long slot = blockIdx.x; slot < nslot; slot += gridDim.x) {
        const int n = (int)(slot / bpi), b = (int)(slot - (long)n * bpi);
        Acc<K> acc;
#pragma unroll
        for (int k = 0; k < K; ++k) { acc.I[k] = 0.0; acc.S[k] = 0.0; acc.Y[k] = 0u; }
        const size_t img = (size_t)n * HW * K;
        for (long u = (long)b * WG + threadIdx.x; u < units; u += (long)bpi * WG) {
            const f32x4 fp = *reinterpret_cast<const f32x4*>(prob + img + (size_t)u * 4);
            const i32x4 il = *reinterpret_cast<const i32x4*>(lab + img + (size_t)u * 4);
            float pv[4]; int lv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { pv[e] = fp[e]; lv[e] = il[e]; }
#pragma unroll
            for (int j = 0; j < PPT; ++j) sum_pixel<K>(pv + j * K, lv + j * K, K, ignore_empty, acc);
        }
        write_partials<K>(acc, K, part, n, b, bpi);
    }
}

template <int KC>
__global__ __launch_bounds__(WG) void region_sums_generic_kernel(const float* __restrict__ prob, int ldp, const int* __restrict__ lab,
        int ignore_empty, int N, long HW, int K, int bpi, double* __restrict__ part) {
    const long nslot = (long)N * bpi;
    for (long slot = blockIdx.x; slot < nslot; slot += gridDim.x) {
        const int n = (int)(slot / bpi), b = (int)(slot - (long)n * bpi);
        Acc<KC> acc;
#pragma unroll
        for (int k = 0; k < KC; ++k) { acc.I[k] = 0.0; acc.S[k] = 0.0; acc.Y[k] = 0u; }
        const size_t pix0 = (size_t)n * HW;
        for (long u = (long)b * WG + threadIdx.x; u < HW; u += (long)bpi * WG)
            sum_pixel<KC>(prob + (pix0 + u) * ldp, lab + (pix0 + u) * K, K, ignore_empty, acc);
        write_partials<KC>(acc, K, part, n, b, bpi);
    }
}

// One workgroup.  Wave w takes the pairs (n, k) = w, w + 4, ..: lane i adds the partials i, i + 64, .. in index order, then lanes combine
// 1, 2, 4, .. 32 apart: a fixed order for a given bpi.  T_nk goes to tbuf (workspace, behind the partials); wave 0 then adds each class's
// T over the images the same way.
__global__ __launch_bounds__(WG) void region_finalize_kernel(const double* __restrict__ part, int bpi, int N, int K, float alpha, float beta,
        float smooth, float scale, const float* __restrict__ cw, float* __restrict__ coef, float* __restrict__ stats, double* __restrict__ tbuf) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double csum = cw ? 0.0 : (double)K;
    if (cw) for (int k = 0; k < K; ++k) csum += (double)cw[k];
    const double a = (double)alpha, be = (double)beta, s = (double)smooth, sc = (double)scale, r = 1.0 - a - be;
    for (int pair = wave; pair < N * K; pair += WG / 64) {
        const double* p = part + (size_t)pair * 3 * bpi;
        double I = 0.0, S = 0.0, Y = 0.0;
        for (int b = lane; b < bpi; b += 64) { I += p[b]; S += p[bpi + b]; Y += p[2 * bpi + b]; }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { I += __shfl_xor(I, o); S += __shfl_xor(S, o); Y += __shfl_xor(Y, o); }
        if (lane == 0) {
            const int k = pair % K;
            const double ct = (cw ? (double)cw[k] : 1.0) / csum;
            const double D = r * I + a * S + be * Y + s, num = I + s;
            const double A = 1.0 / D - num * r / (D * D), B = -a * num / (D * D);
            coef[2 * pair] = (float)(-sc * ct * A);
            coef[2 * pair + 1] = (float)(-sc * ct * B);
            tbuf[pair] = num / D;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double loss = 0.0;
        for (int k = 0; k < K; ++k) {
            double t = 0.0, u = 0.0;
            for (int n = lane; n < N; n += 64) { const double T = tbuf[(size_t)n * K + k]; t += T; u += 1.0 - T; }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { t += __shfl_xor(t, o); u += __shfl_xor(u, o); }
            loss += (cw ? (double)cw[k] : 1.0) / csum * u;
            if (lane == 0) stats[1 + k] = (float)(t / (double)N);
        }
        if (lane == 0) stats[0] = (float)(sc * loss);
    }
}

// dz row += p_j (g_j - sum_k p_k g_k), g_k = coef[k][0] y_k + coef[k][1]; an addend of zero leaves the stored bits (also a -0.0) alone
template <int KC>
__device__ __forceinline__ void bwd_pixel(const float* pp, const int* lp, int K, int ignore_empty, const float* __restrict__ cf,
                                          const float* dzin, float* dzout) {
    int t;
    if (!truth_of<KC>(lp, K, ignore_empty, t)) {
        if (KC != 0 && dzin != dzout) for (int k = 0; k < KC; ++k) dzout[k] = dzin[k];
        return;
    }
    float dot = 0.f;
    if constexpr (KC != 0) {
#pragma unroll
        for (int k = 0; k < KC; ++k) { const float g = k == t ? cf[2 * k] + cf[2 * k + 1] : cf[2 * k + 1]; dot += pp[k] * g; }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float g = k == t ? cf[2 * k] + cf[2 * k + 1] : cf[2 * k + 1];
            const float add = pp[k] * (g - dot);
            dzout[k] = add == 0.f ? dzin[k] : dzin[k] + add;
        }
    } else {
        for (int k = 0; k < K; ++k) { const float g = k == t ? cf[2 * k] + cf[2 * k + 1] : cf[2 * k + 1]; dot += pp[k] * g; }
        for (int k = 0; k < K; ++k) {
            const float g = k == t ? cf[2 * k] + cf[2 * k + 1] : cf[2 * k + 1];
            const float add = pp[k] * (g - dot);
            if (add != 0.f) dzout[k] = dzin[k] + add;
        }
    }
}

template <int K>
__global__ __launch_bounds__(WG) void region_bwd_dense_kernel(const float* __restrict__ prob, const int* __restrict__ lab, int ignore_empty,
        const float* __restrict__ coef, float* __restrict__ dz, int N, long HW, int bpi) {
    constexpr int PPT = 4 / K;
    const long units = HW / PPT, nslot = (long)N * bpi;
    for (long slot = blockIdx.x; slot < nslot; slot += gridDim.x) {
        const int n = (int)(slot / bpi), b = (int)(slot - (long)n * bpi);
        float cf[2 * K];
#pragma unroll
        for (int e = 0; e < 2 * K; ++e) cf[e] = coef[(size_t)n * K * 2 + e];
        const size_t img = (size_t)n * HW * K;
        for (long u = (long)b * WG + threadIdx.x; u < units; u += (long)bpi * WG) {
            const f32x4 fp = *reinterpret_cast<const f32x4*>(prob + img + (size_t)u * 4);
            const i32x4 il = *reinterpret_cast<const i32x4*>(lab + img + (size_t)u * 4);
            const f32x4 fd = *reinterpret_cast<const f32x4*>(dz + img + (size_t)u * 4);
            float pv[4], dv[4], ov[4]; int lv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { pv[e] = fp[e]; lv[e] = il[e]; dv[e] = fd[e]; }
#pragma unroll
            for (int j = 0; j < PPT; ++j) bwd_pixel<K>(pv + j * K, lv + j * K, K, ignore_empty, cf, dv + j * K, ov + j * K);
            f32x4 od;
#pragma unroll
            for (int e = 0; e < 4; ++e) od[e] = ov[e];
            *reinterpret_cast<f32x4*>(dz + img + (size_t)u * 4) = od;
        }
    }
}

__global__ __launch_bounds__(WG) void region_bwd_generic_kernel(const float* __restrict__ prob, int ldp, const int* __restrict__ lab,
        int ignore_empty, const float* __restrict__ coef, float* __restrict__ dz, int lddz, int N, long HW, int K, int bpi) {
    const long nslot = (long)N * bpi;
    for (long slot = blockIdx.x; slot < nslot; slot += gridDim.x) {
        const int n = (int)(slot / bpi), b = (int)(slot - (long)n * bpi);
        const size_t pix0 = (size_t)n * HW;
        const float* cf = coef + (size_t)n * K * 2;
        for (long u = (long)b * WG + threadIdx.x; u < HW; u += (long)bpi * WG) {
            float* d = dz + (pix0 + u) * lddz;
            bwd_pixel<0>(prob + (pix0 + u) * ldp, lab + (pix0 + u) * K, K, ignore_empty, cf, d, d);
        }
    }
}

int bpi_for(long units) { long b = (units + WG - 1) / WG; if (b > MAX_BPI) b = MAX_BPI; if (b < 1) b = 1; return (int)b; }
int grid_for(int N, int bpi) { const long s = (long)N * bpi; return (int)(s < MAX_GRID ? s : MAX_GRID); }

}  // namespace

// the generic path's partials (one pixel per lane: the larger bpi) + one T per image and class
extern "C" size_t unet_region_loss_workspace(int N, long HW, int K) {
    if (N <= 0 || HW <= 0 || K <= 0) return 0;
    return ((size_t)N * K * 3 * bpi_for(HW) + (size_t)N * K) * sizeof(double);
}

extern "C" int unet_region_loss_sums(const float* prob, int ldp, const int* labels_onehot, int ignore_empty, int N, long HW, int K, float alpha,
        float beta, float smooth, float scale, const float* class_weight, float* coef_out, float* stats_out, void* ws, size_t ws_bytes,
        void* stream) {
    UNET_CHECK_ARG(prob && labels_onehot && coef_out && stats_out && ws && N > 0 && HW > 0 && K > 0 && K <= REGION_MAX_K && ldp >= K);
    UNET_CHECK_ARG(smooth > 0.f && alpha >= 0.f && beta >= 0.f);                 // (a NaN fails each)
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0);
    if (ws_bytes < unet_region_loss_workspace(N, HW, K)) return UNET_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    const bool dense = (K == 2 || K == 4) && ldp == K && (K == 4 || HW % 2 == 0) && unet_aligned16(prob) && unet_aligned16(labels_onehot);
    int bpi;
    if (dense && K == 2) {
        bpi = bpi_for(HW / 2);
        region_sums_dense_kernel<2><<<grid_for(N, bpi), WG, 0, st>>>(prob, labels_onehot, ignore_empty, N, HW, bpi, part);
    } else if (dense) {
        bpi = bpi_for(HW);
        region_sums_dense_kernel<4><<<grid_for(N, bpi), WG, 0, st>>>(prob, labels_onehot, ignore_empty, N, HW, bpi, part);
    } else if (K <= 8) {
        bpi = bpi_for(HW);
        region_sums_generic_kernel<8><<<grid_for(N, bpi), WG, 0, st>>>(prob, ldp, labels_onehot, ignore_empty, N, HW, K, bpi, part);
    } else {
        bpi = bpi_for(HW);
        region_sums_generic_kernel<REGION_MAX_K><<<grid_for(N, bpi), WG, 0, st>>>(prob, ldp, labels_onehot, ignore_empty, N, HW, K, bpi, part);
    }
    int rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    region_finalize_kernel<<<1, WG, 0, st>>>(part, bpi, N, K, alpha, beta, smooth, scale, class_weight, coef_out, stats_out,
                                            part + (size_t)N * K * 3 * bpi);
    return UNET_LAUNCH_STATUS();
}

extern "C" int unet_region_loss_bwd(const float* prob, int ldp, const int* labels_onehot, int ignore_empty, const float* coef, float* dlogits,
        int lddz, int N, long HW, int K, void* stream) {
    UNET_CHECK_ARG(prob && labels_onehot && coef && dlogits && N > 0 && HW > 0 && K > 0 && K <= REGION_MAX_K && ldp >= K && lddz >= K);
    hipStream_t st = (hipStream_t)stream;
    const bool dense = (K == 2 || K == 4) && ldp == K && lddz == K && (K == 4 || HW % 2 == 0) && unet_aligned16(prob) &&
                       unet_aligned16(labels_onehot) && unet_aligned16(dlogits);
    if (dense && K == 2) {
        const int bpi = bpi_for(HW / 2);
        region_bwd_dense_kernel<2><<<grid_for(N, bpi), WG, 0, st>>>(prob, labels_onehot, ignore_empty, coef, dlogits, N, HW, bpi);
    } else if (dense) {
        const int bpi = bpi_for(HW);
        region_bwd_dense_kernel<4><<<grid_for(N, bpi), WG, 0, st>>>(prob, labels_onehot, ignore_empty, coef, dlogits, N, HW, bpi);
    } else {
        const int bpi = bpi_for(HW);
        region_bwd_generic_kernel<<<grid_for(N, bpi), WG, 0, st>>>(prob, ldp, labels_onehot, ignore_empty, coef, dlogits, lddz, N, HW, K, bpi);
    }
    return UNET_LAUNCH_STATUS();
}
