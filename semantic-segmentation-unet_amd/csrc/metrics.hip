// Per-class segmentation metrics on the device: the K x K confusion matrix cm[truth][prediction] (unsigned 64-bit counts) that per-class
// IoU / Dice / precision / recall are derived from on the host (metrics.py).  Two producers, both ACCUMULATING into the caller's matrix:
//   unet_confusion_scores  class scores [P][lds] + one-hot labels [P][K] (the eval / train step: logits and labels are on the device)
//   unet_confusion_scores_valid  the same with unlabeled pixels (no positive entry in the one-hot row) counted nowhere: the pair of
//                          unet_softmax_ce_weighted(ignore_empty) (loss.hip), trace = its `correct`, sum = its `valid`
//   unet_confusion_masks   predicted class map against a ground-truth class map (whole-image inference: the mask before its download)
// The prediction is the FIRST maximum of the scores (start at class 0, replace on v > m: softmax_ce_kernel / argmax_kernel of misc.hip), the
// truth the first maximum of the one-hot row by the loop of softmax_ce_kernel, so trace(cm) is exactly the `correct_out` of unet_softmax_ce
// on the same logits and labels.  Everything is integer counting: the result does not depend on launch order or on the path taken.
//
// A histogram with very few bins: at K = 2 the 64 lanes of a wave hit one of four cells, and one atomic per pixel (LDS or memory) serialises the
// wave.  So by K:
//   K <= 4   (K^2 <= 16) no atomic in the pixel loop: per cell the wave adds popcount(ballot(cell == c)) to a wave-uniform counter; the waves
//            of a workgroup combine through LDS at the end and one thread per non-zero cell issues one 64-bit atomicAdd;
//   K <= 64  a workgroup-private LDS histogram of K^2 32-bit counters (<= 16 KB), LDS atomics, flushed once with 64-bit global atomics;
//   K > 64   64-bit global atomics per pixel (correctness only).
// Grids are sized by the pixel count (at most 1024 workgroups, like unet_softmax_ce), raised where needed so that no workgroup sees more than
// 2^31 pixels: a 32-bit counter cannot wrap.  No allocation, no globals, no environment.
#include "common.h"

namespace {

typedef unsigned long long u64;
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WG = 256;

template <int K> __device__ __forceinline__ int first_max(const float* v) {
    float m = v[0]; int am = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) if (v[k] > m) { m = v[k]; am = k; }
    return am;
}
template <int K> __device__ __forceinline__ int first_max(const int* v) {
    int m = v[0]; int am = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) if (v[k] > m) { m = v[k]; am = k; }
    return am;
}

// wave-uniform count of the lanes whose `hit` is set (every lane of the wave must get here)
__device__ __forceinline__ unsigned wave_count(bool hit) { return (unsigned)__popcll(__ballot(hit)); }

// the per-wave counters of the ballot paths -> LDS -> one 64-bit atomic per non-zero cell.  `sh` holds NC zeroed words; cell c of the
// kernel's KB-wide numbering is cm[(c / KB) * K + c % KB].
template <int NC, int KB>
__device__ __forceinline__ void flush_wave_counts(const unsigned (&cnt)[NC], unsigned* sh, u64* __restrict__ cm, int K) {
    __syncthreads();                                         // sh zeroed by the first NC threads before the loop
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) if (cnt[c]) atomicAdd(&sh[c], cnt[c]);
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < NC && sh[c]) atomicAdd(cm + (c / KB) * K + c % KB, (u64)sh[c]);
}

// ---- scores, K <= 4.  PPT pixels per thread; DENSE: lds == K and both pointers aligned to PPT * K * 4 bytes, so a thread's PPT * K scores
// (and labels) are one 8- or 16-byte load.  VALID (unet_confusion_scores_valid): a pixel whose one-hot row has no positive entry is unlabeled
// and counted nowhere.
template <int K> __device__ __forceinline__ bool any_positive(const int* v) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; ++k) any |= v[k] > 0;
    return any;
}

template <int K, int PPT, int DENSE, int VALID>
__global__ __launch_bounds__(WG) void confusion_scores_ballot_kernel(const float* __restrict__ z, int ldz, const int* __restrict__ lab, long P,
                                                                     u64* __restrict__ cm) {
    constexpr int KK = K * K, NV = PPT * K;
    __shared__ unsigned sh[KK];
    unsigned cnt[KK];
#pragma unroll
    for (int c = 0; c < KK; ++c) cnt[c] = 0;
    if (threadIdx.x < KK) sh[threadIdx.x] = 0;
    const long nq = (P + PPT - 1) / PPT, stride = (long)gridDim.x * WG;
    for (long q0 = (long)blockIdx.x * WG; q0 < nq; q0 += stride) {          // q0 is uniform over the workgroup: every wave reaches the ballots
        const long q = q0 + threadIdx.x;
        int cell[PPT];
#pragma unroll
        for (int j = 0; j < PPT; ++j) cell[j] = -1;
        if (q < nq) {
            const long pix0 = q * PPT;
            float s[NV]; int l[NV];
            int np = PPT;
            bool loaded = false;
            if constexpr (DENSE != 0 && NV > 1) {
                if (pix0 + PPT <= P) {
                    typedef float FV __attribute__((ext_vector_type(NV)));
                    typedef int IV __attribute__((ext_vector_type(NV)));
                    const FV fs = *reinterpret_cast<const FV*>(z + (size_t)pix0 * K);
                    const IV il = *reinterpret_cast<const IV*>(lab + (size_t)pix0 * K);
#pragma unroll
                    for (int e = 0; e < NV; ++e) { s[e] = fs[e]; l[e] = il[e]; }
                    loaded = true;
                }
            }
            if (!loaded) {
                if (P - pix0 < np) np = (int)(P - pix0);
#pragma unroll
                for (int j = 0; j < PPT; ++j) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        s[j * K + k] = j < np ? z[(size_t)(pix0 + j) * ldz + k] : 0.f;
                        l[j * K + k] = j < np ? lab[(size_t)(pix0 + j) * K + k] : 0;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < PPT; ++j)
                if (j < np && (VALID == 0 || any_positive<K>(l + j * K))) cell[j] = first_max<K>(l + j * K) * K + first_max<K>(s + j * K);
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
#pragma unroll
            for (int c = 0; c < KK; ++c) cnt[c] += wave_count(cell[j] == c);
        }
    }
    flush_wave_counts<KK, K>(cnt, sh, cm, K);
}

// ---- scores, K > 4: LDS histogram (use_lds, K <= 64) or global atomics
__global__ __launch_bounds__(WG) void confusion_scores_hist_kernel(const float* __restrict__ z, int ldz, const int* __restrict__ lab, long P, int K,
                                                                   u64* __restrict__ cm, int use_lds, int skip_empty) {
    extern __shared__ unsigned hist[];
    const int KK = K * K;
    if (use_lds) {
        for (int c = threadIdx.x; c < KK; c += WG) hist[c] = 0;
        __syncthreads();
    }
    const long stride = (long)gridDim.x * WG;
    for (long pix = (long)blockIdx.x * WG + threadIdx.x; pix < P; pix += stride) {
        const float* zp = z + (size_t)pix * ldz;
        float m = zp[0]; int am = 0;
        for (int k = 1; k < K; ++k) { const float v = zp[k]; if (v > m) { m = v; am = k; } }
        const int* lp = lab + (size_t)pix * K;
        int lbest = lp[0], al = 0;
        for (int k = 1; k < K; ++k) { const int li = lp[k]; if (li > lbest) { lbest = li; al = k; } }
        if (skip_empty && lbest <= 0) continue;
        const int cell = al * K + am;
        if (use_lds) atomicAdd(&hist[cell], 1u);
        else atomicAdd(cm + cell, (u64)1);
    }
    if (use_lds) {
        __syncthreads();
        for (int c = threadIdx.x; c < KK; c += WG) { const unsigned v = hist[c]; if (v) atomicAdd(cm + c, (u64)v); }
    }
}

// ---- class maps.  One thread per (row, 4 columns); element sizes are run-time (wave-uniform branches): 4 elements are one 4 / 8 / 16-byte
// load where the address allows.  sgn: 4-byte elements are int32 (a negative truth / prediction is out of range).
__device__ __forceinline__ void load4(const void* base, size_t index, int elem, int nk, int (&v)[4]) {
    if (elem == 1) {
        const uint8_t* p = (const uint8_t*)base + index;
        if (nk == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
            const unsigned t = *reinterpret_cast<const unsigned*>(p);
            v[0] = t & 255u; v[1] = (t >> 8) & 255u; v[2] = (t >> 16) & 255u; v[3] = t >> 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < nk ? (int)p[k] : 0;
        }
    } else if (elem == 2) {
        const uint16_t* p = (const uint16_t*)base + index;
        if (nk == 4 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
            const unet_u32x2 t = *reinterpret_cast<const unet_u32x2*>(p);
            v[0] = t[0] & 0xffffu; v[1] = t[0] >> 16; v[2] = t[1] & 0xffffu; v[3] = t[1] >> 16;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < nk ? (int)p[k] : 0;
        }
    } else {
        const int* p = (const int*)base + index;
        if (nk == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            const i32x4 t = *reinterpret_cast<const i32x4*>(p);
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < nk ? p[k] : 0;
        }
    }
}

// cell of one pixel in a KB-wide numbering: -1 = not counted (ignored, or out of range: then `bad` is set)
__device__ __forceinline__ int mask_cell(int t, int p, int K, int KB, int ignore_label, bool& bad) {
    bad = false;
    if (ignore_label != -1 && t == ignore_label) return -1;                 // -1 skips nothing: a truth of -1 is out of range like any negative
    if ((unsigned)t >= (unsigned)K || (unsigned)p >= (unsigned)K) { bad = true; return -1; }
    return t * KB + p;
}

// MODE 0: K <= KB in {2, 4}, ballot counting; MODE 1: LDS histogram (K <= 64); MODE 2: global atomics
template <int MODE, int KB>
__global__ __launch_bounds__(WG) void confusion_masks_kernel(const void* __restrict__ pred, int pe, long ppitch, const void* __restrict__ truth, int te,
        long tpitch, int H, int W, int K, int ignore_label, u64* __restrict__ cm, u64* __restrict__ oor) {
    constexpr int NC = MODE == 0 ? KB * KB : 1;
    extern __shared__ unsigned hist[];
    __shared__ unsigned sh[NC];
    __shared__ unsigned sbad;
    unsigned cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = 0;
    unsigned nbad = 0;                                       // wave-uniform
    if (threadIdx.x < NC) sh[threadIdx.x] = 0;
    if (threadIdx.x == 0) sbad = 0;
    if (MODE == 1) for (int c = threadIdx.x; c < K * K; c += WG) hist[c] = 0;
    __syncthreads();
    const int nq = (W + 3) / 4;
    const long total = (long)H * nq, stride = (long)gridDim.x * WG;
    for (long i0 = (long)blockIdx.x * WG; i0 < total; i0 += stride) {       // uniform over the workgroup
        const long i = i0 + threadIdx.x;
        int cell[4] = {-1, -1, -1, -1};
        bool bad[4] = {false, false, false, false};
        if (i < total) {
            const int r = (int)(i / nq), c = (int)(i - (long)r * nq) * 4;
            const int nk = W - c < 4 ? W - c : 4;
            int pv[4], tv[4];
            load4(pred, (size_t)r * ppitch + c, pe, nk, pv);
            load4(truth, (size_t)r * tpitch + c, te, nk, tv);
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < nk) cell[k] = mask_cell(tv[k], pv[k], K, MODE == 0 ? KB : K, ignore_label, bad[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nbad += wave_count(bad[k]);
            if (MODE == 0) {
#pragma unroll
                for (int c = 0; c < NC; ++c) cnt[c] += wave_count(cell[k] == c);
            } else if (cell[k] >= 0) {
                if (MODE == 1) atomicAdd(&hist[cell[k]], 1u);
                else atomicAdd(cm + cell[k], (u64)1);
            }
        }
    }
    if (MODE == 0) flush_wave_counts<NC, KB>(cnt, sh, cm, K);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(&sbad, nbad);
    __syncthreads();
    if (MODE == 1) for (int c = threadIdx.x; c < K * K; c += WG) { const unsigned v = hist[c]; if (v) atomicAdd(cm + c, (u64)v); }
    if (threadIdx.x == 0 && sbad && oor) atomicAdd(oor, (u64)sbad);
}

// workgroups for `items` thread-items covering `pixels` pixels: by the item count, at most 1024, more only to keep every workgroup's share
// of the pixels <= 2^31
int grid_counting(long items, long pixels) {
    long b = (items + WG - 1) / WG;
    if (b > 1024) b = 1024;
    const long need = (pixels + (1L << 31) - 1) >> 31;
    if (b < need) b = need;
    return (int)(b < 1 ? 1 : b);
}

bool aligned_to(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

template <int K, int VALID>
int launch_scores_ballot(const float* z, int ldz, const int* lab, long P, u64* cm, hipStream_t st) {
    if constexpr (K == 2) {
        if (ldz == 2 && aligned_to(z, 16) && aligned_to(lab, 16) && P >= 2) {
            confusion_scores_ballot_kernel<2, 2, 1, VALID><<<grid_counting((P + 1) / 2, P), WG, 0, st>>>(z, ldz, lab, P, cm);
            return UNET_LAUNCH_STATUS();
        }
        if (ldz == 2 && aligned_to(z, 8) && aligned_to(lab, 8)) {
            confusion_scores_ballot_kernel<2, 1, 1, VALID><<<grid_counting(P, P), WG, 0, st>>>(z, ldz, lab, P, cm);
            return UNET_LAUNCH_STATUS();
        }
    }
    if constexpr (K == 4) {
        if (ldz == 4 && aligned_to(z, 16) && aligned_to(lab, 16)) {
            confusion_scores_ballot_kernel<4, 1, 1, VALID><<<grid_counting(P, P), WG, 0, st>>>(z, ldz, lab, P, cm);
            return UNET_LAUNCH_STATUS();
        }
    }
    confusion_scores_ballot_kernel<K, 1, 0, VALID><<<grid_counting(P, P), WG, 0, st>>>(z, ldz, lab, P, cm);
    return UNET_LAUNCH_STATUS();
}

template <int VALID>
int confusion_scores(const float* scores, int lds, const int* labels_onehot, long P, int K, void* cmv, void* stream) {
    UNET_CHECK_ARG(scores && labels_onehot && cmv && P > 0 && K >= 1 && K <= 1024 && lds >= K);
    UNET_CHECK_ARG(aligned_to(scores, 4) && aligned_to(labels_onehot, 4) && aligned_to(cmv, 8));
    u64* cm = (u64*)cmv;
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
        case 1: return launch_scores_ballot<1, VALID>(scores, lds, labels_onehot, P, cm, st);
        case 2: return launch_scores_ballot<2, VALID>(scores, lds, labels_onehot, P, cm, st);
        case 3: return launch_scores_ballot<3, VALID>(scores, lds, labels_onehot, P, cm, st);
        case 4: return launch_scores_ballot<4, VALID>(scores, lds, labels_onehot, P, cm, st);
        default: break;
    }
    const int use_lds = K <= 64;
    confusion_scores_hist_kernel<<<grid_counting(P, P), WG, use_lds ? (size_t)K * K * 4 : 0, st>>>(scores, lds, labels_onehot, P, K, cm, use_lds, VALID);
    return UNET_LAUNCH_STATUS();
}

}  // namespace

extern "C" int unet_confusion_scores(const float* scores, int lds, const int* labels_onehot, long P, int K, void* cmv, void* stream) {
    return confusion_scores<0>(scores, lds, labels_onehot, P, K, cmv, stream);
}

// the same counting with unlabeled pixels (no positive entry in the one-hot row) skipped: the pair of unet_softmax_ce_weighted(ignore_empty)
extern "C" int unet_confusion_scores_valid(const float* scores, int lds, const int* labels_onehot, long P, int K, void* cmv, void* stream) {
    return confusion_scores<1>(scores, lds, labels_onehot, P, K, cmv, stream);
}

extern "C" int unet_confusion_masks(const void* pred, int pred_elem, long pred_pitch, const void* truth, int truth_elem, long truth_pitch,
                                    int H, int W, int K, int ignore_label, void* cmv, void* out_of_range, void* stream) {
    UNET_CHECK_ARG(pred && truth && cmv && H > 0 && W > 0 && K >= 1 && K <= 1024 && pred_pitch >= W && truth_pitch >= W);
    UNET_CHECK_ARG((pred_elem == 1 || pred_elem == 4) && (truth_elem == 1 || truth_elem == 2 || truth_elem == 4));
    UNET_CHECK_ARG(aligned_to(pred, (unsigned)pred_elem) && aligned_to(truth, (unsigned)truth_elem) && aligned_to(cmv, 8) && aligned_to(out_of_range, 8));
    u64 *cm = (u64*)cmv, *oor = (u64*)out_of_range;
    hipStream_t st = (hipStream_t)stream;
    const int g = grid_counting((long)H * ((W + 3) / 4), (long)H * W);
    if (K <= 2)       confusion_masks_kernel<0, 2><<<g, WG, 0, st>>>(pred, pred_elem, pred_pitch, truth, truth_elem, truth_pitch, H, W, K, ignore_label, cm, oor);
    else if (K <= 4)  confusion_masks_kernel<0, 4><<<g, WG, 0, st>>>(pred, pred_elem, pred_pitch, truth, truth_elem, truth_pitch, H, W, K, ignore_label, cm, oor);
    else if (K <= 64) confusion_masks_kernel<1, 1><<<g, WG, (size_t)K * K * 4, st>>>(pred, pred_elem, pred_pitch, truth, truth_elem, truth_pitch, H, W, K, ignore_label, cm, oor);
    else              confusion_masks_kernel<2, 1><<<g, WG, 0, st>>>(pred, pred_elem, pred_pitch, truth, truth_elem, truth_pitch, H, W, K, ignore_label, cm, oor);
    return UNET_LAUNCH_STATUS();
}
