// Element-wise expressions shared by the kernels at the two full-resolution ends of the network (norm.hip, conv_direct.hip).
// A kernel that materialises one of these tensors and a kernel that forms it on load call the SAME function, so the two paths agree bit
// for bit (same operations, same fma contraction):
//   unet_bn_y          y  of BatchNorm apply                      (bn_apply_kernel | the class-map forward / weight gradient reading r)
//   unet_classmap_dy   dy of the class map's input gradient       (conv1x1 dgrad kernels | BatchNorm backward of the layer in front of it)
//   unet_bn_bwd_coef / unet_bn_bwd_dz   dz of BatchNorm backward  (bn_bwd_apply_kernel and its class-map form)
#pragma once
#include "common.h"

// y = scale * r + shift (UNet/model.py:36)
__device__ __forceinline__ float unet_bn_y(float scale, float r, float shift) { return fmaf(scale, r, shift); }

// dy[c] = sum_k dz[k] * w[c][k] of Conv2D(1x1) (UNet/model.py:136): g = the pixel's K class gradients, w = row c of the [Cin][K] kernel;
// terms in class order, the first added to zero
__device__ __forceinline__ float unet_classmap_dy_term(float acc, float g, float w) { return fmaf(g, w, acc); }
template <int KK> __device__ __forceinline__ float unet_classmap_dy(const float (&g)[KK], const float (&w)[KK], int K) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) if (k < K) acc = unet_classmap_dy_term(acc, g[k], w[k]);
    return acc;
}

// BatchNorm backward as two FMAs per element: dz = relu'(r) * (A * dy + B * r + K).  With a = gamma * invstd, c1 = dbeta / P, c2 = dgamma / P:
// A = a, B = -a * c2 * invstd, K = a * (c2 * invstd * mean - c1)
__device__ __forceinline__ void unet_bn_bwd_coef(float gamma, float invstd, float mean, float dgamma, float dbeta, float invP,
                                                 float& A, float& B, float& K) {
    const float a = gamma * invstd, c1 = dbeta * invP, c2 = dgamma * invP;
    A = a; B = -(a * (c2 * invstd)); K = a * (c2 * invstd * mean - c1);
}
__device__ __forceinline__ float unet_bn_bwd_dz(float A, float B, float K, float dy, float r, int relu) {
    float d = fmaf(A, dy, fmaf(B, r, K));
    if (relu && !(r > 0.f)) d = 0.f;
    return d;
}
