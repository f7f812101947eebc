// Ray formation for one (image, pixel) pick, shared by the get-rays kernels
// (train.hip) and the batch sampler (sample.hip): the callers run the same
// code under the same contraction policy, so the same pick gives the same bits
// whichever entry formed it.
//
// train_ml.py:84-96 + datasets/ray_utils.py:45-70 (get_rays): rays_d = R dir,
// rays_o = T, imgs_d = R mean_dir.  The 3x3 rotation is applied as three dot
// products in (x, y, z) order.
#pragma once
#include "rn_common.h"
#pragma clang fp contract(off)

// P: the pick's (3, 4) row-major pose; d: its camera-space direction; row r of
// the outputs is written (imgs_d may be NULL)
__device__ __forceinline__ void rn_rays_plain(int64_t r, const float* __restrict__ P,
                                              const float* __restrict__ d,
                                              const float* __restrict__ mean_dir,
                                              float* __restrict__ rays_o,
                                              float* __restrict__ rays_d,
                                              float* __restrict__ imgs_d) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rays_d[3 * r + i] = d[0] * P[4 * i] + d[1] * P[4 * i + 1] + d[2] * P[4 * i + 2];
        rays_o[3 * r + i] = P[4 * i + 3];
        if (imgs_d)
            imgs_d[3 * r + i] = mean_dir[0] * P[4 * i] + mean_dir[1] * P[4 * i + 1] +
                                mean_dir[2] * P[4 * i + 2];
    }
}

// ---- pose refinement (--optimize_ext: train_ml.py:90-93, ray_utils.py:73-100)
// Rodrigues coefficients of A(v) = I + a K + b K^2 at theta = |v| + 1e-7 and
// their derivatives in theta.  fp32: below theta = 1e-2 the closed forms cancel
// (theta cos - sin ~ theta^3 / 3 out of terms of size theta), so the Taylor
// series take over there (next terms theta^4 / 120 and smaller); above it
// 1 - cos is formed as 2 sin^2(theta / 2), which does not cancel.
struct RodCoef { float a, b, da, db; };

__device__ inline RodCoef rod_coef(float th) {
    RodCoef c;
    const float t2 = th * th;
    if (th < 1e-2f) {
        c.a = 1.0f - t2 / 6.0f;
        c.b = 0.5f - t2 / 24.0f;
        c.da = -th / 3.0f + th * t2 / 30.0f;
        c.db = -th / 12.0f + th * t2 / 180.0f;
    } else {
        const float s = sinf(th), co = cosf(th), sh = sinf(0.5f * th);
        const float omc = 2.0f * sh * sh;                  // 1 - cos(theta)
        c.a = s / th;
        c.b = omc / t2;
        c.da = (th * co - s) / t2;
        c.db = (th * s - 2.0f * omc) / (t2 * th);
    }
    return c;
}

// K = skew(v), row-major 3x3
__device__ inline void skew3(const float* v, float* K) {
    K[0] = 0.f;   K[1] = -v[2]; K[2] = v[1];
    K[3] = v[2];  K[4] = 0.f;   K[5] = -v[0];
    K[6] = -v[1]; K[7] = v[0];  K[8] = 0.f;
}

__device__ inline void mm3(const float* X, const float* Y, float* Z) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Z[3 * i + j] = X[3 * i] * Y[j] + X[3 * i + 1] * Y[3 + j] + X[3 * i + 2] * Y[6 + j];
}

__device__ inline float dot9(const float* X, const float* Y) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) s += X[i] * Y[i];
    return s;
}

// rn_rays_plain with the refinement of image `im` applied first: R = A(dR[im])
// R0, T = T0 + dT[im] (the rotation is not applied to the translation, as in
// the reference).  R is then applied with rn_rays_plain's dot products, so
// zero dR / dT (A = I exactly) reproduce its outputs.  dR, dT may be NULL.
__device__ __forceinline__ void rn_rays_pose(int64_t r, int64_t im, const float* __restrict__ P,
                                             const float* __restrict__ d,
                                             const float* __restrict__ dR,
                                             const float* __restrict__ dT,
                                             const float* __restrict__ mean_dir,
                                             float* __restrict__ rays_o,
                                             float* __restrict__ rays_d,
                                             float* __restrict__ imgs_d) {
    float R[9];
    if (dR) {
        const float v[3] = {dR[3 * im], dR[3 * im + 1], dR[3 * im + 2]};
        const float th = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + 1e-7f;
        const RodCoef c = rod_coef(th);
        float K[9], K2[9], A[9], R0[9];
        skew3(v, K);
        mm3(K, K, K2);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            A[i] = ((i % 4 == 0) ? 1.0f : 0.0f) + (c.a * K[i] + c.b * K2[i]);
            R0[i] = P[4 * (i / 3) + i % 3];
        }
        mm3(A, R0, R);
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = P[4 * (i / 3) + i % 3];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rays_d[3 * r + i] = d[0] * R[3 * i] + d[1] * R[3 * i + 1] + d[2] * R[3 * i + 2];
        const float T0 = P[4 * i + 3];
        rays_o[3 * r + i] = dT ? T0 + dT[3 * im + i] : T0;
        if (imgs_d)
            imgs_d[3 * r + i] = mean_dir[0] * R[3 * i] + mean_dir[1] * R[3 * i + 1] +
                                mean_dir[2] * R[3 * i + 2];
    }
}
