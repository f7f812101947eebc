// Depth supervision: the batch's target ray parameters from device-resident
// depth maps (rn_gather_depth), after the picks exist.  The ray-termination
// second moment is formed inside the composite kernels (composite.hip, DEPTH),
// the two depth terms and their seeds in train.hip (rn_depth_loss).
// include/radnerf.h states the operation order.
#include "rn_common.h"
#pragma clang fp contract(off)

namespace {

// One thread per ray: the pick's raw depth -> the ray parameter t at which the
// ray meets the measured surface; 0 = no measurement.
// FP32: the maps' element type; EUCLID: kind 1 (range along the ray).
template <bool FP32, bool EUCLID>
__global__ void __launch_bounds__(256)
k_gather_depth(const void* __restrict__ depths, uint64_t n_images, uint64_t n_pix, float scale,
               const float* __restrict__ dirs, const int64_t* __restrict__ img_idx,
               const int64_t* __restrict__ pix_idx, int64_t n, float* __restrict__ target_t) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t im = img_idx[r], px = pix_idx[r];
    float t = 0.f;
    // a pick outside the maps reads nothing
    if (im >= 0 && (uint64_t)im < n_images && px >= 0 && (uint64_t)px < n_pix) {
        const uint64_t e = (uint64_t)im * n_pix + (uint64_t)px;        // 64-bit element offset
        const float v = FP32 ? ((const float*)depths)[e] : (float)((const uint16_t*)depths)[e];
        if (v > 0.f) {                  // false for 0, a negative value and NaN
            t = v * scale;
            if (EUCLID) {
                const float dx = dirs[3 * px], dy = dirs[3 * px + 1], dz = dirs[3 * px + 2];
                t = t / sqrtf((dx * dx + dy * dy) + dz * dz);
            }
            if (!(t > 0.f)) t = 0.f;    // a scale <= 0, an underflow, a zero direction's NaN
        }
    }
    target_t[r] = t;
}

}  // namespace

extern "C" {

int rn_gather_depth(const void* depths, int32_t depth_dtype, int64_t n_images, int64_t n_pix,
                    float scale, int32_t kind, const float* directions, const int64_t* img_idxs,
                    const int64_t* pix_idxs, int64_t n_rays, float* target_t, void* stream) {
    RN_CHECK_ARG(n_images >= 1 && n_images < ((int64_t)1 << 32) && n_pix >= 1 &&
                 n_pix < ((int64_t)1 << 32), "n_images and n_pix must be in [1, 2^32)");
    RN_CHECK_ARG(depth_dtype == 0 || depth_dtype == 1, "depth_dtype must be 0 (uint16) or 1 (fp32)");
    RN_CHECK_ARG(kind == 0 || kind == 1, "kind must be 0 (ray parameter) or 1 (Euclidean range)");
    RN_CHECK_ARG(n_rays >= 0 && n_rays < ((int64_t)1 << 38), "bad sizes");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(depths && img_idxs && pix_idxs && target_t && (kind == 0 || directions),
                 "null pointer");
    const int blocks = (int)((n_rays + 255) / 256);
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t ni = (uint64_t)n_images, np = (uint64_t)n_pix;
    if (depth_dtype == 1) {
        if (kind) k_gather_depth<true, true><<<blocks, 256, 0, st>>>(
            depths, ni, np, scale, directions, img_idxs, pix_idxs, n_rays, target_t);
        else k_gather_depth<true, false><<<blocks, 256, 0, st>>>(
            depths, ni, np, scale, directions, img_idxs, pix_idxs, n_rays, target_t);
    } else {
        if (kind) k_gather_depth<false, true><<<blocks, 256, 0, st>>>(
            depths, ni, np, scale, directions, img_idxs, pix_idxs, n_rays, target_t);
        else k_gather_depth<false, false><<<blocks, 256, 0, st>>>(
            depths, ni, np, scale, directions, img_idxs, pix_idxs, n_rays, target_t);
    }
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
