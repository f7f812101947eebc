// The inputs of one training step from a device-resident training set
// (datasets/base.py:23-31: the per-batch image and pixel picks and the target
// gather; train_ml.py:84-96: the rays of those picks; train_ml.py:180 /
// ml_rendering.py:192-198: the march jitter and the random background) in one
// launch.  Everything random is a counter-based hash of (seed, rank, step):
// no generator state, so a step's batch depends on nothing but its key, the
// ranks of a data-parallel run draw different pixels, and a resumed run
// continues the stream.  include/radnerf.h states the stream.
#include "rn_common.h"
#include "rn_rays.h"
#pragma clang fp contract(off)

namespace {

constexpr uint64_t SB_NOISE = 0xd1b54a32d192ed03ull;
constexpr uint64_t SB_BG = 0x8cb92ba72f3d8dd7ull;

struct SampleBatch {
    const void* images;             // (n_images, n_pix, 3) uint8 or fp32
    const float* dirs;              // (n_pix, 3)
    const float* poses;             // (n_images, 3, 4)
    const float* dR;                // (n_images, 3) or NULL
    const float* dT;
    const float* mean_dir;          // NULL together with imgs_d
    uint64_t key;
    uint64_t n_images, n_pix;
    int64_t n;
    int K;
    int64_t* img_idx;
    int64_t* pix_idx;
    float* target;
    float* rays_o;
    float* rays_d;
    float* imgs_d;
    float* noise;                   // (K, n) or NULL
    float* bg;                      // 3 or NULL
};

// One thread per ray: its pick, the target, the rays, and its column of the
// jitter; the first three threads of block 0 also write the background.
// FP32: the images' element type; POSE: dR or dT given.
template <bool FP32, bool POSE>
__global__ void __launch_bounds__(256)
k_sample_batch(SampleBatch s) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s.bg && blockIdx.x == 0 && threadIdx.x < 3)
        s.bg[threadIdx.x] = rn_unit64(rn_mix64((s.key ^ SB_BG) +
                                               (uint64_t)(threadIdx.x + 1) * RN_GOLDEN64));
    if (r >= s.n) return;
    const uint64_t z = rn_mix64(s.key + (uint64_t)(r + 1) * RN_GOLDEN64);
    const uint64_t im = ((z >> 32) * s.n_images) >> 32;                 // < n_images
    const uint64_t px = ((z & 0xffffffffull) * s.n_pix) >> 32;          // < n_pix
    s.img_idx[r] = (int64_t)im;
    s.pix_idx[r] = (int64_t)px;
    // 64-bit element offset: a few hundred 12-Mpixel images pass 2^32 bytes
    const uint64_t e = (im * s.n_pix + px) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (FP32) {
            s.target[3 * r + c] = ((const float*)s.images)[e + c];
        } else {
            // a division, as torch's u8.float() / 255 (a multiply by the
            // reciprocal differs on 126 of the 256 values)
            s.target[3 * r + c] = (float)((const uint8_t*)s.images)[e + c] / 255.0f;
        }
    }
    const float* P = s.poses + 12 * im;
    const float* d = s.dirs + 3 * px;
    if (POSE)
        rn_rays_pose(r, (int64_t)im, P, d, s.dR, s.dT, s.mean_dir, s.rays_o, s.rays_d, s.imgs_d);
    else
        rn_rays_plain(r, P, d, s.mean_dir, s.rays_o, s.rays_d, s.imgs_d);
    if (s.noise) {
        for (int k = 0; k < s.K; ++k) {
            const uint64_t j = (uint64_t)k * (uint64_t)s.n + (uint64_t)r;
            s.noise[j] = rn_unit64(rn_mix64((s.key ^ SB_NOISE) + (j + 1) * RN_GOLDEN64));
        }
    }
}

}  // namespace

extern "C" int rn_sample_batch(const void* images, int32_t image_dtype, int64_t n_images,
                               int64_t n_pix, const float* directions, const float* poses,
                               const float* dR, const float* dT, const float* mean_dir,
                               uint64_t seed, int64_t step, int32_t rank, int64_t n_rays,
                               int32_t n_models, int64_t* img_idxs, int64_t* pix_idxs,
                               float* target_rgb, float* rays_o, float* rays_d, float* imgs_d,
                               float* noise, float* bg, void* stream) {
    RN_CHECK_ARG(step >= 0 && step < ((int64_t)1 << 40), "step must be in [0, 2^40)");
    RN_CHECK_ARG(rank >= 0 && rank < (1 << 24), "rank must be in [0, 2^24)");
    RN_CHECK_ARG(n_images >= 1 && n_images < ((int64_t)1 << 32) && n_pix >= 1 &&
                 n_pix < ((int64_t)1 << 32), "n_images and n_pix must be in [1, 2^32)");
    RN_CHECK_ARG(image_dtype == 0 || image_dtype == 1, "image_dtype must be 0 (uint8) or 1 (fp32)");
    RN_CHECK_ARG(n_rays >= 0 && n_rays < ((int64_t)1 << 38) && n_models >= 1, "bad sizes");
    RN_CHECK_ARG((imgs_d == nullptr) == (mean_dir == nullptr),
                 "imgs_d and mean_dir must be given together");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(images && directions && poses && img_idxs && pix_idxs && target_rgb && rays_o &&
                 rays_d, "null pointer");
    SampleBatch s;
    s.images = images; s.dirs = directions; s.poses = poses; s.dR = dR; s.dT = dT;
    s.mean_dir = mean_dir;
    s.key = rn_mix64(seed * RN_GOLDEN64 + (((uint64_t)rank << 40) | (uint64_t)step));
    s.n_images = (uint64_t)n_images; s.n_pix = (uint64_t)n_pix;
    s.n = n_rays; s.K = n_models;
    s.img_idx = img_idxs; s.pix_idx = pix_idxs; s.target = target_rgb;
    s.rays_o = rays_o; s.rays_d = rays_d; s.imgs_d = imgs_d; s.noise = noise; s.bg = bg;
    const int blocks = (int)((n_rays + 255) / 256);
    const hipStream_t st = (hipStream_t)stream;
    const bool pose = dR || dT;
    if (image_dtype == 1) {
        if (pose) k_sample_batch<true, true><<<blocks, 256, 0, st>>>(s);
        else k_sample_batch<true, false><<<blocks, 256, 0, st>>>(s);
    } else {
        if (pose) k_sample_batch<false, true><<<blocks, 256, 0, st>>>(s);
        else k_sample_batch<false, false><<<blocks, 256, 0, st>>>(s);
    }
    RN_CHECK_LAUNCH();
    return 0;
}
