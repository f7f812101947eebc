// Error-guided pixel sampling (include/radnerf.h states the rule, bit by bit):
// a tiled error map over the training set, its integer weights and CDF
// (rn_guided_weights), the batch drawn from the mixture of the uniform and the
// map's density with each ray's importance weight (rn_sample_batch_guided),
// the loss epilogue that records the per-ray error and weights the backward
// seeds (rn_guided_epilogue), and the map's update (rn_guided_refresh).
// rn_sample_batch (sample.hip) is not touched: the uniform path keeps its
// device code.  The part of the batch that follows the picks (target, rays,
// jitter, background) is restated here statement for statement, so the same
// picks give the same bits from either entry.
#include "rn_common.h"
#include "rn_rays.h"
#pragma clang fp contract(off)

namespace {

constexpr uint64_t SB_NOISE = 0xd1b54a32d192ed03ull;
constexpr uint64_t SB_BG = 0x8cb92ba72f3d8dd7ull;
constexpr uint64_t SB_BRANCH = 0xa0761d6478bd642full;
constexpr uint64_t SB_CELL = 0xe7037ed1a0b428dbull;

constexpr int GD_T = 256;                   // threads of a scan block
constexpr int GD_PER = 4;                   // cells per thread
constexpr int GD_CELLS = GD_T * GD_PER;     // cells per scan block
constexpr int GD_TOP = 1024;                // threads of the block that scans the block sums
constexpr int64_t GD_MAX_CELLS = (int64_t)1 << 24;
constexpr int GD_LDS_IMAGES = 20480;        // image totals staged in LDS: up to its 160 KiB
static_assert(GD_MAX_CELLS / GD_CELLS * 8 <= RN_GUIDED_WORK_BYTES, "block sums fit the scratch");

struct Geom {
    uint32_t W, H, tile, tw, th, cpi;       // cpi: cells per image
};

__device__ __forceinline__ uint32_t gd_cw(const Geom& g, uint32_t tx) {
    return min(g.tile, g.W - tx * g.tile);
}
__device__ __forceinline__ uint32_t gd_ch(const Geom& g, uint32_t ty) {
    return min(g.tile, g.H - ty * g.tile);
}
__device__ __forceinline__ uint32_t gd_npx(const Geom& g, uint32_t c) {
    const uint32_t rem = c % g.cpi;
    return gd_cw(g, rem % g.tw) * gd_ch(g, rem / g.tw);
}

__device__ __forceinline__ uint32_t gd_weight(float e) {
    const float v = rintf(e * 65536.0f);
    if (!(v >= 1.0f)) return 1u;            // also a NaN
    return v >= 16777216.0f ? (1u << 24) : (uint32_t)v;
}

// inclusive prefix sum over the block's threads (T a multiple of 64, at most
// 1024); *total gets the block's sum.  sW: T / 64 words of LDS.
template <int T>
__device__ __forceinline__ uint64_t gd_block_scan(uint64_t v, uint64_t* sW, uint64_t* total) {
    const int lane = rn_lane(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < RN_WAVE; off <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)v, off);
        if (lane >= off) v += t;
    }
    if (lane == RN_WAVE - 1) sW[wave] = v;
    __syncthreads();
    uint64_t carry = 0, all = 0;
#pragma unroll
    for (int i = 0; i < T / RN_WAVE; ++i) {
        const uint64_t s = sW[i];
        if (i < wave) carry += s;
        all += s;
    }
    *total = all;
    return v + carry;
}

// pass 1: w, and each block's mass
__global__ void __launch_bounds__(GD_T)
k_gw_sums(const float* __restrict__ emap, Geom g, uint32_t n_cells, uint32_t* __restrict__ w,
          uint64_t* __restrict__ block_sum) {
    __shared__ uint64_t sW[GD_T / RN_WAVE];
    const uint32_t c0 = blockIdx.x * GD_CELLS + threadIdx.x * GD_PER;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < GD_PER; ++i) {
        const uint32_t c = c0 + i;
        if (c < n_cells) {
            const uint32_t wc = gd_weight(emap[c]);
            w[c] = wc;
            m += (uint64_t)wc * gd_npx(g, c);
        }
    }
    uint64_t total;
    gd_block_scan<GD_T>(m, sW, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// pass 2, one block: the block sums become their exclusive prefix sums
__global__ void __launch_bounds__(GD_TOP)
k_gw_scan_blocks(uint64_t* __restrict__ block_sum, uint32_t n_blocks) {
    __shared__ uint64_t sW[GD_TOP / RN_WAVE];
    const uint32_t per = (n_blocks + GD_TOP - 1) / GD_TOP;
    const uint32_t b0 = threadIdx.x * per;
    uint64_t m = 0;
    for (uint32_t i = 0; i < per; ++i)
        if (b0 + i < n_blocks) m += block_sum[b0 + i];
    uint64_t total;
    uint64_t run = gd_block_scan<GD_TOP>(m, sW, &total) - m;
    for (uint32_t i = 0; i < per; ++i) {
        if (b0 + i < n_blocks) {
            const uint64_t v = block_sum[b0 + i];
            block_sum[b0 + i] = run;
            run += v;
        }
    }
}

// pass 3: the cells' inclusive sums
__global__ void __launch_bounds__(GD_T)
k_gw_cdf(const uint32_t* __restrict__ w, Geom g, uint32_t n_cells,
         const uint64_t* __restrict__ block_off, uint64_t* __restrict__ cdf) {
    __shared__ uint64_t sW[GD_T / RN_WAVE];
    const uint32_t c0 = blockIdx.x * GD_CELLS + threadIdx.x * GD_PER;
    uint64_t m[GD_PER], sum = 0;
#pragma unroll
    for (int i = 0; i < GD_PER; ++i) {
        const uint32_t c = c0 + i;
        m[i] = c < n_cells ? (uint64_t)w[c] * gd_npx(g, c) : 0;
        sum += m[i];
    }
    uint64_t total;
    uint64_t run = gd_block_scan<GD_T>(sum, sW, &total) - sum + block_off[blockIdx.x];
#pragma unroll
    for (int i = 0; i < GD_PER; ++i) {
        run += m[i];
        if (c0 + i < n_cells) cdf[c0 + i] = run;
    }
}

struct GuidedBatch {
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
    Geom g;
    float frac;
    int lds;                        // the image totals are staged in LDS
    const uint32_t* w;
    const uint64_t* cdf;
    int32_t* cell;
    float* weight;
};

// the smallest index in [lo, hi] whose entry exceeds t (the last one does)
template <typename F>
__device__ __forceinline__ uint32_t gd_upper(uint32_t lo, uint32_t hi, uint64_t t, F at) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (at(mid) > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One thread per ray, as k_sample_batch; the guided branch searches the image
// totals, then the image's cells.
template <bool FP32, bool POSE>
__global__ void __launch_bounds__(256)
k_sample_guided(GuidedBatch s) {
    extern __shared__ uint64_t sTot[];      // cdf at each image's last cell
    const Geom g = s.g;
    if (s.lds) {
        for (uint32_t i = threadIdx.x; i < (uint32_t)s.n_images; i += blockDim.x)
            sTot[i] = s.cdf[(uint64_t)(i + 1) * g.cpi - 1];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s.bg && blockIdx.x == 0 && threadIdx.x < 3)
        s.bg[threadIdx.x] = rn_unit64(rn_mix64((s.key ^ SB_BG) +
                                               (uint64_t)(threadIdx.x + 1) * RN_GOLDEN64));
    if (r >= s.n) return;
    const uint64_t ctr = (uint64_t)(r + 1) * RN_GOLDEN64;
    const uint64_t z = rn_mix64(s.key + ctr);
    const float u = rn_unit64(rn_mix64((s.key ^ SB_BRANCH) + ctr));
    const uint64_t n_cells = s.n_images * g.cpi;
    const uint64_t total = s.cdf[n_cells - 1];
    uint64_t im, px;
    uint32_t c;
    if (u < s.frac) {
        im = ((z >> 32) * s.n_images) >> 32;                            // < n_images
        px = ((z & 0xffffffffull) * s.n_pix) >> 32;                     // < n_pix
        const uint32_t y = (uint32_t)px / g.W, x = (uint32_t)px % g.W;
        c = ((uint32_t)im * g.th + y / g.tile) * g.tw + x / g.tile;
    } else {
        const uint64_t z2 = rn_mix64((s.key ^ SB_CELL) + ctr);
        const uint64_t t = __umul64hi(z2, total);                       // < total
        const uint64_t* cdf = s.cdf;
        const uint32_t last = (uint32_t)s.n_images - 1;
        const uint32_t img = s.lds
            ? gd_upper(0, last, t, [&](uint32_t i) { return sTot[i]; })
            : gd_upper(0, last, t, [&](uint32_t i) { return cdf[(uint64_t)(i + 1) * g.cpi - 1]; });
        c = gd_upper(img * g.cpi, (img + 1) * g.cpi - 1, t, [&](uint32_t i) { return cdf[i]; });
        const uint64_t below = c ? cdf[c - 1] : 0;
        const uint32_t rem = c - img * g.cpi;
        const uint32_t ty = rem / g.tw, tx = rem % g.tw, cw = gd_cw(g, tx);
        // < n_px(c) when w and cdf belong together (rn_guided_weights); the
        // clamp keeps a caller's mismatched pair inside the image
        const uint32_t j = (uint32_t)min((t - below) / max(s.w[c], 1u),
                                         (uint64_t)(cw * gd_ch(g, ty) - 1));
        im = img;
        px = (uint64_t)(ty * g.tile + j / cw) * g.W + (tx * g.tile + j % cw);
    }
    s.cell[r] = (int32_t)c;
    {
        const double f = (double)s.frac;
        const double n_all = (double)(s.n_images * s.n_pix);
        s.weight[r] = (float)(1.0 / (f + (((1.0 - f) * (double)s.w[c]) * n_all) / (double)total));
    }
    s.img_idx[r] = (int64_t)im;
    s.pix_idx[r] = (int64_t)px;
    // from here on k_sample_batch (sample.hip), statement for statement
    const uint64_t e = (im * s.n_pix + px) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (FP32) {
            s.target[3 * r + ch] = ((const float*)s.images)[e + ch];
        } else {
            s.target[3 * r + ch] = (float)((const uint8_t*)s.images)[e + ch] / 255.0f;
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

// One thread per ray.  The lanes of a wave that share a cell are summed and
// their first lane issues the two atomics: a batch that sits in one cell
// sends one pair per wave instead of 64 to one address.
__global__ void __launch_bounds__(256)
k_guided_epilogue(const float* __restrict__ rgb, const float* __restrict__ target,
                  const int32_t* __restrict__ cell_idx, const float* __restrict__ ray_weight,
                  int64_t n, int K, int64_t n_cells, uint64_t* __restrict__ acc_sum,
                  uint32_t* __restrict__ acc_cnt, float* __restrict__ d_rgb,
                  float* __restrict__ d_op, float* __restrict__ d_depth) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = r < n;
    if (acc_sum) {                          // uniform: no lane leaves before the loop
        int32_t cell = -1;
        uint32_t q = 0;
        if (in) {
            const float d0 = rgb[3 * r] - target[3 * r], d1 = rgb[3 * r + 1] - target[3 * r + 1],
                        d2 = rgb[3 * r + 2] - target[3 * r + 2];
            const float e = (d0 * d0 + d1 * d1) + d2 * d2;
            const int32_t c = cell_idx[r];
            if (isfinite(e) && c >= 0 && (int64_t)c < n_cells) {
                cell = c;
                q = (uint32_t)fminf(rintf(e * 1048576.0f), 16777216.0f);
            }
        }
        const int lane = rn_lane();
        unsigned long long pending = __ballot(cell >= 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int32_t lc = __shfl(cell, leader);
            const bool mine = cell == lc;
            const unsigned long long grp = __ballot(mine);
            uint32_t v = mine ? q : 0u;     // at most 64 * 2^24
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
            if (lane == leader) {
                atomicAdd((unsigned long long*)acc_sum + lc, (unsigned long long)v);
                atomicAdd(acc_cnt + lc, (uint32_t)__popcll(grp));
            }
            pending &= ~grp;
        }
    }
    if (!in) return;
    const float wgt = ray_weight[r];
#pragma unroll
    for (int i = 0; i < 3; ++i) d_rgb[3 * r + i] = d_rgb[3 * r + i] * wgt;
    d_op[r] = d_op[r] * wgt;
    if (d_depth)
        for (int k = 0; k < K; ++k) d_depth[r * K + k] = d_depth[r * K + k] * wgt;
}

__global__ void __launch_bounds__(256)
k_guided_refresh(float* __restrict__ emap, uint64_t* __restrict__ acc_sum,
                 uint32_t* __restrict__ acc_cnt, int64_t n_cells, float alpha) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t cnt = acc_cnt[c];
    if (cnt == 0) return;                   // (acc_sum is 0 with it)
    const float mean = (float)(((double)acc_sum[c] * (1.0 / 1048576.0)) / (double)cnt);
    const float e = emap[c];
    emap[c] = e + alpha * (mean - e);
    acc_sum[c] = 0;
    acc_cnt[c] = 0;
}

// the geometry's checks, shared by the two entries that take it
int gd_geom(const char* who, int64_t n_images, int32_t W, int32_t H, int32_t tile, Geom* g,
            int64_t* n_cells) {
    RN_CHECK_ARG_AS(who, tile >= 1 && tile <= 256, "tile must be in 1..256");
    RN_CHECK_ARG_AS(who, W >= 1 && H >= 1 && n_images >= 1, "W, H and n_images must be >= 1");
    const int64_t tw = ((int64_t)W + tile - 1) / tile, th = ((int64_t)H + tile - 1) / tile;
    RN_CHECK_ARG_AS(who, n_images < GD_MAX_CELLS && tw * th < GD_MAX_CELLS &&
                    n_images * tw * th < GD_MAX_CELLS, "n_cells must be below 2^24");
    g->W = (uint32_t)W; g->H = (uint32_t)H; g->tile = (uint32_t)tile;
    g->tw = (uint32_t)tw; g->th = (uint32_t)th; g->cpi = (uint32_t)(tw * th);
    *n_cells = n_images * tw * th;
    return 0;
}

}  // namespace

extern "C" int rn_guided_weights(const float* emap, int64_t n_images, int32_t W, int32_t H,
                                 int32_t tile, uint32_t* w, uint64_t* cdf, void* work,
                                 void* stream) {
    Geom g;
    int64_t n_cells;
    if (int st = gd_geom(__func__, n_images, W, H, tile, &g, &n_cells)) return st;
    RN_CHECK_ARG(emap && w && cdf && work, "null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = nblk(n_cells, GD_CELLS);         // at most 2^14
    uint64_t* sums = (uint64_t*)work;
    k_gw_sums<<<blocks, GD_T, 0, st>>>(emap, g, (uint32_t)n_cells, w, sums);
    RN_CHECK_LAUNCH();
    k_gw_scan_blocks<<<1, GD_TOP, 0, st>>>(sums, (uint32_t)blocks);
    RN_CHECK_LAUNCH();
    k_gw_cdf<<<blocks, GD_T, 0, st>>>(w, g, (uint32_t)n_cells, sums, cdf);
    RN_CHECK_LAUNCH();
    return 0;
}

extern "C" int rn_sample_batch_guided(const void* images, int32_t image_dtype, int64_t n_images,
                                      int64_t n_pix, const float* directions, const float* poses,
                                      const float* dR, const float* dT, const float* mean_dir,
                                      uint64_t seed, int64_t step, int32_t rank, int64_t n_rays,
                                      int32_t n_models, int64_t* img_idxs, int64_t* pix_idxs,
                                      float* target_rgb, float* rays_o, float* rays_d,
                                      float* imgs_d, float* noise, float* bg, int32_t W,
                                      int32_t H, int32_t tile, float uniform_frac,
                                      const uint32_t* w, const uint64_t* cdf, int32_t* cell_idx,
                                      float* ray_weight, void* stream) {
    RN_CHECK_ARG(step >= 0 && step < ((int64_t)1 << 40), "step must be in [0, 2^40)");
    RN_CHECK_ARG(rank >= 0 && rank < (1 << 24), "rank must be in [0, 2^24)");
    RN_CHECK_ARG(n_images >= 1 && n_images < ((int64_t)1 << 32) && n_pix >= 1 &&
                 n_pix < ((int64_t)1 << 32), "n_images and n_pix must be in [1, 2^32)");
    RN_CHECK_ARG(image_dtype == 0 || image_dtype == 1, "image_dtype must be 0 (uint8) or 1 (fp32)");
    RN_CHECK_ARG(n_rays >= 0 && n_rays < ((int64_t)1 << 38) && n_models >= 1, "bad sizes");
    RN_CHECK_ARG((imgs_d == nullptr) == (mean_dir == nullptr),
                 "imgs_d and mean_dir must be given together");
    RN_CHECK_ARG(uniform_frac >= 0.0f && uniform_frac <= 1.0f, "uniform_frac must be in [0, 1]");
    GuidedBatch s;
    int64_t n_cells;
    if (int st = gd_geom(__func__, n_images, W, H, tile, &s.g, &n_cells)) return st;
    RN_CHECK_ARG((int64_t)W * H == n_pix, "W * H must equal n_pix");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(images && directions && poses && img_idxs && pix_idxs && target_rgb && rays_o &&
                 rays_d && w && cdf && cell_idx && ray_weight, "null pointer");
    s.images = images; s.dirs = directions; s.poses = poses; s.dR = dR; s.dT = dT;
    s.mean_dir = mean_dir;
    s.key = rn_mix64(seed * RN_GOLDEN64 + (((uint64_t)rank << 40) | (uint64_t)step));
    s.n_images = (uint64_t)n_images; s.n_pix = (uint64_t)n_pix;
    s.n = n_rays; s.K = n_models;
    s.img_idx = img_idxs; s.pix_idx = pix_idxs; s.target = target_rgb;
    s.rays_o = rays_o; s.rays_d = rays_d; s.imgs_d = imgs_d; s.noise = noise; s.bg = bg;
    s.frac = uniform_frac;
    // all-uniform batches never search: nothing to stage
    s.lds = n_images <= GD_LDS_IMAGES && uniform_frac < 1.0f;
    s.w = w; s.cdf = cdf; s.cell = cell_idx; s.weight = ray_weight;
    const int blocks = (int)((n_rays + 255) / 256);
    const size_t lds = s.lds ? (size_t)n_images * sizeof(uint64_t) : 0;
    const hipStream_t st = (hipStream_t)stream;
    const bool pose = dR || dT;
    if (image_dtype == 1) {
        if (pose) k_sample_guided<true, true><<<blocks, 256, lds, st>>>(s);
        else k_sample_guided<true, false><<<blocks, 256, lds, st>>>(s);
    } else {
        if (pose) k_sample_guided<false, true><<<blocks, 256, lds, st>>>(s);
        else k_sample_guided<false, false><<<blocks, 256, lds, st>>>(s);
    }
    RN_CHECK_LAUNCH();
    return 0;
}

extern "C" int rn_guided_epilogue(const float* rgb, const float* target_rgb,
                                  const int32_t* cell_idx, const float* ray_weight,
                                  int64_t n_rays, int32_t n_models, int64_t n_cells,
                                  uint64_t* acc_sum, uint32_t* acc_cnt, float* dL_drgb,
                                  float* dL_dopacity, float* dL_ddepth, void* stream) {
    RN_CHECK_ARG(n_rays >= 0 && n_rays < ((int64_t)1 << 38) && n_models >= 1, "bad sizes");
    RN_CHECK_ARG((acc_sum == nullptr) == (acc_cnt == nullptr),
                 "acc_sum and acc_cnt must be given together");
    RN_CHECK_ARG(!acc_sum || (n_cells >= 1 && n_cells < GD_MAX_CELLS),
                 "n_cells must be in [1, 2^24)");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(ray_weight && dL_drgb && dL_dopacity, "null pointer");
    RN_CHECK_ARG(!acc_sum || (rgb && target_rgb && cell_idx), "null pointer");
    k_guided_epilogue<<<nblk(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
        rgb, target_rgb, cell_idx, ray_weight, n_rays, n_models, n_cells, acc_sum, acc_cnt,
        dL_drgb, dL_dopacity, dL_ddepth);
    RN_CHECK_LAUNCH();
    return 0;
}

extern "C" int rn_guided_refresh(float* emap, uint64_t* acc_sum, uint32_t* acc_cnt,
                                 int64_t n_cells, float alpha, void* stream) {
    RN_CHECK_ARG(n_cells >= 1 && n_cells < GD_MAX_CELLS, "n_cells must be in [1, 2^24)");
    RN_CHECK_ARG(alpha > 0.0f && alpha <= 1.0f, "alpha must be in (0, 1]");
    RN_CHECK_ARG(emap && acc_sum && acc_cnt, "null pointer");
    k_guided_refresh<<<nblk(n_cells, 256), 256, 0, (hipStream_t)stream>>>(emap, acc_sum, acc_cnt,
                                                                         n_cells, alpha);
    RN_CHECK_LAUNCH();
    return 0;
}
