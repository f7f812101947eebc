// Whole-image validation (train_ml.py:214-250): the test-time gated combine
// that fills an image buffer chunk by chunk, and the two image metrics of
// validation_step -- the squared-error sum behind PSNR and the Gaussian-window
// SSIM -- on the renderer's own (H*W, C) interleaved layout.
//
// Both metrics are deterministic: every block writes one partial (its values
// summed in a fixed order, no atomics), and k_sum_partials adds the partials in
// a fixed order in double.  Two calls on the same inputs give the same bits.
#include "rn_common.h"

#include <cmath>

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / RN_WAVE;
constexpr int MT_MAX_BLOCKS = RN_METRICS_WORK_BYTES / 8;    // one double partial per block

// ---- test-time combine (ml_rendering.py:65-68,149-153; train_ml.py:243) -----
// The op order is rendering.ml_render's: per sub-NeRF rgb_i + bg (1 - op_i),
// then acc + that * gate_i, i ascending (contraction is off in this library).
__global__ void __launch_bounds__(MT_THREADS)
k_ml_combine_test(int n, int K, const float* __restrict__ gate, const float* __restrict__ op_k,
                  const float* __restrict__ depth_k, const float* __restrict__ rgb_k,
                  const float* __restrict__ bg, int64_t ray0, float* __restrict__ rgb,
                  float* __restrict__ opacity, float* __restrict__ depth,
                  float* __restrict__ depth_k_out) {
    const int b = blockIdx.x * MT_THREADS + threadIdx.x;
    if (b >= n) return;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, op = 0.f, de = 0.f;
    const int64_t row = ray0 + b;
    for (int i = 0; i < K; ++i) {
        const float g = gate ? gate[(int64_t)b * K + i] : 1.0f;
        const int64_t s = (int64_t)i * n + b;
        const float o = op_k[s], d = depth_k[s];
        const float rest = 1.0f - o;
        r0 = r0 + (rgb_k[3 * s + 0] + bg0 * rest) * g;
        r1 = r1 + (rgb_k[3 * s + 1] + bg1 * rest) * g;
        r2 = r2 + (rgb_k[3 * s + 2] + bg2 * rest) * g;
        op = op + o * g;
        de = de + d * g;
        if (depth_k_out) depth_k_out[row * K + i] = d;
    }
    rgb[3 * row + 0] = r0;
    rgb[3 * row + 1] = r1;
    rgb[3 * row + 2] = r2;
    opacity[row] = op;
    depth[row] = de;
}

// ---- fixed-order sums ---------------------------------------------------------
// the block's value: lane 0 of every wave holds a double, summed wave 0..3
__device__ __forceinline__ void block_partial(double wave_acc, double* __restrict__ work) {
    __shared__ double wsum[MT_WAVES];
    if (rn_lane() == 0) wsum[threadIdx.x / RN_WAVE] = wave_acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
        for (int w = 1; w < MT_WAVES; ++w) s += wsum[w];
        work[blockIdx.x] = s;
    }
}

// out = sum of work[0, n_part): thread t adds its strided share in ascending
// order, then a fixed tree over the 256 threads
__global__ void __launch_bounds__(MT_THREADS)
k_sum_partials(const double* __restrict__ work, int n_part, double* __restrict__ out) {
    __shared__ double red[MT_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_part; i += MT_THREADS) s += work[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = MT_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---- squared error (PeakSignalNoiseRatio's sum_squared_error) -----------------
__global__ void __launch_bounds__(MT_THREADS)
k_image_sse(int64_t n, const float* __restrict__ pred, const float* __restrict__ target,
            double* __restrict__ work) {
    // fp32 over a thread's few elements and across the wave, double from there
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * MT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += stride) {
        const float d = pred[i] - target[i];
        acc += d * d;
    }
    block_partial((double)rn_wave_sum(acc), work);
}

// ---- SSIM (StructuralSimilarityIndexMeasure, Gaussian 11 x 11, sigma 1.5) -----
constexpr int SS_WIN = 11;
constexpr int SS_TILE = 32;                       // valid outputs per tile side
constexpr int SS_HALO = SS_TILE + SS_WIN - 1;     // 42 staged pixels per side
constexpr int SS_PER_THREAD = SS_TILE * SS_TILE / MT_THREADS;
struct SsimWin { float w[SS_WIN]; };

// One block takes tiles t = blockIdx.x, + gridDim.x, ... (a fixed assignment);
// per tile and channel it stages the 42 x 42 halo of both images in LDS, runs
// the horizontal pass of the five moments (p, t, pp, tt, pt) into LDS, then
// the vertical pass with 4 outputs per thread.  The p and t moments go through
// the same operations in the same order, so pred == target gives mu_p == mu_t
// and s_pp == s_tt == s_pt bit for bit and the pixel value is exactly 1.
__global__ void __launch_bounds__(MT_THREADS)
k_ssim(int H, int W, int C, const float* __restrict__ pred, const float* __restrict__ target,
       SsimWin win, int tiles_x, int n_tiles, double* __restrict__ work,
       float* __restrict__ ssim_map) {
    __shared__ float sp[SS_HALO][SS_HALO + 1];
    __shared__ float st[SS_HALO][SS_HALO + 1];
    __shared__ float hm[5][SS_HALO][SS_TILE];
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    const int oh = H - (SS_WIN - 1), ow = W - (SS_WIN - 1);
    double wave_acc = 0.0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int y0 = (tile / tiles_x) * SS_TILE, x0 = (tile % tiles_x) * SS_TILE;
        for (int c = 0; c < C; ++c) {
            for (int i = threadIdx.x; i < SS_HALO * SS_HALO; i += MT_THREADS) {
                const int ly = i / SS_HALO, lx = i % SS_HALO;
                const int y = y0 + ly, x = x0 + lx;
                float p = 0.f, t = 0.f;
                if (y < H && x < W) {
                    const int64_t a = ((int64_t)y * W + x) * C + c;
                    p = pred[a];
                    t = target[a];
                }
                sp[ly][lx] = p;
                st[ly][lx] = t;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < SS_HALO * SS_TILE; i += MT_THREADS) {
                const int ly = i / SS_TILE, lx = i % SS_TILE;
                float mp = 0.f, mt = 0.f, pp = 0.f, tt = 0.f, pt = 0.f;
#pragma unroll
                for (int k = 0; k < SS_WIN; ++k) {
                    const float w = win.w[k], p = sp[ly][lx + k], t = st[ly][lx + k];
                    mp += w * p;
                    mt += w * t;
                    pp += w * (p * p);
                    tt += w * (t * t);
                    pt += w * (p * t);
                }
                hm[0][ly][lx] = mp;
                hm[1][ly][lx] = mt;
                hm[2][ly][lx] = pp;
                hm[3][ly][lx] = tt;
                hm[4][ly][lx] = pt;
            }
            __syncthreads();
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < SS_PER_THREAD; ++j) {
                const int i = j * MT_THREADS + threadIdx.x;
                const int ly = i / SS_TILE, lx = i % SS_TILE;
                float mp = 0.f, mt = 0.f, pp = 0.f, tt = 0.f, pt = 0.f;
#pragma unroll
                for (int k = 0; k < SS_WIN; ++k) {
                    const float w = win.w[k];
                    mp += w * hm[0][ly + k][lx];
                    mt += w * hm[1][ly + k][lx];
                    pp += w * hm[2][ly + k][lx];
                    tt += w * hm[3][ly + k][lx];
                    pt += w * hm[4][ly + k][lx];
                }
                const float mpp = mp * mp, mtt = mt * mt, mpt = mp * mt;
                const float vp = pp - mpp, vt = tt - mtt, vpt = pt - mpt;
                const float v = ((2.0f * mpt + c1) * (2.0f * vpt + c2)) /
                                ((mpp + mtt + c1) * (vp + vt + c2));
                const int y = y0 + ly, x = x0 + lx;
                if (y < oh && x < ow) {
                    acc += v;
                    if (ssim_map) ssim_map[((int64_t)y * ow + x) * C + c] = v;
                }
            }
            // each wave reduces its values; lane 0 keeps the wave's running double
            wave_acc += (double)rn_wave_sum(acc);
            // (the next channel's staging writes sp / st only, which the
            // vertical pass does not read; hm is rewritten after the next barrier)
        }
    }
    block_partial(wave_acc, work);
}

SsimWin gaussian_window() {
    // exp(-(d / sigma)^2 / 2) normalised to sum 1, formed in double
    double g[SS_WIN], s = 0.0;
    for (int k = 0; k < SS_WIN; ++k) {
        const double d = k - (SS_WIN - 1) / 2;
        g[k] = std::exp(-(d / 1.5) * (d / 1.5) / 2.0);
        s += g[k];
    }
    SsimWin w;
    for (int k = 0; k < SS_WIN; ++k) w.w[k] = (float)(g[k] / s);
    return w;
}

}  // namespace

extern "C" {

int rn_ml_combine_test(const float* gate, const float* opacity_k, const float* depth_k,
                       const float* rgb_k, const float* bg, int64_t n_rays, int32_t n_models,
                       int64_t ray0, float* rgb, float* opacity, float* depth,
                       float* depth_k_out /*may be NULL*/, void* stream) {
    RN_CHECK_ARG(n_rays >= 0 && n_rays <= 0x7fffffff && n_models >= 1 && ray0 >= 0, "bad sizes");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(opacity_k && depth_k && rgb_k && bg && rgb && opacity && depth, "null pointer");
    RN_CHECK_ARG(gate || n_models == 1, "gate may be NULL (exactly 1) for one model only");
    k_ml_combine_test<<<nblk(n_rays, MT_THREADS), MT_THREADS, 0, (hipStream_t)stream>>>(
        (int)n_rays, n_models, gate, opacity_k, depth_k, rgb_k, bg, ray0, rgb, opacity, depth,
        depth_k_out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_image_sse(const float* pred, const float* target, int64_t n_elems, void* work,
                 double* out_sse, void* stream) {
    RN_CHECK_ARG(n_elems >= 0, "bad sizes");
    RN_CHECK_ARG(out_sse && (n_elems == 0 || (pred && target && work)), "null pointer");
    // 8 elements per thread and pass before the grid is capped
    int blocks = 0;
    if (n_elems > 0) {
        const int64_t nb = (n_elems + 8 * MT_THREADS - 1) / (8 * MT_THREADS);
        blocks = (int)(nb < MT_MAX_BLOCKS ? nb : MT_MAX_BLOCKS);
        k_image_sse<<<blocks, MT_THREADS, 0, (hipStream_t)stream>>>(n_elems, pred, target,
                                                                    (double*)work);
    }
    // no partials: the sum of nothing, written by the same kernel (sse 0)
    k_sum_partials<<<1, MT_THREADS, 0, (hipStream_t)stream>>>((const double*)work, blocks,
                                                              out_sse);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_ssim(const float* pred, const float* target, int32_t H, int32_t W, int32_t C, void* work,
            double* out_sum, float* ssim_map /*may be NULL*/, void* stream) {
    RN_CHECK_ARG(H >= SS_WIN && W >= SS_WIN,
                 "H and W must be at least 11 (one 11 x 11 window)");
    RN_CHECK_ARG(C >= 1 && C <= 4, "C must be 1..4");
    RN_CHECK_ARG(pred && target && work && out_sum, "null pointer");
    static const SsimWin win = gaussian_window();
    const int tiles_x = nblk(W - (SS_WIN - 1), SS_TILE), tiles_y = nblk(H - (SS_WIN - 1), SS_TILE);
    const int64_t n_tiles = (int64_t)tiles_x * tiles_y;
    RN_CHECK_ARG(n_tiles <= 0x7fffffff, "image too large");
    const int blocks = (int)(n_tiles < MT_MAX_BLOCKS ? n_tiles : MT_MAX_BLOCKS);
    k_ssim<<<blocks, MT_THREADS, 0, (hipStream_t)stream>>>(H, W, C, pred, target, win, tiles_x,
                                                           (int)n_tiles, (double*)work, ssim_map);
    k_sum_partials<<<1, MT_THREADS, 0, (hipStream_t)stream>>>((const double*)work, blocks,
                                                              out_sum);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
