// LPIPS (VGG) on the device: the input step, the 3 x 3 convolution stack of
// VGG16 on v_mfma_f32_32x32x16_f16, the 2 x 2 max-pool and the per-tap
// distance (include/radnerf.h "LPIPS"; DESIGN.md §4 "LPIPS").
//
// Activations are f16, (n_img, H, W, C) with the channels innermost; weights
// are f16 MFMA fragments packed once (radnerf_amd/lpips.py pack_conv), the
// bias is fp32, every accumulation is fp32.  No kernel here uses an atomic:
// each output element is written by one thread, and the distance sums
// per-block partials in a fixed order in double, so a result is a function of
// the inputs alone.
//
// The convolution as an implicit GEMM, per block:
//   C[cout][pixel] += A[cout][k] . B[k][pixel],  k = (tap, cin)
// A = a pre-packed weight fragment (rn_mlp.h lane map: lane l holds
// A[l & 31][8 (l >> 5) + j]), B = 8 consecutive input channels of the pixel
// l & 31 at the tap, one 16-byte LDS read from the staged halo tile.  A block
// is 4 waves on an 8 x 32 pixel tile and 64 output channels; a wave takes two
// image rows of 32 pixels and both 32-channel halves (4 accumulator tiles), so
// every A and every B fragment feeds two MFMAs.  The input channels go through
// LDS in chunks of 64: (8 + 2) x (32 + 2) pixels x 64 halfs, with the pixel
// stride padded to 72 halfs so the 16-byte reads of 16 consecutive pixels fall
// on 16 different bank groups.
#include "rn_mlp.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / RN_WAVE;
constexpr int LP_MAX_BLOCKS = RN_METRICS_WORK_BYTES / 8;    // one double partial per block

// ---- input step ---------------------------------------------------------------
// per element, fp32, every operation rounded on its own:
//   v = min(max(2 x - 1, -1), 1);  y = (v - shift[c]) / scale[c];  f16(y)
__global__ void __launch_bounds__(LP_THREADS)
k_lpips_prepare(int64_t n, const float* __restrict__ rgb, rn_half* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % 3);
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    float v = 2.0f * rgb[i] - 1.0f;
    v = fminf(fmaxf(v, -1.0f), 1.0f);
    out[i] = (rn_half)((v - shift) / scale);
}

// ---- 3 x 3 convolution + bias + ReLU --------------------------------------------
constexpr int CV_TH = 8, CV_TW = 32;            // output pixels per block
constexpr int CV_CO = 64;                       // output channels per block
constexpr int CV_CK = 64;                       // input channels per LDS chunk
constexpr int CV_HH = CV_TH + 2, CV_HW = CV_TW + 2;
constexpr int CV_PS = CV_CK + 8;                // pixel stride in halfs (144 B)
constexpr int CV_PS1 = 40;                      // first layer: 32 k + 8 (80 B)
constexpr int CV_LDS_HALFS = CV_HH * CV_HW * CV_PS;

typedef int lp_i4 __attribute__((ext_vector_type(4)));
typedef int lp_i2 __attribute__((ext_vector_type(2)));

// FIRST: Cin = 3.  The 27 products of a pixel are one reduction padded to 32
// (k = 3 tap + c; k >= 27 is zero in the weights and in the staged image), so
// the tile is staged as im2col rows [pixel][32] and the loop is two k-steps.
template <bool FIRST>
__global__ void __launch_bounds__(LP_THREADS)
k_conv3x3_relu(int H, int W, int Cin, int Cout, const rn_half* __restrict__ in,
               const rn_half* __restrict__ wfrag, const float* __restrict__ bias,
               rn_half* __restrict__ out, int tiles_x) {
    __shared__ __attribute__((aligned(16))) rn_half lds[FIRST ? CV_TH * CV_TW * CV_PS1
                                                              : CV_LDS_HALFS];
    const int y0 = (blockIdx.x / tiles_x) * CV_TH, x0 = (blockIdx.x % tiles_x) * CV_TW;
    const int cg = blockIdx.y;                   // 64 output channels
    const int64_t img = blockIdx.z;
    const rn_half* src = in + img * H * W * Cin;
    const int lane = rn_lane(), wave = threadIdx.x / RN_WAVE, r = lane & 31, h = lane >> 5;
    f32x16 acc[2][2];                            // [cout half][row of the wave]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[t][q] = rn_zero16();

    if (FIRST) {
        for (int i = threadIdx.x; i < CV_TH * CV_TW * 32; i += LP_THREADS) {
            const int p = i >> 5, k = i & 31;
            rn_half v = (rn_half)0.f;
            if (k < 27) {
                const int tap = k / 3, c = k % 3;
                const int y = y0 + p / CV_TW + tap / 3 - 1, x = x0 + p % CV_TW + tap % 3 - 1;
                if (y >= 0 && y < H && x >= 0 && x < W) v = src[((int64_t)y * W + x) * 3 + c];
            }
            lds[p * CV_PS1 + k] = v;
        }
        __syncthreads();
        const rn_half* wf = wfrag + (int64_t)(cg * 2) * 2 * RN_FRAG_HALFS;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const half8 a0 = rn_frag(wf, ks), a1 = rn_frag(wf, 2 + ks);
            const rn_half* bp = lds + ((wave * 2) * CV_TW + r) * CV_PS1 + ks * 16 + 8 * h;
            const half8 b0 = *reinterpret_cast<const half8*>(bp);
            const half8 b1 = *reinterpret_cast<const half8*>(bp + CV_TW * CV_PS1);
            acc[0][0] = rn_mfma(a0, b0, acc[0][0]);
            acc[0][1] = rn_mfma(a0, b1, acc[0][1]);
            acc[1][0] = rn_mfma(a1, b0, acc[1][0]);
            acc[1][1] = rn_mfma(a1, b1, acc[1][1]);
        }
    } else {
        const int n_chunk = Cin / CV_CK;
        // fragments of one 32-channel output tile: [chunk][tap][k-step]
        const int64_t tile_frags = (int64_t)n_chunk * 9 * (CV_CK / 16);
        const rn_half* wf0 = wfrag + (int64_t)(cg * 2) * tile_frags * RN_FRAG_HALFS;
        const rn_half* wf1 = wf0 + tile_frags * RN_FRAG_HALFS;
        for (int ch = 0; ch < n_chunk; ++ch) {
            if (ch) __syncthreads();             // the previous chunk's reads are done
            for (int i = threadIdx.x; i < CV_HH * CV_HW * (CV_CK / 8); i += LP_THREADS) {
                const int p = i >> 3, v = i & 7;
                const int y = y0 - 1 + p / CV_HW, x = x0 - 1 + p % CV_HW;
                lp_i4 val = {0, 0, 0, 0};
                if (y >= 0 && y < H && x >= 0 && x < W)
                    val = *reinterpret_cast<const lp_i4*>(
                        src + ((int64_t)y * W + x) * Cin + ch * CV_CK + v * 8);
                *reinterpret_cast<lp_i4*>(lds + p * CV_PS + v * 8) = val;
            }
            __syncthreads();
            const int f0 = ch * 9 * (CV_CK / 16);
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                const int dy = tap / 3, dx = tap % 3;
                const rn_half* bp = lds + ((wave * 2 + dy) * CV_HW + r + dx) * CV_PS + 8 * h;
#pragma unroll
                for (int ks = 0; ks < CV_CK / 16; ++ks) {
                    const int f = f0 + tap * (CV_CK / 16) + ks;
                    const half8 a0 = rn_frag(wf0, f), a1 = rn_frag(wf1, f);
                    const half8 b0 = *reinterpret_cast<const half8*>(bp + ks * 16);
                    const half8 b1 = *reinterpret_cast<const half8*>(bp + CV_HW * CV_PS + ks * 16);
                    acc[0][0] = rn_mfma(a0, b0, acc[0][0]);
                    acc[0][1] = rn_mfma(a0, b1, acc[0][1]);
                    acc[1][0] = rn_mfma(a1, b0, acc[1][0]);
                    acc[1][1] = rn_mfma(a1, b1, acc[1][1]);
                }
            }
        }
    }

    // bias, ReLU, f16: reg i of lane (r, h) is channel (i & 3) + 8 (i >> 2) + 4 h
    // of pixel r, so four consecutive channels leave as one 8-byte store
    const int x = x0 + r;
    if (x >= W) return;
    rn_half* dst = out + img * H * W * Cout;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int y = y0 + wave * 2 + q;
        if (y >= H) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = cg * CV_CO + t * 32 + 8 * g + 4 * h;
                half4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    o[j] = (rn_half)fmaxf(acc[t][q][4 * g + j] + bias[co + j], 0.0f);
                *reinterpret_cast<half4*>(dst + ((int64_t)y * W + x) * Cout + co) = o;
            }
    }
}

// ---- 2 x 2 stride-2 max-pool (floor sizes) ---------------------------------------
// one thread per 8 channels of an output pixel
__global__ void __launch_bounds__(LP_THREADS)
k_maxpool2(int64_t n_vec, int H, int W, int C8, const rn_half* __restrict__ in,
           rn_half* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= n_vec) return;
    const int Ho = H / 2, Wo = W / 2;
    const int v = (int)(i % C8);
    const int64_t p = i / C8;
    const int xo = (int)(p % Wo), yo = (int)((p / Wo) % Ho);
    const int64_t img = p / ((int64_t)Wo * Ho);
    const rn_half* s = in + ((img * H + 2 * yo) * W + 2 * xo) * (int64_t)C8 * 8 + v * 8;
    const int64_t row = (int64_t)W * C8 * 8;
    const half8 a = *reinterpret_cast<const half8*>(s);
    const half8 b = *reinterpret_cast<const half8*>(s + C8 * 8);
    const half8 c = *reinterpret_cast<const half8*>(s + row);
    const half8 d = *reinterpret_cast<const half8*>(s + row + C8 * 8);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const rn_half m0 = a[j] > b[j] ? a[j] : b[j], m1 = c[j] > d[j] ? c[j] : d[j];
        o[j] = m0 > m1 ? m0 : m1;
    }
    *reinterpret_cast<half8*>(out + i * 8) = o;
}

// ---- per-tap distance -------------------------------------------------------------
// Eight lanes share a pixel, each with every eighth group of 8 channels (one
// 16-byte load per image and step).  Per pixel, fp32, every operation rounded
// on its own: s = sum f^2 (a lane's channels ascending, then the 8 lanes by a
// fixed xor tree), den = sqrt(s) + 1e-10, n = f / den for both images,
// d = sum w (n0 - n1)^2 in the same order.  Both images go through the same
// operations, so equal features give d = 0 exactly.  The pixels of a lane
// group are added ascending in double; then the wave's 8 groups, the block's
// waves and the blocks in fixed orders.
__device__ __forceinline__ float lp_sum8(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

__global__ void __launch_bounds__(LP_THREADS)
k_lpips_layer(int64_t n_pix, int C, const rn_half* __restrict__ f0, const rn_half* __restrict__ f1,
              const float* __restrict__ w, double* __restrict__ work) {
    __shared__ double wsum[LP_WAVES];
    const int sub = threadIdx.x & 7;
    const int64_t grp = ((int64_t)blockIdx.x * LP_THREADS + threadIdx.x) >> 3;
    const int64_t n_grp = (int64_t)gridDim.x * (LP_THREADS / 8);
    double acc = 0.0;
    // the trip count is the wave's (its first group's), so the shuffles run
    // with every lane active; a group past the end reads pixel 0 and adds 0
    for (int64_t p0 = grp - (rn_lane() >> 3); p0 < n_pix; p0 += n_grp) {
        const int64_t pp = p0 + (rn_lane() >> 3);
        const bool live = pp < n_pix;
        const int64_t p = live ? pp : 0;
        const rn_half* a = f0 + p * C;
        const rn_half* b = f1 + p * C;
        float s0 = 0.f, s1 = 0.f;
        for (int c = sub * 8; c < C; c += 64) {
            const half8 x = *reinterpret_cast<const half8*>(a + c);
            const half8 y = *reinterpret_cast<const half8*>(b + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xf = (float)x[j], yf = (float)y[j];
                s0 += xf * xf;
                s1 += yf * yf;
            }
        }
        const float d0 = sqrtf(lp_sum8(s0)) + 1e-10f, d1 = sqrtf(lp_sum8(s1)) + 1e-10f;
        float d = 0.f;
        for (int c = sub * 8; c < C; c += 64) {
            const half8 x = *reinterpret_cast<const half8*>(a + c);
            const half8 y = *reinterpret_cast<const half8*>(b + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float df = (float)x[j] / d0 - (float)y[j] / d1;
                d += w[c + j] * (df * df);
            }
        }
        const float dp = lp_sum8(d);
        if (live) acc += (double)dp;
    }
    // the wave's 8 groups: lanes 0, 8, ..., 56 in that order
    double ws = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) ws += __shfl(acc, 8 * g);
    if (rn_lane() == 0) wsum[threadIdx.x / RN_WAVE] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
        for (int i = 1; i < LP_WAVES; ++i) s += wsum[i];
        work[blockIdx.x] = s;
    }
}

// out = sum of work[0, n_part): as metrics.hip's k_sum_partials
__global__ void __launch_bounds__(LP_THREADS)
k_lpips_sum_partials(const double* __restrict__ work, int n_part, double* __restrict__ out) {
    __shared__ double red[LP_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_part; i += LP_THREADS) s += work[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = LP_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int rn_lpips_prepare(const float* rgb, int64_t n_pix, void* out_f16, void* stream) {
    RN_CHECK_ARG(n_pix >= 0 && n_pix <= ((int64_t)1 << 40), "bad sizes");
    if (n_pix == 0) return 0;
    RN_CHECK_ARG(rgb && out_f16, "null pointer");
    const int64_t n = 3 * n_pix;
    const int64_t blocks = (n + LP_THREADS - 1) / LP_THREADS;
    RN_CHECK_ARG(blocks <= 0x7fffffff, "image too large");
    k_lpips_prepare<<<(int)blocks, LP_THREADS, 0, (hipStream_t)stream>>>(n, rgb,
                                                                         (rn_half*)out_f16);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_conv3x3_relu_f16(const void* in, const void* wfrag, const float* bias, int32_t n_img,
                        int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* out,
                        void* stream) {
    RN_CHECK_ARG(n_img >= 1 && n_img <= 65535 && H >= 1 && W >= 1, "bad sizes");
    RN_CHECK_ARG(Cin == 3 || (Cin >= CV_CK && Cin % CV_CK == 0),
                 "Cin must be 3 or a multiple of 64");
    RN_CHECK_ARG(Cout >= CV_CO && Cout % CV_CO == 0 && Cout / CV_CO <= 65535,
                 "Cout must be a multiple of 64");
    RN_CHECK_ARG(in && wfrag && bias && out, "null pointer");
    RN_CHECK_ARG(aligned16(wfrag) && ((uintptr_t)out & 7) == 0 && (Cin == 3 || aligned16(in)),
                 "in and wfrag must be 16-byte aligned, out 8-byte");
    const int tiles_x = nblk(W, CV_TW), tiles_y = nblk(H, CV_TH);
    const int64_t tiles = (int64_t)tiles_x * tiles_y;
    RN_CHECK_ARG(tiles <= 0x7fffffff, "image too large");
    const dim3 grid((unsigned)tiles, (unsigned)(Cout / CV_CO), (unsigned)n_img);
    if (Cin == 3)
        k_conv3x3_relu<true><<<grid, LP_THREADS, 0, (hipStream_t)stream>>>(
            H, W, Cin, Cout, (const rn_half*)in, (const rn_half*)wfrag, bias, (rn_half*)out,
            tiles_x);
    else
        k_conv3x3_relu<false><<<grid, LP_THREADS, 0, (hipStream_t)stream>>>(
            H, W, Cin, Cout, (const rn_half*)in, (const rn_half*)wfrag, bias, (rn_half*)out,
            tiles_x);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_maxpool2_f16(const void* in, int32_t n_img, int32_t H, int32_t W, int32_t C, void* out,
                    void* stream) {
    RN_CHECK_ARG(n_img >= 1 && H >= 2 && W >= 2, "H and W must be at least 2");
    RN_CHECK_ARG(C >= 8 && C % 8 == 0, "C must be a multiple of 8");
    RN_CHECK_ARG(in && out, "null pointer");
    RN_CHECK_ARG(aligned16(in) && aligned16(out), "in and out must be 16-byte aligned");
    const int64_t n_vec = (int64_t)n_img * (H / 2) * (W / 2) * (C / 8);
    const int64_t blocks = (n_vec + LP_THREADS - 1) / LP_THREADS;
    RN_CHECK_ARG(blocks <= 0x7fffffff, "image too large");
    k_maxpool2<<<(int)blocks, LP_THREADS, 0, (hipStream_t)stream>>>(
        n_vec, H, W, C / 8, (const rn_half*)in, (rn_half*)out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_lpips_layer(const void* feat0, const void* feat1, const float* lin_w, int64_t n_pix,
                   int32_t C, void* work, double* out_sum, void* stream) {
    RN_CHECK_ARG(n_pix >= 1, "bad sizes");
    RN_CHECK_ARG(C >= 8 && C % 8 == 0, "C must be a multiple of 8");
    RN_CHECK_ARG(feat0 && feat1 && lin_w && work && out_sum, "null pointer");
    RN_CHECK_ARG(aligned16(feat0) && aligned16(feat1), "feat0 and feat1 must be 16-byte aligned");
    // 4 pixels per lane group before the grid is capped
    const int64_t nb = (n_pix + 4 * (LP_THREADS / 8) - 1) / (4 * (LP_THREADS / 8));
    const int blocks = (int)(nb < LP_MAX_BLOCKS ? nb : LP_MAX_BLOCKS);
    k_lpips_layer<<<blocks, LP_THREADS, 0, (hipStream_t)stream>>>(
        n_pix, C, (const rn_half*)feat0, (const rn_half*)feat1, lin_w, (double*)work);
    k_lpips_sum_partials<<<1, LP_THREADS, 0, (hipStream_t)stream>>>((const double*)work, blocks,
                                                                    out_sum);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
