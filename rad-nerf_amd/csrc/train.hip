// Training-step epilogue kernels on either side of the hot path (SURVEY.md
// §8(f) rows 2-3):
//
//  * k_nerf_loss: NeRFLoss.forward (losses.py:44-76) as used by
//    train_ml.py:185-192 -- rgb MSE, opacity entropy, CV^2 of the gate
//    importance, depth-mutual -- fused with its own backward: one pass over
//    the rays writes the loss terms AND the seeds dL/drgb, dL/dopacity,
//    dL/ddepth, dL/dgate that FusedMLRenderer.backward consumes (the
//    reference runs ~15 elementwise torch kernels plus their autograd graph).
//  * k_adam: torch.optim.Adam / apex.FusedAdam(eps=1e-15) (train_ml.py:138-153)
//    over the flat fp32 parameter buffer, one pass that also refreshes the f16
//    copy of the hash table the field kernels gather from.
#include "rn_common.h"
#include "rn_rays.h"
#pragma clang fp contract(off)

namespace {

// loss_out: [0] sum over (B,3) of (rgb - t)^2, [1] sum over B of -o log o
// (lambda applied), [2] cv^2 term (lambda applied), [3] sum over (B,K) of the
// depth-mutual term (lambda applied).  The host divides by the element counts.
// DET (deterministic mode): loss_out is the per-block partial buffer
// [gridDim.x][4] instead -- block b stores its three sums into row b (no
// atomics; block 0 keeps the cv^2 term in [0][2]) and k_loss_sum adds the rows
// in block order.  The per-ray part and the seeds are the same code.
// ROUTED (routed training, rn_nerf_loss_routed / _det): `gate` is gate_used
// (exactly 0 on a dead pair, whose depth is 0 too) and live [B][K] marks the
// pairs that were marched; a dead pair adds nothing to the depth-mutual sum and
// gets d_depth = 0.  The divisor stays B K, so with every pair live the results
// are the dense ones bit for bit.  importance is still the full softmax gate's
// column sums and d_gate the seed on that gate.
template <bool DET, bool ROUTED>
__device__ __forceinline__ void
nerf_loss_body(int64_t B, int K, const float* __restrict__ rgb, const float* __restrict__ target,
               const float* __restrict__ opacity, const float* __restrict__ depth,
               const float* __restrict__ gate, const uint8_t* __restrict__ live,
               const float* __restrict__ importance, float lambda_opacity, float lambda_cv,
               float lambda_dm, float* __restrict__ loss_out, float* __restrict__ d_rgb,
               float* __restrict__ d_opacity, float* __restrict__ d_depth,
               float* __restrict__ d_gate) {
    __shared__ float red[4][RN_WAVE];
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = r < B;
    const bool multi = K > 1;
    // CV^2 of the importance (torch.var: unbiased), losses.py:68-70
    float mu = 0.f, var = 0.f, den = 1.f;
    const bool use_cv = multi && lambda_cv > 0.f;
    if (use_cv) {
        for (int k = 0; k < K; ++k) mu += importance[k];
        mu /= K;
        for (int k = 0; k < K; ++k) { const float e = importance[k] - mu; var += e * e; }
        var /= (K - 1);
        den = mu * mu + 1e-10f;
    }
    float l_rgb = 0.f, l_op = 0.f, l_dm = 0.f;
    if (valid) {
        // rgb MSE, mean over B x 3 (losses.py:51)
        const float inv3b = 1.0f / (3.0f * (float)B);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float e = rgb[3 * r + c] - target[3 * r + c];
            l_rgb += e * e;
            d_rgb[3 * r + c] = 2.0f * e * inv3b;
        }
        // opacity entropy, o = opacity + 1e-10 (losses.py:53-55)
        const float o = opacity[r] + 1e-10f;
        const float lg = logf(o);
        l_op = lambda_opacity * (-o * lg);
        d_opacity[r] = lambda_opacity * (-(lg + 1.0f)) / (float)B;
        // depth-mutual against the detached gate-weighted depth (losses.py:72-73)
        if (multi && lambda_dm > 0.f) {
            float mean_d = 0.f;
            for (int k = 0; k < K; ++k) mean_d += depth[r * K + k] * gate[r * K + k];
            const float s = 2.0f * lambda_dm / ((float)B * K);
            for (int k = 0; k < K; ++k) {
                const float e = depth[r * K + k] - mean_d;
                if (ROUTED && live[r * K + k] == 0) { d_depth[r * K + k] = 0.f; continue; }
                l_dm += lambda_dm * e * e;
                d_depth[r * K + k] = s * e;
            }
        } else {
            for (int k = 0; k < K; ++k) d_depth[r * K + k] = 0.f;
        }
        // dL/dgate from the CV^2 term: every ray adds to importance_k
        for (int k = 0; k < K; ++k) {
            float g = 0.f;
            if (use_cv) {
                const float e = importance[k] - mu;
                g = lambda_cv * ((2.0f * e / (K - 1)) / den - var * (2.0f * mu / K) / (den * den));
            }
            d_gate[r * K + k] = g;
        }
    }
    // block reduction of the three per-ray sums, one atomic each per block
    const int lane = rn_lane(), wid = threadIdx.x / RN_WAVE;
    float v[3] = {l_rgb, l_op, l_dm};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float x = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0) red[q][wid] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float x = 0.f;
        for (int w = 0; w < (int)(blockDim.x / RN_WAVE); ++w) x += red[threadIdx.x][w];
        const int q = threadIdx.x == 2 ? 3 : threadIdx.x;
        if (DET) loss_out[4 * (size_t)blockIdx.x + q] = x;
        else atomicAdd(&loss_out[q], x);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && use_cv) loss_out[2] = lambda_cv * var / den;
}

template <bool DET>
__global__ void __launch_bounds__(256)
k_nerf_loss(int64_t B, int K, const float* __restrict__ rgb, const float* __restrict__ target,
            const float* __restrict__ opacity, const float* __restrict__ depth,
            const float* __restrict__ gate, const float* __restrict__ importance,
            float lambda_opacity, float lambda_cv, float lambda_dm, float* __restrict__ loss_out,
            float* __restrict__ d_rgb, float* __restrict__ d_opacity, float* __restrict__ d_depth,
            float* __restrict__ d_gate) {
    nerf_loss_body<DET, false>(B, K, rgb, target, opacity, depth, gate, nullptr, importance,
                               lambda_opacity, lambda_cv, lambda_dm, loss_out, d_rgb, d_opacity,
                               d_depth, d_gate);
}

// a kernel of its own, so that the dense one keeps its code
template <bool DET>
__global__ void __launch_bounds__(256)
k_nerf_loss_routed(int64_t B, int K, const float* __restrict__ rgb,
                   const float* __restrict__ target, const float* __restrict__ opacity,
                   const float* __restrict__ depth, const float* __restrict__ gate_used,
                   const uint8_t* __restrict__ live, const float* __restrict__ importance,
                   float lambda_opacity, float lambda_cv, float lambda_dm,
                   float* __restrict__ loss_out, float* __restrict__ d_rgb,
                   float* __restrict__ d_opacity, float* __restrict__ d_depth,
                   float* __restrict__ d_gate) {
    nerf_loss_body<DET, true>(B, K, rgb, target, opacity, depth, gate_used, live, importance,
                              lambda_opacity, lambda_cv, lambda_dm, loss_out, d_rgb, d_opacity,
                              d_depth, d_gate);
}

// deterministic mode: the blocks' partial sums of k_nerf_loss<true> in block
// order, one thread per term; the cv^2 term is block 0's
__global__ void k_loss_sum(const float* __restrict__ part, int n_blocks, int use_cv,
                           float* __restrict__ loss_out) {
    const int q = threadIdx.x;
    if (q >= 4) return;
    if (q == 2) { loss_out[2] = use_cv ? part[2] : 0.f; return; }
    float acc = 0.f;
    for (int b = 0; b < n_blocks; ++b) acc += part[4 * (size_t)b + q];
    loss_out[q] = acc;
}

// Depth supervision (rn_depth_loss), after k_nerf_loss and the guided epilogue:
// the expected-depth term and the ray-termination second moment (dvar_k, from
// the composite) with their seeds, added into the loss kernel's.
// part: [blocks][2] (mean term, second-moment term), block sums by
// a fixed xor butterfly per wave and the four waves in order
__global__ void __launch_bounds__(256)
k_depth_loss(int64_t B, int K, const float* __restrict__ depth, const float* __restrict__ gate,
             const float* __restrict__ dvar_k, const float* __restrict__ target_t,
             const float* __restrict__ ray_weight, float lambda_d, float lambda_v,
             float* __restrict__ part, float* __restrict__ d_depth, float* __restrict__ d_gate,
             float* __restrict__ d_dvar) {
    __shared__ float red[2][256 / RN_WAVE];
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float l_d = 0.f, l_v = 0.f;
    if (r < B) {
        const float z = target_t[r];
        const bool m = z > 0.f;
        const float rw = ray_weight ? ray_weight[r] : 1.0f;
        if (lambda_d > 0.f && m) {
            float mean_d = 0.f;
            for (int k = 0; k < K; ++k) mean_d += gate[r * K + k] * depth[r * K + k];
            const float e = mean_d - z;
            l_d = lambda_d * (e * e);
            const float s = ((2.0f * lambda_d / (float)B) * e) * rw;
            for (int k = 0; k < K; ++k) {
                const float g = gate[r * K + k], D = depth[r * K + k];
                d_depth[r * K + k] += s * g;
                d_gate[r * K + k] += s * D;
            }
        }
        if (dvar_k) {
            const float s = m && lambda_v > 0.f ? (lambda_v / (float)B) * rw : 0.f;
            float acc = 0.f;
            for (int k = 0; k < K; ++k) {
                const float g = gate[r * K + k], V = dvar_k[(int64_t)k * B + r];
                if (m) acc += g * V;
                d_dvar[(int64_t)k * B + r] = s * g;
                if (s != 0.f) d_gate[r * K + k] += s * V;
            }
            l_v = lambda_v * acc;
        }
    }
    const int lane = rn_lane(), wid = threadIdx.x / RN_WAVE;
    float v[2] = {l_d, l_v};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float x = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0) red[q][wid] = x;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        float x = 0.f;
        for (int w = 0; w < (int)(blockDim.x / RN_WAVE); ++w) x += red[threadIdx.x][w];
        part[2 * (size_t)blockIdx.x + threadIdx.x] = x;
    }
}

// the blocks' partial sums in block order, one thread per term
__global__ void k_depth_loss_sum(const float* __restrict__ part, int n_blocks,
                                 float* __restrict__ loss_out) {
    const int q = threadIdx.x;
    if (q >= 2) return;
    float acc = 0.f;
    for (int b = 0; b < n_blocks; ++b) acc += part[2 * (size_t)b + q];
    loss_out[q] = acc;
}

// out[i] = (...((out[i] + part[0][i]) + part[1][i]) + ...) + part[n_slots - 1][i]:
// one thread per i, plain fp32 adds in ascending slot order (the order is the
// contract: include/radnerf.h), loads coalesced over i
__global__ void __launch_bounds__(256)
k_reduce_partials(const float* __restrict__ part, int n_slots, int64_t n,
                  float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = out[i];
    const float* p = part + i;
#pragma unroll 8
    for (int s = 0; s < n_slots; ++s) acc += p[(size_t)s * n];
    out[i] = acc;
}

// out[c] = sum over rows of x[r][c], block c = column c, one wave: lane l adds
// the sums of the 32-row tiles l, l + 64, ... in ascending order (each tile
// summed row by row from 0), then a fixed xor butterfly over the lanes.  The
// tree depends on (rows, cols) alone; no atomics.
constexpr int RN_COLSUM_TILE = 32;

__global__ void __launch_bounds__(RN_WAVE)
k_colsum_ordered(const float* __restrict__ x, int64_t rows, int cols, float* __restrict__ out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t n_tiles = (rows + RN_COLSUM_TILE - 1) / RN_COLSUM_TILE;
    float acc = 0.f;
    for (int64_t t = lane; t < n_tiles; t += RN_WAVE) {
        const int64_t r0 = t * RN_COLSUM_TILE;
        const int64_t r1 = r0 + RN_COLSUM_TILE < rows ? r0 + RN_COLSUM_TILE : rows;
        float s = 0.f;
        for (int64_t r = r0; r < r1; ++r) s += x[r * cols + c];
        acc += s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) out[c] = acc;
}

// Adam with bias correction, in torch.optim.Adam's operation order (no weight
// decay; apex FusedAdam with weight_decay 0 is the same update):
//   m = lerp(m, g, 1-b1) ;  v = v*b2 + (1-b2)*g*g
//   p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
// half_out (optional): f16 copy of p[0, n_half) written in the same pass.
__global__ void __launch_bounds__(256)
k_adam(int64_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
       float* __restrict__ v, float step_size, float omb1, float b2, float omb2, float eps,
       float bc2_sqrt, float grad_scale, _Float16* __restrict__ half_out, int64_t n_half) {
    // torch.optim.Adam (single-tensor form): exp_avg.lerp_(g, 1-b1);
    // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2);
    // p.addcdiv_(exp_avg, exp_avg_sq.sqrt() / sqrt(bc2) + eps, -lr/bc1)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i] * grad_scale;
        const float m0 = m[i];
        const float mi = m0 + omb1 * (gi - m0);
        const float vi = v[i] * b2 + omb2 * (gi * gi);
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        const float pi = p[i] - step_size * (mi / denom);
        p[i] = pi;
        if (i < n_half) half_out[i] = (_Float16)pi;
    }
}

// train_ml.py:84-96 + datasets/ray_utils.py:45-70 (get_rays) for a batch of
// (image, pixel) picks: rays_d = R dir, rays_o = T, imgs_d = R mean_dir
// (rn_rays.h rn_rays_plain, shared with the batch sampler).
__global__ void __launch_bounds__(256)
k_get_rays(int64_t n, const float* __restrict__ dirs, const float* __restrict__ poses,
           const int64_t* __restrict__ img_idx, const int64_t* __restrict__ pix_idx,
           const float* __restrict__ mean_dir, float* __restrict__ rays_o,
           float* __restrict__ rays_d, float* __restrict__ imgs_d) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float* P = poses + 12 * (img_idx ? img_idx[r] : 0);     // (3, 4) row-major
    const float* d = dirs + 3 * (pix_idx ? pix_idx[r] : r);
    rn_rays_plain(r, P, d, mean_dir, rays_o, rays_d, imgs_d);
}

// k_get_rays with the per-image refinement applied first (--optimize_ext:
// train_ml.py:90-93, ray_utils.py:73-100; rn_rays.h rn_rays_pose).
__global__ void __launch_bounds__(256)
k_get_rays_pose(int64_t n, const float* __restrict__ dirs, const float* __restrict__ poses,
                const float* __restrict__ dR, const float* __restrict__ dT,
                const int64_t* __restrict__ img_idx, const int64_t* __restrict__ pix_idx,
                const float* __restrict__ mean_dir, float* __restrict__ rays_o,
                float* __restrict__ rays_d, float* __restrict__ imgs_d) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t im = img_idx[r];
    const float* P = poses + 12 * im;                             // (3, 4) row-major
    const float* d = dirs + 3 * (pix_idx ? pix_idx[r] : r);
    rn_rays_pose(r, im, P, d, dR, dT, mean_dir, rays_o, rays_d, imgs_d);
}

// Backward of k_get_rays_pose into dL/ddR, dL/ddT: one 256-thread block per
// image.  The block scans the batch's image indices (B int64 from L2 per
// image, no sort), each thread sums its matching rays in ascending ray order,
// then a fixed xor-butterfly per wave and a fixed-order sum over the four
// waves: no atomics, bit-identical from run to run.  Every image's rows are
// written (zeros when the batch holds none of its rays).
//   dL/dT = sum g_o ;  G = sum g_d (x) d_c + (sum g_i) (x) mean_dir ;
//   M = dL/dA = G R0^T ;
//   dL/dv_k = a <M, E_k> + b <M, E_k K + K E_k>
//             + (a' <M, K> + b' <M, K^2>) v_k / |v|        (0 at |v| = 0)
constexpr int RN_POSE_ACC = 15;     // g_o (3), g_d (x) d_c (9), g_i (3)

__global__ void __launch_bounds__(256)
k_get_rays_pose_bw(int64_t n, const float* __restrict__ dirs, const float* __restrict__ poses,
                   const float* __restrict__ dR, const int64_t* __restrict__ img_idx,
                   const int64_t* __restrict__ pix_idx, const float* __restrict__ mean_dir,
                   const float* __restrict__ g_o, const float* __restrict__ g_d,
                   const float* __restrict__ g_i, float* __restrict__ d_dR,
                   float* __restrict__ d_dT) {
    __shared__ float red[256 / RN_WAVE][RN_POSE_ACC];
    const int64_t im = blockIdx.x;
    float acc[RN_POSE_ACC];
#pragma unroll
    for (int q = 0; q < RN_POSE_ACC; ++q) acc[q] = 0.f;
#pragma unroll 4
    for (int64_t r = threadIdx.x; r < n; r += 256) {
        if (img_idx[r] != im) continue;
        const float* d = dirs + 3 * (pix_idx ? pix_idx[r] : r);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            acc[i] += g_o[3 * r + i];
            const float gd = g_d[3 * r + i];
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 + 3 * i + j] += gd * d[j];
            if (g_i) acc[12 + i] += g_i[3 * r + i];
        }
    }
    const int lane = rn_lane(), wid = threadIdx.x / RN_WAVE;
#pragma unroll
    for (int q = 0; q < RN_POSE_ACC; ++q) {
        float x = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0) red[wid][q] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float s[RN_POSE_ACC];
#pragma unroll
    for (int q = 0; q < RN_POSE_ACC; ++q) {
        float x = red[0][q];
        for (int w = 1; w < 256 / RN_WAVE; ++w) x += red[w][q];
        s[q] = x;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) d_dT[3 * im + i] = s[i];
    const float* P = poses + 12 * im;
    float G[9], R0t[9], M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            G[3 * i + j] = g_i ? s[3 + 3 * i + j] + s[12 + i] * mean_dir[j] : s[3 + 3 * i + j];
            R0t[3 * i + j] = P[4 * j + i];
        }
    mm3(G, R0t, M);
    float v[3] = {0.f, 0.f, 0.f};
    if (dR) { v[0] = dR[3 * im]; v[1] = dR[3 * im + 1]; v[2] = dR[3 * im + 2]; }
    const float nv = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const RodCoef c = rod_coef(nv + 1e-7f);
    float K[9], K2[9];
    skew3(v, K);
    mm3(K, K, K2);
    // the theta path: d theta / d v_k = v_k / |v|, torch's subgradient 0 at 0
    const float radial = nv > 0.f ? (c.da * dot9(M, K) + c.db * dot9(M, K2)) / nv : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float e[3] = {0.f, 0.f, 0.f}, E[9], EK[9], KE[9];
        e[k] = 1.f;
        skew3(e, E);                                               // E_k = dK / dv_k
        mm3(E, K, EK);
        mm3(K, E, KE);
        d_dR[3 * im + k] = c.a * dot9(M, E) + c.b * (dot9(M, EK) + dot9(M, KE)) + radial * v[k];
    }
}

}  // namespace

extern "C" {

int rn_nerf_loss(const float* rgb, const float* target_rgb, const float* opacity,
                 const float* depth, const float* gate, const float* importance, int64_t n_rays,
                 int32_t n_models, float lambda_opacity, float lambda_cv, float lambda_dm,
                 float* loss_out, float* dL_drgb, float* dL_dopacity, float* dL_ddepth,
                 float* dL_dgate, void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1, "bad sizes");
    RN_CHECK_ARG(rgb && target_rgb && opacity && depth && gate && importance && loss_out &&
                 dL_drgb && dL_dopacity && dL_ddepth && dL_dgate, "null pointer");
    if (hipMemsetAsync(loss_out, 0, 4 * sizeof(float), (hipStream_t)stream) != hipSuccess) {
        rn_set_error("rn_nerf_loss: hipMemsetAsync failed");
        return 2;
    }
    k_nerf_loss<false><<<nblk(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
        n_rays, n_models, rgb, target_rgb, opacity, depth, gate, importance, lambda_opacity,
        lambda_cv, lambda_dm, loss_out, dL_drgb, dL_dopacity, dL_ddepth, dL_dgate);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_nerf_loss_det(const float* rgb, const float* target_rgb, const float* opacity,
                     const float* depth, const float* gate, const float* importance,
                     int64_t n_rays, int32_t n_models, float lambda_opacity, float lambda_cv,
                     float lambda_dm, float* loss_out, float* part, float* dL_drgb,
                     float* dL_dopacity, float* dL_ddepth, float* dL_dgate, void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1, "bad sizes");
    RN_CHECK_ARG(rgb && target_rgb && opacity && depth && gate && importance && loss_out && part &&
                 dL_drgb && dL_dopacity && dL_ddepth && dL_dgate, "null pointer");
    RN_CHECK_ARG(nblk(n_rays, 256) <= 0x7fffffff / 4, "too many rays");
    const int nb = nblk(n_rays, 256);
    // the same test as the kernel's use_cv
    const int use_cv = n_models > 1 && lambda_cv > 0.f;
    k_nerf_loss<true><<<nb, 256, 0, (hipStream_t)stream>>>(
        n_rays, n_models, rgb, target_rgb, opacity, depth, gate, importance, lambda_opacity,
        lambda_cv, lambda_dm, part, dL_drgb, dL_dopacity, dL_ddepth, dL_dgate);
    RN_CHECK_LAUNCH();
    k_loss_sum<<<1, 64, 0, (hipStream_t)stream>>>(part, nb, use_cv, loss_out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_nerf_loss_routed(const float* rgb, const float* target_rgb, const float* opacity,
                        const float* depth, const float* gate_used, const uint8_t* live,
                        const float* importance, int64_t n_rays, int32_t n_models,
                        float lambda_opacity, float lambda_cv, float lambda_dm, float* loss_out,
                        float* dL_drgb, float* dL_dopacity, float* dL_ddepth, float* dL_dgate,
                        void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1, "bad sizes");
    RN_CHECK_ARG(rgb && target_rgb && opacity && depth && gate_used && live && importance &&
                 loss_out && dL_drgb && dL_dopacity && dL_ddepth && dL_dgate, "null pointer");
    RN_CHECK_HIP(hipMemsetAsync(loss_out, 0, 4 * sizeof(float), (hipStream_t)stream),
                 "loss memset");
    k_nerf_loss_routed<false><<<nblk(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
        n_rays, n_models, rgb, target_rgb, opacity, depth, gate_used, live, importance,
        lambda_opacity, lambda_cv, lambda_dm, loss_out, dL_drgb, dL_dopacity, dL_ddepth, dL_dgate);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_nerf_loss_routed_det(const float* rgb, const float* target_rgb, const float* opacity,
                            const float* depth, const float* gate_used, const uint8_t* live,
                            const float* importance, int64_t n_rays, int32_t n_models,
                            float lambda_opacity, float lambda_cv, float lambda_dm,
                            float* loss_out, float* part, float* dL_drgb, float* dL_dopacity,
                            float* dL_ddepth, float* dL_dgate, void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1, "bad sizes");
    RN_CHECK_ARG(rgb && target_rgb && opacity && depth && gate_used && live && importance &&
                 loss_out && part && dL_drgb && dL_dopacity && dL_ddepth && dL_dgate,
                 "null pointer");
    RN_CHECK_ARG(nblk(n_rays, 256) <= 0x7fffffff / 4, "too many rays");
    const int nb = nblk(n_rays, 256);
    const int use_cv = n_models > 1 && lambda_cv > 0.f;
    k_nerf_loss_routed<true><<<nb, 256, 0, (hipStream_t)stream>>>(
        n_rays, n_models, rgb, target_rgb, opacity, depth, gate_used, live, importance,
        lambda_opacity, lambda_cv, lambda_dm, part, dL_drgb, dL_dopacity, dL_ddepth, dL_dgate);
    RN_CHECK_LAUNCH();
    k_loss_sum<<<1, 64, 0, (hipStream_t)stream>>>(part, nb, use_cv, loss_out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_depth_loss(const float* depth, const float* gate, const float* dvar_k,
                  const float* target_t, const float* ray_weight, int64_t n_rays,
                  int32_t n_models, float lambda_depth, float lambda_depth_var, float* loss_out,
                  float* part, float* dL_ddepth, float* dL_dgate, float* dL_ddvar, void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1, "bad sizes");
    RN_CHECK_ARG(nblk(n_rays, 256) <= 0x7fffffff / 2, "too many rays");
    RN_CHECK_ARG(depth && gate && target_t && loss_out && part && dL_ddepth && dL_dgate,
                 "null pointer");
    RN_CHECK_ARG((dvar_k == nullptr) == (dL_ddvar == nullptr),
                 "dvar_k and dL_ddvar must be given together");
    const int nb = nblk(n_rays, 256);
    k_depth_loss<<<nb, 256, 0, (hipStream_t)stream>>>(
        n_rays, n_models, depth, gate, dvar_k, target_t, ray_weight, lambda_depth,
        lambda_depth_var, part, dL_ddepth, dL_dgate, dL_ddvar);
    RN_CHECK_LAUNCH();
    k_depth_loss_sum<<<1, 64, 0, (hipStream_t)stream>>>(part, nb, loss_out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_reduce_partials(const float* part, int32_t n_slots, int64_t n, float* out, void* stream) {
    RN_CHECK_ARG(n_slots >= 1 && n >= 0, "bad sizes");
    RN_CHECK_ARG(part && out, "null pointer");
    if (n == 0) return 0;
    RN_CHECK_ARG((n + 255) / 256 <= 0x7fffffff, "n too large");
    k_reduce_partials<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(part, n_slots, n, out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_colsum_ordered(const float* x, int64_t rows, int32_t cols, float* out, void* stream) {
    RN_CHECK_ARG(rows >= 0 && cols >= 1 && cols <= 16, "rows >= 0, cols in 1..16");
    RN_CHECK_ARG(out && (rows == 0 || x), "null pointer");
    k_colsum_ordered<<<cols, RN_WAVE, 0, (hipStream_t)stream>>>(x, rows, cols, out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
            double lr, double beta1, double beta2, double eps, int32_t step, float grad_scale,
            void* params_f16, int64_t n_f16, void* stream) {
    RN_CHECK_ARG(n >= 0 && step >= 1 && n_f16 >= 0 && n_f16 <= n, "bad sizes");
    if (n == 0) return 0;
    RN_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && (n_f16 == 0 || params_f16),
                 "null pointer");
    // step constants in double, as torch / apex compute them on the host,
    // rounded once to the kernel's fp32
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const int64_t nb = nblk(n, 256);
    const int blocks = (int)(nb < 256 * 16 ? nb : 256 * 16);
    k_adam<<<blocks, 256, 0, (hipStream_t)stream>>>(
        n, params, grads, exp_avg, exp_avg_sq, (float)(lr / bc1), (float)(1.0 - beta1),
        (float)beta2, (float)(1.0 - beta2), (float)eps, (float)sqrt(bc2), grad_scale,
        (_Float16*)params_f16, n_f16);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_get_rays(const float* directions, const float* poses, const int64_t* img_idxs,
                const int64_t* pix_idxs, int64_t n_rays, const float* mean_dir, float* rays_o,
                float* rays_d, float* imgs_d, void* stream) {
    RN_CHECK_ARG(n_rays >= 0, "bad sizes");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(directions && poses && rays_o && rays_d && (!imgs_d || mean_dir), "null pointer");
    k_get_rays<<<nblk(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
        n_rays, directions, poses, img_idxs, pix_idxs, mean_dir, rays_o, rays_d, imgs_d);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_get_rays_pose(const float* directions, const float* poses, const float* dR,
                     const float* dT, const int64_t* img_idxs, const int64_t* pix_idxs,
                     int64_t n_rays, const float* mean_dir, float* rays_o, float* rays_d,
                     float* imgs_d, void* stream) {
    RN_CHECK_ARG(n_rays >= 0, "bad sizes");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(directions && poses && img_idxs && rays_o && rays_d && (!imgs_d || mean_dir),
                 "null pointer");
    k_get_rays_pose<<<nblk(n_rays, 256), 256, 0, (hipStream_t)stream>>>(
        n_rays, directions, poses, dR, dT, img_idxs, pix_idxs, mean_dir, rays_o, rays_d, imgs_d);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_get_rays_pose_bw(const float* directions, const float* poses, const float* dR,
                        const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays,
                        int64_t n_images, const float* mean_dir, const float* dL_drays_o,
                        const float* dL_drays_d, const float* dL_dimgs_d, float* dL_ddR,
                        float* dL_ddT, void* stream) {
    RN_CHECK_ARG(n_rays >= 0 && n_images >= 0 && n_images <= 0x7fffffff, "bad sizes");
    RN_CHECK_ARG(n_images == 0 || (dL_ddR && dL_ddT), "null pointer");
    if (n_images == 0) return 0;
    if (n_rays == 0) {
        // no ray: every row is zero, and no kernel is needed to say so
        if (hipMemsetAsync(dL_ddR, 0, 3 * n_images * sizeof(float), (hipStream_t)stream) !=
                hipSuccess ||
            hipMemsetAsync(dL_ddT, 0, 3 * n_images * sizeof(float), (hipStream_t)stream) !=
                hipSuccess) {
            rn_set_error("rn_get_rays_pose_bw: hipMemsetAsync failed");
            return 2;
        }
        return 0;
    }
    RN_CHECK_ARG(directions && poses && img_idxs && dL_drays_o && dL_drays_d &&
                 (!dL_dimgs_d || mean_dir), "null pointer");
    k_get_rays_pose_bw<<<(int)n_images, 256, 0, (hipStream_t)stream>>>(
        n_rays, directions, poses, dR, img_idxs, pix_idxs, mean_dir, dL_drays_o, dL_drays_d,
        dL_dimgs_d, dL_ddR, dL_ddT);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
