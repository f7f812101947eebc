// Gate-sparse test-time render, first half: which (ray, sub-NeRF) pairs the
// gate keeps (rn_gate_select; rn_render_test_list, render.hip, renders them).
//
// Reference: ml_rendering.py:33-36,65-68 weights every sub-NeRF's render by the
// softmax gate; Ray_Gate.forward (networks.py:1087-1093) returns a third value,
// top_k_indices, hard-wired to None: sparse gating was planned and not built.
// The semantics here are this project's (include/radnerf.h states them).
//
// Three launches on the caller's stream, no host synchronisation, no atomics:
//   k_gs_mark   lane per ray, the row's K <= 16 gates in registers: live,
//               gate_used, zeros in the dead slots of the per-pair outputs, and
//               the block's live count per sub-NeRF (ballots) into `work`;
//   k_gs_scan   one block per sub-NeRF: exclusive scan of the <= 1024 block
//               counts in place, the total into count[k];
//   k_gs_write  recomputes the ballots from `live` and writes ray r at
//               block offset + rank inside the block: ascending ray order.
// Block b owns the contiguous rays [b * span, (b + 1) * span), span a multiple
// of 256, so the lists are a pure function of the gate.
#include "rn_common.h"
#pragma clang fp contract(off)

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / RN_WAVE;
constexpr int GS_MAX_K = 16;
constexpr int GS_MAX_BLOCKS = RN_GATE_SELECT_WORK_BYTES / (GS_MAX_K * 4);   // 1024
static_assert(GS_MAX_BLOCKS == 4 * GS_THREADS, "k_gs_scan takes 4 block counts per thread");

struct SelectArgs {
    const float* gate;            // [n][K]
    int n, K, span;               // span: rays per block (a multiple of GS_THREADS)
    float gate_min; int topk, renorm;
    uint8_t* live; float* gate_used;              // [n][K]
    float* opacity; float* depth; float* rgb;     // [K][n], [K][n], [K][n][3] (or all NULL)
    int32_t* n_samples;                           // [K][n]
    int32_t* list; int32_t* count;                // [K][n], [K]
    int32_t* work;                                // [GS_MAX_K][GS_MAX_BLOCKS]
};

// lanes below this one
__device__ __forceinline__ int lanes_below(unsigned long long b) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0));
}

__global__ void __launch_bounds__(GS_THREADS) k_gs_mark(SelectArgs a) {
    __shared__ int wcnt[GS_WAVES][GS_MAX_K];
    const int wid = threadIdx.x / RN_WAVE, lane = rn_lane();
    const int64_t first = (int64_t)blockIdx.x * a.span;
    const int64_t end = first + a.span < a.n ? first + a.span : a.n;
    int run = 0;                  // lane i < K of wave 0: the block's count of sub-NeRF i
    for (int64_t base = first; base < end; base += GS_THREADS) {
        const int64_t r = base + threadIdx.x;
        const bool in = r < end;
        // the row; slots past K hold -inf and never outrank a gate
        float g[GS_MAX_K];
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i)
            g[i] = (in && i < a.K) ? a.gate[r * a.K + i] : -__builtin_inff();
        // live: rank by gate descending, index ascending; the first maximal
        // gate (rank 0) is live whatever gate_min says
        uint32_t lv = 0;
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < GS_MAX_K; ++j)
                rank += (g[j] > g[i] || (j < i && g[j] == g[i])) ? 1 : 0;
            const bool l = in && i < a.K && rank < a.topk && (g[i] >= a.gate_min || rank == 0);
            lv |= (l ? 1u : 0u) << i;
        }
        // S: the live gates summed in index order (0 + g is g)
        float S = 0.f;
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i)
            if ((lv >> i) & 1u) S = S + g[i];
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i) {
            const bool l = (lv >> i) & 1u;       // never set for i >= K or a ray past the end
            if (in && i < a.K) {
                const int64_t o = r * a.K + i;
                a.live[o] = l ? 1 : 0;
                a.gate_used[o] = l ? (a.renorm ? g[i] / S : g[i]) : 0.0f;
                if (!l && a.opacity) {
                    const int64_t s = (int64_t)i * a.n + r;
                    a.opacity[s] = 0.f; a.depth[s] = 0.f;
                    a.rgb[3 * s] = 0.f; a.rgb[3 * s + 1] = 0.f; a.rgb[3 * s + 2] = 0.f;
                    a.n_samples[s] = 0;
                }
            }
            const int c = __popcll(__ballot(l));
            if (lane == 0) wcnt[wid][i] = c;
        }
        __syncthreads();
        if (threadIdx.x < a.K) {
            for (int w = 0; w < GS_WAVES; ++w) run += wcnt[w][threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x < a.K) a.work[threadIdx.x * GS_MAX_BLOCKS + blockIdx.x] = run;
}

// block k: work[k][0, nb) -> its exclusive prefix sums, the total -> count[k]
__global__ void __launch_bounds__(GS_THREADS) k_gs_scan(int32_t* __restrict__ work, int nb,
                                                         int32_t* __restrict__ count) {
    __shared__ int wtot[GS_WAVES];
    int32_t* w = work + blockIdx.x * GS_MAX_BLOCKS;
    const int e0 = 4 * threadIdx.x;
    int v[4], mine = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = e0 + q < nb ? w[e0 + q] : 0;
        mine += v[q];
    }
    const int incl = rn_wave_incl_sum_i(mine);
    const int wid = threadIdx.x / RN_WAVE;
    if (rn_lane() == RN_WAVE - 1) wtot[wid] = incl;
    __syncthreads();
    int off = incl - mine, total = 0;
    for (int q = 0; q < GS_WAVES; ++q) {
        if (q < wid) off += wtot[q];
        total += wtot[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (e0 + q < nb) w[e0 + q] = off;
        off += v[q];
    }
    if (threadIdx.x == 0) count[blockIdx.x] = total;
}

__global__ void __launch_bounds__(GS_THREADS) k_gs_write(SelectArgs a) {
    __shared__ int wcnt[GS_WAVES][GS_MAX_K];
    const int wid = threadIdx.x / RN_WAVE, lane = rn_lane();
    const int64_t first = (int64_t)blockIdx.x * a.span;
    const int64_t end = first + a.span < a.n ? first + a.span : a.n;
    // every lane keeps sub-NeRF i's running offset of the block in run[i]
    int run[GS_MAX_K];
#pragma unroll
    for (int i = 0; i < GS_MAX_K; ++i)
        run[i] = i < a.K ? a.work[i * GS_MAX_BLOCKS + blockIdx.x] : 0;
    for (int64_t base = first; base < end; base += GS_THREADS) {
        const int64_t r = base + threadIdx.x;
        const bool in = r < end;
        unsigned long long bal[GS_MAX_K];
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i) {
            bal[i] = __ballot(in && i < a.K && a.live[r * a.K + i] != 0);
            if (lane == 0) wcnt[wid][i] = __popcll(bal[i]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i) {
            int before = 0, all = 0;             // (sub-NeRFs past K: empty ballots, nothing written)
            for (int w = 0; w < GS_WAVES; ++w) {
                const int c = wcnt[w][i];
                before += w < wid ? c : 0;
                all += c;
            }
            if ((bal[i] >> lane) & 1ull) {
                // run + before + rank < count[i] <= n: inside the model's list
                a.list[(int64_t)i * a.n + run[i] + before + lanes_below(bal[i])] = (int32_t)r;
            }
            run[i] += all;
        }
        __syncthreads();
    }
}

// Routed training: the backward of k_gs_mark's gate_used with the selection
// held constant (include/radnerf.h rn_gate_select_bw).  Lane per ray, the
// row's gates, live bits and incoming gradients in registers; every load of
// the row comes before its first store, so d_used and d_gate may be one buffer.
__global__ void __launch_bounds__(GS_THREADS)
k_gs_bw(const float* __restrict__ gate, const uint8_t* __restrict__ live, const float* d_used,
        int64_t n, int K, int renorm, float* d_gate) {
    const int64_t r = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x;
    if (r >= n) return;
    float g[GS_MAX_K], d[GS_MAX_K];
    uint32_t lv = 0;
#pragma unroll
    for (int i = 0; i < GS_MAX_K; ++i) {
        const bool in = i < K;
        g[i] = in ? gate[r * K + i] : 0.f;
        d[i] = in ? d_used[r * K + i] : 0.f;
        lv |= (in && live[r * K + i] != 0 ? 1u : 0u) << i;
    }
    // S as k_gs_mark forms it; D = sum over live j of d_j u_j, u_j = g_j / S
    float S = 0.f, D = 0.f;
#pragma unroll
    for (int i = 0; i < GS_MAX_K; ++i)
        if ((lv >> i) & 1u) S = S + g[i];
    if (renorm) {
#pragma unroll
        for (int i = 0; i < GS_MAX_K; ++i)
            if ((lv >> i) & 1u) D = D + d[i] * (g[i] / S);
    }
#pragma unroll
    for (int i = 0; i < GS_MAX_K; ++i) {
        if (i < K) {
            float o = 0.f;
            if ((lv >> i) & 1u) o = renorm ? (S == 0.f ? 0.f : (d[i] - D) / S) : d[i];
            d_gate[r * K + i] = o;
        }
    }
}

}  // namespace

extern "C" {

int rn_gate_select_bw(const float* gate, const uint8_t* live, const float* dL_dgate_used,
                      int64_t n_rays, int32_t n_models, int32_t renormalize, float* dL_dgate,
                      void* stream) {
    RN_CHECK_ARG(n_rays >= 0 && n_rays < (1ll << 31) && n_models >= 1 && n_models <= GS_MAX_K,
                 "bad sizes (1 <= n_models <= 16)");
    if (n_rays == 0) return 0;
    RN_CHECK_ARG(gate && live && dL_dgate_used && dL_dgate, "null pointer");
    k_gs_bw<<<nblk(n_rays, GS_THREADS), GS_THREADS, 0, (hipStream_t)stream>>>(
        gate, live, dL_dgate_used, n_rays, n_models, renormalize != 0, dL_dgate);
    RN_CHECK_LAUNCH();
    return 0;
}


int rn_gate_select(const float* gate, int64_t n_rays, int32_t n_models, float gate_min,
                   int32_t gate_topk, int32_t renormalize, uint8_t* live, float* gate_used,
                   int32_t* list, int32_t* count, float* opacity_k, float* depth_k, float* rgb_k,
                   int32_t* n_samples, void* work, void* stream) {
    RN_CHECK_ARG(n_rays >= 0 && n_rays < (1ll << 31) && n_models >= 1 && n_models <= GS_MAX_K,
                 "bad sizes (1 <= n_models <= 16)");
    RN_CHECK_ARG(gate_min >= 0.0f && gate_min < 1.0f, "gate_min must be in [0, 1)");
    RN_CHECK_ARG(gate_topk >= 1 && gate_topk <= n_models, "gate_topk must be in [1, n_models]");
    RN_CHECK_ARG(count, "null pointer");
    const bool outs = opacity_k || depth_k || rgb_k || n_samples;
    RN_CHECK_ARG(!outs || (opacity_k && depth_k && rgb_k && n_samples),
                 "opacity_k, depth_k, rgb_k and n_samples go together (all or none)");
    hipStream_t st = (hipStream_t)stream;
    if (n_rays == 0) {
        RN_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * n_models, st), "count memset");
        return 0;
    }
    RN_CHECK_ARG(gate && live && gate_used && list && work, "null pointer");
    SelectArgs a{};
    a.gate = gate; a.n = (int)n_rays; a.K = n_models;
    const int steps = nblk(n_rays, GS_THREADS);
    a.span = nblk(steps, GS_MAX_BLOCKS) * GS_THREADS;
    const int blocks = nblk(n_rays, a.span);              // <= GS_MAX_BLOCKS
    a.gate_min = gate_min; a.topk = gate_topk; a.renorm = renormalize != 0;
    a.live = live; a.gate_used = gate_used;
    a.opacity = opacity_k; a.depth = depth_k; a.rgb = rgb_k; a.n_samples = n_samples;
    a.list = list; a.count = count; a.work = (int32_t*)work;
    k_gs_mark<<<blocks, GS_THREADS, 0, st>>>(a);
    k_gs_scan<<<n_models, GS_THREADS, 0, st>>>(a.work, blocks, count);
    k_gs_write<<<blocks, GS_THREADS, 0, st>>>(a);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
