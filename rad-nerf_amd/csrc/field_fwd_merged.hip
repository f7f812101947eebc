// Merged forwards of the fused Rad-NeRF field for gfx950: the K sub-NeRFs
// evaluated together over the plan's merged (ray, t) order (field_plan.hip),
// so that samples of different models on one ray share their hash-grid lines.
//
// Reference (behaviour): models/networks.py:291-328 (MNGP.density/forward),
// :229-289 (tcnn Grid/Hash encoding, SH degree 4, FullyFusedMLP), custom_functions.py
// :162-173 (TruncExp); restated in DESIGN.md §2.  Per-sample arithmetic is that
// of k_field_fwd (field.hip): one wave = 32 samples, the lane map of rn_field.h.
//
// Kernels:
//  * k_field_fwd_merged: blocks take the plan's chunks from a ticket queue and
//    interleave the K models' tiles of a chunk on one CU.
//  * k_enc_prep + k_field_encode_levels + k_field_mlp_planes: the
//    level-partitioned forward (the encoding split by level over the XCDs,
//    then the MLP tiles), static splits.
// Entries: rn_field_fwd_merged, rn_field_fwd_levels, rn_set_level_pairing.
#include "rn_field.h"
#include "rn_merge.h"
#pragma clang fp contract(off)

static uint64_t g_level_pairing = 0;     // rn_field_fwd_levels' level groups (0 = default)

namespace {

// ---------------------------------------------------------------------------
// Merged forward: blocks take the plan's chunks (whole rays) and evaluate the
// K models' tiles of a chunk interleaved (tile i of model 0, tile i of model
// 1, ...), so the models' samples of the same rays are gathered close in time
// by the same CU: the second model's corners hit L1/L2 lines the first one
// fetched (the fine levels otherwise miss L2 for every sample).  With
// K <= FM_LDS_K the K models' forward fragments sit in LDS (dynamic, K x
// 24 KB); with more (GW), the MLP tiles read them from global memory (L2).
// Same outputs as k_field_fwd (per-sample arithmetic is identical).
// ---------------------------------------------------------------------------
#define FM_KMAX 8
#define FM_LDS_K 4
// (the chunk descriptor, rn_merge.h, is laid out for MB_KMAX models)
static_assert(FM_KMAX == MB_KMAX, "k_field_fwd_merged reads the plan's descriptors");

template <int CACHE, bool ENC_M, bool GW>
__global__ void __launch_bounds__(1024)
k_field_fwd_merged(FieldArgs a, MergeArgs m) {
    extern __shared__ __attribute__((aligned(16))) rn_half sWm[];   // [K][24 frags]
    __shared__ LvTab sT;
    __shared__ int32_t sCh[2][2 + 2 * FM_KMAX];      // this and the previous chunk
    const int K = m.n_models, B = m.n_rays;
    if (!GW) {
        for (int k = 0; k < K; ++k)
            rn_block_copy16(sWm + (size_t)k * FIELD_FWD_FRAGS * RN_FRAG_HALFS,
                            a.frags + (size_t)k * FIELD_FRAGS * RN_FRAG_HALFS,
                            FIELD_FWD_FRAGS * RN_FRAG_BYTES);
    }
    lv_stage(sT, a.gm);
    const int waves = blockDim.x / RN_WAVE;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / RN_WAVE);
    const int lane = rn_lane(), c = lane & 31, h = lane >> 5;
    int ticket = 0, n_chunks = 0;
    if (threadIdx.x == 0) { n_chunks = m.queue[1]; ticket = atomicAdd(m.queue + 2, 1); }

    // per-model MLP tile u of chunk descriptor ch (tile i of model 0, tile i
    // of model 1, ...); false: past the end
    auto mlp_tile = [&](const int32_t* ch, int u) {
        const int k = u % K, t = u / K;
        const int n_k = ch[2 + FM_KMAX + k];
        if (t * 32 >= n_k) return;                           // wave-uniform
        rn_lds_order();
        const int i = t * 32 + c;
        const bool valid = i < n_k;
        const int64_t s = ch[2 + k] + (valid ? i : 0);
        FwdState st;
        float ux, uy, uz;
        constexpr int TC = ENC_M ? CACHE_READ_NT : CACHE;
        const rn_half* W = GW ? a.frags + (size_t)k * FIELD_FRAGS * RN_FRAG_HALFS
                              : sWm + (size_t)k * FIELD_FWD_FRAGS * RN_FRAG_HALFS;
        tile_forward_s<1, TC>(a, sT, W, s, valid, TC != CACHE_NONE ? cache_slot(a, s) : nullptr,
                              st, ux, uy, uz);
        if (valid && h == 0) {
            a.sigma[s] = expf(st.g0);
            a.rgb[3 * s + 0] = sigmoidf(st.out[0]);
            a.rgb[3 * s + 1] = sigmoidf(st.out[1]);
            a.rgb[3 * s + 2] = sigmoidf(st.out[2]);
        }
    };
    auto mlp_tiles = [&](const int32_t* ch) {
        int max_t = 0;
        for (int k = 0; k < K; ++k) max_t = max(max_t, (ch[2 + FM_KMAX + k] + 31) >> 5);
        return max_t * K;
    };

    bool prev_live = false;
    for (int it = 0;; ++it) {
        int32_t* cur = sCh[it & 1];
        const int32_t* prev = sCh[(it & 1) ^ 1];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int ch = ticket;
            ticket = atomicAdd(m.queue + 2, 1);           // the next chunk's, ahead
            int4 d[CH_DESC / 4];
            if (ch < n_chunks) {
#pragma unroll
                for (int q = 0; q < CH_DESC / 4; ++q)
                    d[q] = reinterpret_cast<const int4*>(m.desc + (size_t)ch * CH_DESC)[q];
            }
            const int32_t* di = reinterpret_cast<const int32_t*>(d);
            cur[0] = ch < n_chunks ? di[CH_R0] : B;
            cur[1] = ch < n_chunks ? di[CH_R1] : B;
            for (int k = 0; k < K; ++k) {
                cur[2 + k] = di[ch_first(k)];
                cur[2 + FM_KMAX + k] = ch < n_chunks ? di[ch_count(k)] : 0;
            }
        }
        __syncthreads();
        const bool live = cur[0] < B;
        if (!ENC_M) {
            if (!live) break;
            const int nt = mlp_tiles(cur);
            for (int u = wid; u < nt; u += waves) mlp_tile(cur, u);
            continue;
        }
        // Merged-order encoding, software-pipelined over chunks: iteration it
        // encodes chunk it in merged (ray, t, model) order into the encoding
        // cache -- a tile mixes the sub-NeRFs of one ray stretch, so its
        // corners share more lines (tools/fwd_lines_sim.py: 20.9 vs 28.2 lines
        // per sample) -- and runs the per-model MLP tiles of chunk it - 1,
        // whose encodings the barrier above published; one work list, no
        // barrier between the two kinds of tile.
        if (!live && !prev_live) break;
        int p_base = 0, n_p = 0;
        if (live) { p_base = m.mstart[cur[0]]; n_p = m.mstart[cur[1]] - p_base; }
        const int nA = (n_p + 31) >> 5;
        const int nB = prev_live ? mlp_tiles(prev) : 0;
        for (int u = wid; u < nA + nB; u += waves) {
            if (u >= nA) { mlp_tile(prev, u - nA); continue; }
            const int q = u * 32 + c;
            const bool valid = q < n_p;
            const int64_t s = m.perm[p_base + (valid ? q : 0)];
            float x, y, z, dx, dy, dz;
            load_sample<1>(a, s, x, y, z, dx, dy, dz);
            const float ux = unit_coord(x, a.xyz_min[0], a.extent[0]);
            const float uy = unit_coord(y, a.xyz_min[1], a.extent[1]);
            const float uz = unit_coord(z, a.xyz_min[2], a.extent[2]);
            half8 e0, e1;
            encode_lane(a, sT, rn_rsrc(a.grid, a.grid_bytes), h, ux, uy, uz, valid, e0, e1);
            if (valid) { half8* fc = cache_slot(a, s); fc[0] = e0; fc[1] = e1; }
        }
        prev_live = live;
    }
}


// ---------------------------------------------------------------------------
// Level-partitioned forward (round 3, after a probe: tools/enc_probe.py).
// The merged forward gathers all sixteen levels of a sample on one CU, so
// every XCD's 4 MB L2 faces the whole 23 MB table and the fine levels miss
// it for nearly every sample (27 fabric requests per sample at C5).  Here
// the encoding is split by level instead:
//   1. k_enc_prep: per merged position p the sample's unit coordinates and
//      index (16 B), computed once (bit-identical to load_sample<1>);
//   2. k_field_encode_levels: block b encodes levels g and 15 - g, g = b % 8,
//      for every sample (one level after the other).  Workgroups are dispatched to the XCDs round-robin
//      (a rotation that varies by dispatch: measured, group g ran on XCD
//      g - 1 for all its blocks), so each XCD gathers from two levels' tables
//      only; correctness does not depend on the mapping.  Output: one f16x2
//      plane per level, planes[L][s] (bit-identical to encode_lane);
//   3. k_field_mlp_planes: the MLP tiles per model read the 8 levels of each
//      lane from the planes, write sigma / rgb and the encoding cache (tile
//      layout) that the backward and the input-gradient kernels read.
// Static splits, no ticket queues (a per-XCD ticket word serialised at
// ~100 ns per ticket: 1.9 ms at C3).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_enc_prep(FieldArgs a, MergeArgs m, float4* __restrict__ prep) {
    const int P = m.mstart[m.n_rays];
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int s = m.perm[p];
        float x, y, z, dx, dy, dz;
        load_sample<1>(a, s, x, y, z, dx, dy, dz);
        prep[p] = make_float4(unit_coord(x, a.xyz_min[0], a.extent[0]),
                              unit_coord(y, a.xyz_min[1], a.extent[1]),
                              unit_coord(z, a.xyz_min[2], a.extent[2]), __int_as_float(s));
    }
}

__global__ void __launch_bounds__(256)
k_field_encode_levels(FieldArgs a, MergeArgs m, const float4* __restrict__ prep,
                      int32_t* __restrict__ xq, uint64_t pairing) {
    __shared__ LvTab sT;
    lv_stage(sT, a.gm);
    __syncthreads();
    const int g = blockIdx.x & 7;
    if (xq && threadIdx.x == 0) {           // probe: group g's blocks per XCD, its span
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        atomicAdd(xq + 8 * g + (int)(xcc & 7u), 1);
        atomicMin(reinterpret_cast<unsigned long long*>(xq + 64) + g,
                  (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
    // group g's levels: byte g of `pairing` (low nibble la, high lb)
    const int la = (int)((pairing >> (8 * g)) & 15u), lb = (int)((pairing >> (8 * g + 4)) & 15u);
    const int P = m.mstart[m.n_rays];
    const int nt = (P + 31) >> 5;
    const int nb = (int)(gridDim.x >> 3), j = (int)(blockIdx.x >> 3);
    const int t0 = (int)((int64_t)nt * j / nb), t1 = (int)((int64_t)nt * (j + 1) / nb);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), waves = blockDim.x >> 6;
    const int lane = rn_lane(), c = lane & 31, h = lane >> 5;
    const __amdgpu_buffer_rsrc_t rs = rn_rsrc(a.grid, a.grid_bytes);
    const LvConst LA = lv_const_uniform(sT, a.gm, la), LB = lv_const_uniform(sT, a.gm, lb);
    // level la over the block's tiles, then level lb: the XCD's blocks run in
    // step, so its L2 holds one level's table at a time (two hashed levels at
    // once, 4 MB, filled the whole L2).  A wave takes two tiles per pass.
#pragma unroll 1
    for (int ph = 0; ph < 2; ++ph) {
        const LvConst& LC = ph ? LB : LA;
        uint32_t* const out = const_cast<uint32_t*>(a.planes) + (size_t)(ph ? lb : la) * a.plane_stride;
        for (int t = t0 + 2 * wid; t < t1; t += 2 * waves) {
            const bool v0 = t * 32 + c < P;
            const bool v1 = t + 1 < t1 && (t + 1) * 32 + c < P;
            const bool valid = h ? v1 : v0;
            const int p = (t + h) * 32 + c;
            const float4 q = prep[valid ? p : 0];
            const uint32_t v = encode_tiles(a, rs, h, LC, q.x, q.y, q.z, v0, v1);
            if (valid) __builtin_nontemporal_store(v, out + __float_as_int(q.w));
        }
    }
    if (xq) {
        __syncthreads();
        if (threadIdx.x == 0)
            atomicMax(reinterpret_cast<unsigned long long*>(xq + 80) + g,
                      (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
}

// MLP tiles of the K models (tile u of the flat list: model k's 32 samples
// from seg_base[k] + 32 t).  Block b takes a contiguous range of the list,
// which spans one or two models at the bench sizes; their forward fragments
// are staged in LDS, FM_LDS_K models at a time.
__global__ void __launch_bounds__(1024)
k_field_mlp_planes(FieldArgs a, int K) {
    extern __shared__ __attribute__((aligned(16))) rn_half sWm[];   // [<= FM_LDS_K][24 frags]
    __shared__ LvTab sT;
    // the K segments (first sample, count), read once: per tile they were a
    // global round trip ahead of the tile's dependent loads
    __shared__ int32_t sSeg[2][FM_KMAX];
    lv_stage(sT, a.gm);
    if (threadIdx.x < K) {
        sSeg[0][threadIdx.x] = a.seg_base[threadIdx.x];
        sSeg[1][threadIdx.x] = a.seg_count[threadIdx.x];
    }
    int first[FM_KMAX + 1];
    first[0] = 0;
    for (int k = 0; k < K; ++k)
        first[k + 1] = first[k] + ((__builtin_amdgcn_readfirstlane(a.seg_count[k]) + 31) >> 5);
    const int T = first[K];
    const int u0 = (int)((int64_t)T * blockIdx.x / gridDim.x);
    const int u1 = (int)((int64_t)T * (blockIdx.x + 1) / gridDim.x);
    if (u0 >= u1) return;                                   // block-uniform
    int k_lo = 0, k_hi = 0;
    for (int k = 0; k < K; ++k) {
        if (first[k + 1] <= u0) k_lo = k + 1;
        if (first[k] < u1) k_hi = k;
    }
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), waves = blockDim.x >> 6;
    const int lane = rn_lane(), c = lane & 31, h = lane >> 5;
    for (int kb = k_lo; kb <= k_hi; kb += FM_LDS_K) {
        const int ke = min(k_hi, kb + FM_LDS_K - 1);
        __syncthreads();                                    // previous models' tiles done
        for (int k = kb; k <= ke; ++k)
            rn_block_copy16(sWm + (size_t)(k - kb) * FIELD_FWD_FRAGS * RN_FRAG_HALFS,
                            a.frags + (size_t)k * FIELD_FRAGS * RN_FRAG_HALFS,
                            FIELD_FWD_FRAGS * RN_FRAG_BYTES);
        __syncthreads();
        const int ua = max(u0, first[kb]), ub = min(u1, first[ke + 1]);
        for (int u = ua + wid; u < ub; u += waves) {
            int k = kb;
            while (k < ke && u >= first[k + 1]) ++k;
            const int t = u - first[k];
            const int n_k = sSeg[1][k];
            const int i = t * 32 + c;
            const bool valid = i < n_k;
            const int64_t s = sSeg[0][k] + (valid ? i : 0);
            FwdState st;
            float ux, uy, uz;
            rn_lds_order();
            tile_forward_s<1, CACHE_PLANES>(a, sT, sWm + (size_t)(k - kb) * FIELD_FWD_FRAGS * RN_FRAG_HALFS,
                                            s, valid, a.feat ? cache_slot(a, s) : nullptr, st,
                                            ux, uy, uz);
            if (valid && h == 0) {
                a.sigma[s] = expf(st.g0);
                a.rgb[3 * s + 0] = sigmoidf(st.out[0]);
                a.rgb[3 * s + 1] = sigmoidf(st.out[1]);
                a.rgb[3 * s + 2] = sigmoidf(st.out[2]);
            }
        }
    }
}

}  // namespace

extern "C" {

int rn_set_level_pairing(uint64_t pairing) {
    if (pairing != 0) {
        uint32_t seen = 0;
        for (int i = 0; i < 16; ++i) seen |= 1u << ((pairing >> (4 * i)) & 15u);
        RN_CHECK_ARG(seen == 0xffffu, "pairing: every level exactly once");
    }
    g_level_pairing = pairing;
    return 0;
}

int rn_field_fwd_merged(const float* ts, const int32_t* ray_of, const float* rays_o,
                        const float* rays_d, const int32_t* seg_base, const int32_t* seg_count,
                        const int32_t* chunk_desc, int32_t* queue,
                        int64_t n_rays, int32_t n_models, const void* grid_f16,
                        const uint32_t* level_offset, const uint32_t* level_hsize,
                        const uint32_t* level_res, const float* level_scale,
                        const float* xyz_min, const float* extent, const void* frags,
                        float* sigma, float* rgb, void* feat_cache, const int32_t* mstart,
                        const int32_t* perm, int32_t blocks, int32_t threads, void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1 && n_models <= FM_KMAX && blocks >= 1,
                 "bad sizes (n_models <= 8)");
    RN_CHECK_ARG(threads >= 64 && threads <= 1024 && threads % 64 == 0, "threads: 64..1024, waves");
    RN_CHECK_ARG(ts && ray_of && rays_o && rays_d && seg_base && seg_count &&
                 chunk_desc && queue && grid_f16 && level_offset && level_hsize && level_res &&
                 level_scale && xyz_min && extent && frags && sigma && rgb, "null pointer");
    RN_CHECK_ARG(!(mstart || perm) || (mstart && perm && feat_cache),
                 "merged-order encoding needs mstart, perm and the encoding cache");
    FieldArgs a{};
    field_args_grid(a, grid_f16, level_offset, level_hsize, level_res, level_scale, xyz_min, extent,
                    frags);
    field_args_compact(a, ts, ray_of, rays_o, rays_d, seg_base, seg_count);
    a.sigma = sigma; a.rgb = rgb; a.feat = (rn_half*)feat_cache;
    MergeArgs m{};
    m.desc = chunk_desc; m.queue = queue;
    m.mstart = mstart; m.perm = perm;
    m.n_rays = (int)n_rays; m.n_models = n_models;
    const bool gw = n_models > FM_LDS_K;
    const size_t lds = gw ? 0 : (size_t)n_models * FIELD_FWD_FRAGS * RN_FRAG_BYTES;
    hipStream_t st = (hipStream_t)stream;
    RN_CHECK_HIP(hipMemsetAsync(queue + 2, 0, sizeof(int32_t), st), "ticket reset");
#define RN_FM_LAUNCH(C, E)                                                                     \
    do {                                                                                       \
        if (gw) k_field_fwd_merged<C, E, true><<<blocks, threads, 0, st>>>(a, m);              \
        else k_field_fwd_merged<C, E, false><<<blocks, threads, lds, st>>>(a, m);              \
    } while (0)
    if (mstart) RN_FM_LAUNCH(CACHE_WRITE, true);
    else if (feat_cache) RN_FM_LAUNCH(CACHE_WRITE, false);
    else RN_FM_LAUNCH(CACHE_NONE, false);
#undef RN_FM_LAUNCH
    RN_CHECK_LAUNCH();
    return 0;
}

/* level-partitioned merged forward (k_enc_prep + k_field_encode_levels +
   k_field_mlp_planes): the same outputs and encoding cache as
   rn_field_fwd_merged with the merged-order encoding.  planes: 16 x
   plane_stride u32 (plane_stride >= every sample index + 1); prep: 16 B per
   merged sample; xq (optional probe): 96 int32, [8 g + x] += blocks of level
   group g that ran on XCD x, then u64 [32 + g] first start and [40 + g] last
   end of group g's blocks (s_memrealtime, 100 MHz). */
int rn_field_fwd_levels(const float* ts, const int32_t* ray_of, const float* rays_o,
                        const float* rays_d, const int32_t* seg_base, const int32_t* seg_count,
                        int64_t n_rays, int32_t n_models, const void* grid_f16,
                        const uint32_t* level_offset, const uint32_t* level_hsize,
                        const uint32_t* level_res, const float* level_scale,
                        const float* xyz_min, const float* extent, const void* frags,
                        float* sigma, float* rgb, void* feat_cache, const int32_t* mstart,
                        const int32_t* perm, uint32_t* planes, int64_t plane_stride, void* prep,
                        int32_t prep_ready, int32_t enc_blocks, int32_t mlp_blocks, int32_t* xq,
                        void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1 && n_models <= FM_KMAX && plane_stride >= 1,
                 "bad sizes (n_models <= 8)");
    RN_CHECK_ARG(enc_blocks >= 8 && enc_blocks % 8 == 0 && mlp_blocks >= 1,
                 "bad launch (enc_blocks: a multiple of 8)");
    RN_CHECK_ARG(ts && ray_of && rays_o && rays_d && seg_base && seg_count && grid_f16 &&
                 level_offset && level_hsize && level_res && level_scale && xyz_min && extent &&
                 frags && sigma && rgb && mstart && perm && planes && prep, "null pointer");
    FieldArgs a{};
    field_args_grid(a, grid_f16, level_offset, level_hsize, level_res, level_scale, xyz_min, extent,
                    frags);
    field_args_compact(a, ts, ray_of, rays_o, rays_d, seg_base, seg_count);
    a.sigma = sigma; a.rgb = rgb; a.feat = (rn_half*)feat_cache;
    a.planes = planes; a.plane_stride = plane_stride;
    MergeArgs m{};
    m.mstart = mstart; m.perm = perm; m.n_rays = (int)n_rays; m.n_models = n_models;
    hipStream_t st = (hipStream_t)stream;
    if (xq) {
        RN_CHECK_HIP(hipMemsetAsync(xq, 0, 64 * sizeof(int32_t), st), "probe reset");
        RN_CHECK_HIP(hipMemsetAsync(xq + 64, 0xff, 16 * sizeof(int32_t), st), "probe reset");
        RN_CHECK_HIP(hipMemsetAsync(xq + 80, 0, 16 * sizeof(int32_t), st), "probe reset");
    }
    // (prep_ready: rn_bwd_plan wrote the per-position input as it placed the samples)
    if (!prep_ready) k_enc_prep<<<1024, 256, 0, st>>>(a, m, (float4*)prep);
    // level groups: (g, 15 - g) unless a study set another pairing (each level
    // exactly once: checked on the host)
    uint64_t pairing = g_level_pairing;
    if (pairing == 0)
        for (int g = 0; g < 8; ++g) pairing |= (uint64_t)(g | ((RN_L - 1 - g) << 4)) << (8 * g);
    k_field_encode_levels<<<enc_blocks, 256, 0, st>>>(a, m, (const float4*)prep, xq, pairing);
    k_field_mlp_planes<<<mlp_blocks, 1024,
                         (size_t)min(n_models, FM_LDS_K) * FIELD_FWD_FRAGS * RN_FRAG_BYTES, st>>>(
        a, n_models);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
