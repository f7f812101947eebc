// The fused field's plan for gfx950: the merged (ray, t) order of the K
// sub-NeRFs' samples and the chunk schedule of whole rays that the merged
// forward and backward (field_fwd_merged.hip; k_field_bwd_merged, field.hip) work
// through.  The reference has no counterpart (it runs one model at a time,
// models/networks.py:300-328); the plan changes the order of work, not a value.
//
// Work decomposition: one wave per ray merges the ray's K runs of t in LDS
// (merge path; K > 2: a pairwise merge tree); one thread per chunk then
// finds the chunk's rays by binary search and writes its descriptor (rn_merge.h).
//
// Kernels: k_bwd_plan (K <= 2), k_bwd_plan_multi (K > 2), k_bwd_chunks.
// Entry: rn_bwd_plan.
#include "rn_field.h"
#include "rn_merge.h"
#pragma clang fp contract(off)

namespace {

// Merged order of the K models' samples per ray (ray-major, then t, ties by
// model): perm[mstart[r] + rank] = sample.  One wave per ray; each sample's
// rank = its index in its (model, ray) run + the samples of the other models
// of the ray that precede it (binary search; t increases along a run).  The
// ray's K runs are staged in the wave's LDS slice when they fit (always for
// K = 2), so the searches are LDS reads instead of dependent global loads.
#define PLAN_WAVES 4
#define PLAN_LDS 2048      // floats per wave

// Stage one ray's K runs of t (and, with ids, each sample's position in the
// concatenation) into the wave's LDS slice: position i of the concatenated
// runs [bnd[k], bnd[k+1]) is sample off[k] + i - bnd[k].  Positions are dealt
// over the lanes with PLAN_UNR loads in flight per lane (a loop per run, one
// load then its store, waited for each load: 16 round trips per ray at K = 8,
// and k_bwd_plan_multi took 0.139 ms at C5).  bnd / off are wave-uniform.
#define PLAN_UNR 8

// The level-partitioned forward's per-position input (k_enc_prep's float4:
// unit coordinates, sample id), written by the plan as it places each sample
// (rn_bwd_plan with `prep`): the plan has the sample's t in LDS and its ray,
// so the separate pass that re-read perm, ts and the ray (C3 0.03 ms) goes.
// Arithmetic as load_sample<1> + unit_coord (bit-identical).
struct PlanPrep {
    float4* prep;             // null: the plan writes perm only
    const float* rays_o; const float* rays_d;
    float mn[3], ext[3];
    // 1 / extent when every extent is a power of two (scale 0.5: 1, scale 16:
    // 32): x / ext and x * (1 / ext) are then the same float, and the three
    // IEEE divisions per sample leave the merge's serial chain; 0 otherwise
    float inv[3];
};
struct RayPos { float o[3], d[3]; };
__device__ __forceinline__ RayPos plan_ray(const PlanPrep& P, int r) {
    RayPos q;
#pragma unroll
    for (int c = 0; c < 3; ++c) { q.o[c] = P.rays_o[3 * r + c]; q.d[c] = P.rays_d[3 * r + c]; }
    return q;
}
__device__ __forceinline__ void plan_prep_write(const PlanPrep& P, const RayPos& q, int pos,
                                                float t, int s) {
    const float x = fmaf(t, q.d[0], q.o[0]), y = fmaf(t, q.d[1], q.o[1]), z = fmaf(t, q.d[2], q.o[2]);
    auto u = [&](float v, int c) {
        return P.inv[0] != 0.f ? fminf(fmaxf((v - P.mn[c]) * P.inv[c], 0.0f), 1.0f)
                               : unit_coord(v, P.mn[c], P.ext[c]);
    };
    P.prep[pos] = make_float4(u(x, 0), u(y, 1), u(z, 2), __int_as_float(s));
}

// Ray r's run of each model (count, first sample) and its merged start ms.
// r is wave-uniform (the wave id read back as a scalar), and every model's
// words load unconditionally (index clamped to K - 1, zeroed after): scalar
// loads issued together.  (With the wave id a vector value and each load
// under k < K, the 2K counts / offsets became vector loads waited for one by
// one: ~16 round trips per ray at K = 8.)
__device__ __forceinline__ void plan_ray_runs(int K, int B, int r, const int32_t* __restrict__ counts,
                                              const int32_t* __restrict__ offsets,
                                              const int32_t* __restrict__ seg_base, int* cnt,
                                              int* off, int& ms) {
    int c[MB_KMAX], o[MB_KMAX], sb[MB_KMAX];
#pragma unroll
    for (int k = 0; k < MB_KMAX; ++k) {
        const int kk = k < K ? k : K - 1;
        c[k] = counts[kk * B + r]; o[k] = offsets[kk * B + r]; sb[k] = seg_base[kk];
    }
    ms = 0;
#pragma unroll
    for (int k = 0; k < MB_KMAX; ++k) {
        cnt[k] = k < K ? c[k] : 0;
        off[k] = k < K ? o[k] : 0;
        ms += k < K ? o[k] - sb[k] : 0;
    }
}
__device__ __forceinline__ void plan_stage(int K, int tot_r, const int* bnd, const int* off,
                                           const float* __restrict__ ts, float* st, uint16_t* si) {
    const int lane = rn_lane();
    for (int i0 = 0; i0 < tot_r; i0 += RN_WAVE * PLAN_UNR) {
        float v[PLAN_UNR];
#pragma unroll
        for (int u = 0; u < PLAN_UNR; ++u) {
            const int i = i0 + u * RN_WAVE + lane;
            int base = off[0];                    // off[k] - bnd[k] of i's run (bnd[0] = 0)
#pragma unroll
            for (int kq = 1; kq < MB_KMAX; ++kq)
                base = (kq < K && i >= bnd[kq]) ? off[kq] - bnd[kq] : base;
            v[u] = i < tot_r ? ts[base + i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PLAN_UNR; ++u) {
            const int i = i0 + u * RN_WAVE + lane;
            if (i < tot_r) {
                st[i] = v[u];
                if (si) si[i] = (uint16_t)i;
            }
        }
    }
}

__global__ void __launch_bounds__(PLAN_WAVES * 64)
k_bwd_plan(int B, int K, const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
           const int32_t* __restrict__ seg_base, const int32_t* __restrict__ seg_count,
           const float* __restrict__ ts, int32_t* __restrict__ mstart, int32_t* __restrict__ perm,
           PlanPrep P) {
    __shared__ float sT[PLAN_WAVES][PLAN_LDS];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / RN_WAVE);
    const int r = blockIdx.x * PLAN_WAVES + wid;
    if (r >= B) return;                      // wave-uniform; no block barrier below
    const int lane = rn_lane();
    int ms = 0, tot_r = 0;
    int cnt[MB_KMAX], off[MB_KMAX], loc[MB_KMAX];
    plan_ray_runs(K, B, r, counts, offsets, seg_base, cnt, off, ms);
#pragma unroll
    for (int k = 0; k < MB_KMAX; ++k) { loc[k] = tot_r; tot_r += cnt[k]; }
    if (lane == 0) {
        mstart[r] = ms;
        if (r == 0) {
            int tot = 0;
            for (int k = 0; k < K; ++k) tot += seg_count[k];
            mstart[B] = tot;
        }
    }
    const bool staged = tot_r <= PLAN_LDS;
    float* st = sT[wid];
    const RayPos rq = P.prep ? plan_ray(P, r) : RayPos{};
    if (staged) {
        plan_stage(K, tot_r, loc, off, ts, st, nullptr);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (K == 2 && staged) {
        // merge path: lane j emits merged positions [j L, (j+1) L); it finds
        // how many of them come from model 0 by a binary search on its
        // diagonal (model 0 first on equal t, as below), then merges serially
        // -- ~log2(n) + L dependent LDS reads per lane instead of a search
        // per sample (C3: 0.064 -> 0.040 ms with k_bwd_chunks)
        const float* A = st + loc[0];
        const float* Bv = st + loc[1];
        const int nA = cnt[0], nB = cnt[1], n = nA + nB;
        const int L = (n + RN_WAVE - 1) / RN_WAVE;
        const int d = min(lane * L, n);
        int lo = max(0, d - nB), hi = min(d, nA);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (A[mid] <= Bv[d - 1 - mid]) lo = mid + 1; else hi = mid;
        }
        int a = lo, b = d - lo;
        const int e = min(d + L, n);
        for (int q = d; q < e; ++q) {
            const bool takeA = a < nA && (b >= nB || A[a] <= Bv[b]);
            const int smp = takeA ? off[0] + a : off[1] + b;
            perm[ms + q] = smp;
            if (P.prep) plan_prep_write(P, rq, ms + q, takeA ? A[a] : Bv[b], smp);
            a += takeA ? 1 : 0;
            b += takeA ? 0 : 1;
        }
        return;
    }
    for (int k = 0; k < K; ++k) {
        for (int i = lane; i < cnt[k]; i += RN_WAVE) {
            const float t = staged ? st[loc[k] + i] : ts[off[k] + i];
            int pos = i;
            for (int k2 = 0; k2 < K; ++k2) {
                if (k2 == k) continue;
                int lo = 0, hi = cnt[k2];        // count of t2 < t (k2 > k) or t2 <= t (k2 < k)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const float t2 = staged ? st[loc[k2] + mid] : ts[off[k2] + mid];
                    if (t2 < t || (k2 < k && t2 == t)) lo = mid + 1; else hi = mid;
                }
                pos += lo;
            }
            perm[ms + pos] = off[k] + i;
            if (P.prep) plan_prep_write(P, rq, ms + pos, t, off[k] + i);
        }
    }
}

// The same merged order for K > 2 by a merge tree in LDS: the ray's K runs
// (staged with their sample indices) are merged pairwise, log2(K) levels; each
// pair is merged by the whole wave with merge path (lane j: a diagonal binary
// search, then L serial steps).  Runs are merged in model order and the left
// run wins ties, so the result is ordered by (t, model) like k_bwd_plan's
// ranks.  ~log2(n) + n/64 dependent LDS reads per lane and level instead of
// (K-1) binary searches per sample (C5: K = 8, ~760 samples per ray).
#define PLANM_WAVES 2
#define PLANM_LDS 2048     // samples per wave

// Sample ids in LDS are u16 positions in the ray's staged runs (model k's run
// starts at kb[k]); the last level maps them to global sample indices
// (ko[k] + id - kb[k]).  u16 ids take a block to 48 KB of LDS: 3 blocks (6
// waves) per CU instead of 2, for a latency-bound merge.
__device__ __forceinline__ void merge_pair_wave(const float* tA, const uint16_t* iA, int nA,
                                                const float* tB, const uint16_t* iB, int nB,
                                                float* to, uint16_t* io, int32_t* gout,
                                                const int* kb, const int* ko, int K,
                                                const PlanPrep& P, const RayPos& rq, int gpos) {
    const int lane = rn_lane();
    const int n = nA + nB;
    const int L = (n + RN_WAVE - 1) / RN_WAVE;
    const int d = min(lane * L, n);
    int lo = max(0, d - nB), hi = min(d, nA);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tA[mid] <= tB[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int a = lo, b = d - lo;
    const int e = min(d + L, n);
    for (int q = d; q < e; ++q) {
        // both heads' t and ids read together (one LDS round trip per step;
        // as selects of the addresses, the compare, the id and the output t
        // were three).  a = nA / b = nB read one past their run, inside the
        // wave's slice, and are not used
        const float ta = tA[a], tb = tB[b];
        const int ja = iA[a], jb = iB[b];
        const bool takeA = a < nA && (b >= nB || ta <= tb);
        const int idx = takeA ? ja : jb;
        if (gout) {
            int base = ko[0];
#pragma unroll
            for (int j = 1; j < MB_KMAX; ++j)
                if (j < K && idx >= kb[j]) base = ko[j] - kb[j];
            gout[q] = base + idx;
            if (P.prep) plan_prep_write(P, rq, gpos + q, takeA ? ta : tb, base + idx);
        } else {
            to[q] = takeA ? ta : tb;
            io[q] = (uint16_t)idx;
        }
        a += takeA ? 1 : 0;
        b += takeA ? 0 : 1;
    }
}

__global__ void __launch_bounds__(PLANM_WAVES * 64)
k_bwd_plan_multi(int B, int K, const int32_t* __restrict__ counts,
                 const int32_t* __restrict__ offsets, const int32_t* __restrict__ seg_base,
                 const int32_t* __restrict__ seg_count, const float* __restrict__ ts,
                 int32_t* __restrict__ mstart, int32_t* __restrict__ perm, PlanPrep P) {
    // (+2: a merge step reads one past the last run)
    __shared__ float sT[PLANM_WAVES][2][PLANM_LDS + 2];
    __shared__ uint16_t sI[PLANM_WAVES][2][PLANM_LDS + 2];
    static_assert(PLANM_LDS <= 65536, "u16 sample ids");
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / RN_WAVE);
    const int r = blockIdx.x * PLANM_WAVES + wid;
    if (r >= B) return;                      // wave-uniform; no block barrier below
    const int lane = rn_lane();
    int ms = 0, tot_r = 0;
    int bnd[MB_KMAX + 1], off[MB_KMAX], cnt[MB_KMAX];
    plan_ray_runs(K, B, r, counts, offsets, seg_base, cnt, off, ms);
#pragma unroll
    for (int k = 0; k < MB_KMAX; ++k) { bnd[k] = tot_r; tot_r += cnt[k]; }
    bnd[MB_KMAX] = tot_r;
    const RayPos rq = P.prep ? plan_ray(P, r) : RayPos{};
    if (lane == 0) {
        mstart[r] = ms;
        if (r == 0) {
            int tot = 0;
            for (int k = 0; k < K; ++k) tot += seg_count[k];
            mstart[B] = tot;
        }
    }
    if (tot_r > PLANM_LDS) {
        // (rays longer than the LDS slice: rank by binary searches in global memory)
        for (int k = 0; k < K; ++k) {
            const int ck = bnd[k + 1] - bnd[k];
            for (int i = lane; i < ck; i += RN_WAVE) {
                const float t = ts[off[k] + i];
                int pos = i;
                for (int k2 = 0; k2 < K; ++k2) {
                    if (k2 == k) continue;
                    int lo = 0, hi = bnd[k2 + 1] - bnd[k2];
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        const float t2 = ts[off[k2] + mid];
                        if (t2 < t || (k2 < k && t2 == t)) lo = mid + 1; else hi = mid;
                    }
                    pos += lo;
                }
                perm[ms + pos] = off[k] + i;
                if (P.prep) plan_prep_write(P, rq, ms + pos, t, off[k] + i);
            }
        }
        return;
    }
    int cur = 0;
    int kb[MB_KMAX];                          // the models' runs (bnd is merged below)
#pragma unroll
    for (int k = 0; k < MB_KMAX; ++k) kb[k] = k < K ? bnd[k] : 0;
    plan_stage(K, tot_r, bnd, off, ts, sT[wid][0], sI[wid][0]);
    int nr = K;
    while (true) {
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const bool last = nr <= 2;
        const float* ts_ = sT[wid][cur];
        const uint16_t* is_ = sI[wid][cur];
        for (int p = 0; 2 * p < nr; ++p) {
            const int a0 = bnd[2 * p], a1 = bnd[min(2 * p + 1, nr)], b1 = bnd[min(2 * p + 2, nr)];
            merge_pair_wave(ts_ + a0, is_ + a0, a1 - a0, ts_ + a1, is_ + a1, b1 - a1,
                            sT[wid][cur ^ 1] + a0, sI[wid][cur ^ 1] + a0,
                            nullptr, kb, off, K, P, rq, ms + a0);
        }
        if (last) {
            // the merged order is in LDS like every level's: perm (and the
            // level forward's input) go out in position order, coalesced and
            // off the merge's serial chain (written from inside it, each
            // lane's stores were L positions apart)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const float* to = sT[wid][cur ^ 1];
            const uint16_t* io = sI[wid][cur ^ 1];
            for (int q = lane; q < tot_r; q += RN_WAVE) {
                const int idx = io[q];
                int base = off[0];
#pragma unroll
                for (int jk = 1; jk < MB_KMAX; ++jk)
                    if (jk < K && idx >= kb[jk]) base = off[jk] - kb[jk];
                perm[ms + q] = base + idx;
                if (P.prep) plan_prep_write(P, rq, ms + q, to[q], base + idx);
            }
            return;
        }
        // runs after this level: boundaries of the merged pairs
        const int nn = (nr + 1) / 2;
        for (int p = 0; p < nn; ++p) bnd[p] = bnd[2 * p];
        bnd[nn] = bnd[nr];
        nr = nn;
        cur ^= 1;
    }
}

// Chunk schedule of the merged backward over the merged positions [0, total):
// big chunks for the first 15/16 of the work, then chunks of min_chunk (a short
// tail: blocks finish together).  With `blocks` > 0 the big chunks are a
// multiple of the persistent blocks in number, each <= max_chunk positions
// (size ceil(main / (blocks m)), m = ceil(main / (blocks max_chunk))): every
// block takes m of them.  A count just past a multiple (C4 at 2560: 534 big
// chunks for 256 blocks) left a few blocks one big chunk behind the rest, a
// tail the min_chunk phase was too small to hide (C4 485 vs 523 M samples/s
// at 2560 vs 3072).  Chunk c holds the rays whose merged start lies in
// [bound(c), bound(c+1)), so it is whole rays of at most max_chunk + K *
// max_samples samples (possibly none).
struct ChunkPlan {
    int head_n, head, max_chunk, min_chunk, c1, n;
    // first merged position of head chunk c (c <= head_n): head chunk c holds
    // ~head (c + 1) / head_n positions, a ramp from ~0 to head
    __host__ __device__ int hbound(int c) const {
        return head_n > 0 ? (int)(((int64_t)head * c * (c + 1)) / (2 * (int64_t)head_n)) : 0;
    }
    __host__ __device__ int bound(int c) const {
        const int H = hbound(head_n);
        if (c < head_n) return hbound(c);
        if (c <= c1) return H + (c - head_n) * max_chunk;
        return H + (c1 - head_n) * max_chunk + (c - c1) * min_chunk;
    }
};

// head_n chunks ramping from ~0 to `head` samples first (one per block): the
// blocks' first MLP phases end at staggered times, so the walks' requests
// reach the memory-side atomic units spread out instead of all at once after
// one full chunk's MLP phase, and the blocks stay out of phase after.  A ramp
// to max_chunk: C3 1183.4 -> 1189.2 M samples/s (field_bwd 2.995 -> 2.973
// ms), C2 853.7 -> 862.3; head chunks of one size (rounds 2 and 5) changed
// nothing, and at scale 16 a ramp to max_chunk / 2 lost 2-5 % (the big chunks,
// only ~2 per block there, get shorter); profiles/r06/headramp/.  Then
// max_chunk up to 15/16 of the work, then min_chunk (round 6: a tail of 1/16
// instead of 1/8, with its chunks sized by shape on the host: C3 1191 -> 1194,
// C4 653 -> 658, C5 789 -> 791; no tail at all lost 1 %; profiles/r06/tail/)
__host__ __device__ __forceinline__ ChunkPlan chunk_plan(int total, int head_n, int head,
                                                         int max_chunk, int min_chunk, int blocks) {
    ChunkPlan p;
    p.head = head; p.max_chunk = max_chunk; p.min_chunk = min_chunk;
#ifndef RN_TAIL_SHIFT              // (timing studies: -D overrides the tail's share, 2^-shift)
#define RN_TAIL_SHIFT 4
#endif
    // the cap_chunks bound of include/radnerf.h (total / (8 min_chunk) tail chunks) and
    // Workspace.chunk_list assume a tail of at most 1/8 of the work
    static_assert(RN_TAIL_SHIFT >= 3, "the documented cap_chunks bound assumes a tail <= 1/8");
    const int main_end = total - (RN_TAIL_SHIFT < 31 ? total >> RN_TAIL_SHIFT : 0);
    // the ramp takes ~head (head_n + 1) / 2 positions: none if that is past the main part
    p.head_n = head > 0 && (int64_t)head * (head_n + 1) / 2 <= main_end ? head_n : 0;
    const int H = p.hbound(p.head_n);
    if (blocks > 0 && main_end > H) {
        const int64_t main = main_end - H, per = (int64_t)blocks * max_chunk;
        const int64_t m = (main + per - 1) / per;
        const int64_t sz = (main + (int64_t)blocks * m - 1) / ((int64_t)blocks * m);
        p.max_chunk = (int)(sz < min_chunk ? min_chunk : (sz > max_chunk ? max_chunk : sz));
    }
    p.c1 = p.head_n + (main_end > H ? (main_end - H) / p.max_chunk : 0);
    const int rest = total - p.bound(p.c1);
    p.n = p.c1 + (rest > 0 ? (rest + min_chunk - 1) / min_chunk : 0);
    return p;
}

__global__ void __launch_bounds__(256)
k_bwd_chunks(int B, int K, const int32_t* __restrict__ mstart,
             const int32_t* __restrict__ offsets, const int32_t* __restrict__ seg_base,
             const int32_t* __restrict__ seg_count, int head_n, int head, int max_chunk,
             int min_chunk, int blocks, int cap_chunks, int32_t* __restrict__ chunk_first,
             int32_t* __restrict__ desc, int32_t* __restrict__ queue) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = mstart[B];
    const ChunkPlan p = chunk_plan(total, head_n, head, max_chunk, min_chunk, blocks);
    const int n = min(p.n, cap_chunks);
    if (c == 0) { queue[0] = 0; queue[1] = n; queue[2] = 0; }
    if (c > n) return;
    // first ray with mstart >= bound(cc); the complete schedule ends at B (the
    // rays without samples after the last sample belong to its last chunk).
    // A schedule cut short by cap_chunks (n < p.n) ends where chunk n would
    // have begun: its last chunk is the full schedule's, not the rest of the
    // rays (which would outgrow the scratch rows of rn_field_bwd_merged)
    auto first_ray = [&](int cc) {
        if (cc == p.n) return B;
        const int bound = p.bound(cc);
        int lo = 0, hi = B;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (mstart[mid] < bound) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    if (c == n) { chunk_first[c] = first_ray(c); return; }
    const int first[2] = {first_ray(c), first_ray(c + 1)};
    chunk_first[c] = first[0];
    // descriptor: the chunk's sample range per model (the blocks read it with
    // one 80-B load per ticket)
    int32_t* d = desc + (size_t)c * CH_DESC;
    const int r0 = first[0], r1 = first[1];
    d[CH_R0] = r0; d[CH_R1] = r1; d[2] = 0; d[3] = 0;
    for (int k = 0; k < MB_KMAX; ++k) {
        int a0 = 0, cnt = 0;
        if (k < K && r0 < B) {
            a0 = offsets[k * B + r0];
            const int a1 = r1 < B ? offsets[k * B + r1] : seg_base[k] + seg_count[k];
            cnt = a1 - a0;
        }
        d[ch_first(k)] = a0; d[ch_count(k)] = cnt;
    }
}

}  // namespace

extern "C" {

int rn_bwd_plan(const int32_t* counts, const int32_t* offsets, const int32_t* seg_base,
                const int32_t* seg_count, const float* ts, int64_t n_rays, int32_t n_models,
                int32_t head_chunks, int32_t head_size, int32_t max_chunk, int32_t min_chunk,
                int32_t balance_blocks, int32_t cap_chunks, int32_t* mstart, int32_t* perm,
                int32_t* chunk_first, int32_t* chunk_desc, int32_t* queue, const float* rays_o,
                const float* rays_d, const float* xyz_min, const float* extent, float* prep,
                void* stream) {
    RN_CHECK_ARG(n_rays >= 1 && n_models >= 1 && n_models <= MB_KMAX, "bad sizes");
    RN_CHECK_ARG(max_chunk >= min_chunk && min_chunk >= 1 && cap_chunks >= 1 && head_chunks >= 0 &&
                 head_size >= 0 && head_size <= max_chunk && balance_blocks >= 0,
                 "bad chunk sizes");
    RN_CHECK_ARG(counts && offsets && seg_base && seg_count && ts && mstart && perm &&
                 chunk_first && chunk_desc && queue, "null pointer");
    RN_CHECK_ARG(!prep || (rays_o && rays_d && xyz_min && extent), "null pointer (prep)");
    PlanPrep P{};
    P.prep = (float4*)prep; P.rays_o = rays_o; P.rays_d = rays_d;
    if (prep) {
        bool pow2 = true;
        for (int c = 0; c < 3; ++c) {
            P.mn[c] = xyz_min[c]; P.ext[c] = extent[c];
            int e;
            pow2 = pow2 && extent[c] > 0.f && std::frexp(extent[c], &e) == 0.5f &&
                   e > -120 && e < 120;
        }
        for (int c = 0; c < 3; ++c) P.inv[c] = pow2 ? 1.0f / extent[c] : 0.f;
    }
    if (n_models > 2)
        k_bwd_plan_multi<<<nblk(n_rays, PLANM_WAVES), PLANM_WAVES * 64, 0, (hipStream_t)stream>>>(
            (int)n_rays, n_models, counts, offsets, seg_base, seg_count, ts, mstart, perm, P);
    else
        k_bwd_plan<<<nblk(n_rays, PLAN_WAVES), PLAN_WAVES * 64, 0, (hipStream_t)stream>>>(
            (int)n_rays, n_models, counts, offsets, seg_base, seg_count, ts, mstart, perm, P);
    RN_CHECK_LAUNCH();
    k_bwd_chunks<<<nblk(cap_chunks + 1, 256), 256, 0, (hipStream_t)stream>>>(
        (int)n_rays, n_models, mstart, offsets, seg_base, seg_count, head_chunks, head_size,
        max_chunk, min_chunk, balance_blocks, cap_chunks, chunk_first, chunk_desc, queue);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
