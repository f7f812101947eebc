// Mesh clean-up for gfx950: the connected components of a triangle mesh and
// the compaction of the kept ones (radnerf_amd/mesh.py: components,
// filter_components).  The rules are stated in include/radnerf.h (rn_mesh_*)
// and restated in numpy by tests/mesh_clean_ref.py.
//  * Labelling: rounds of min-label hooking plus pointer jumping, one kernel
//    pair per round.  L[v] starts at v and only ever decreases, by atomicMin,
//    to the index of a vertex of v's own component.  The per-XCD L2s are not
//    coherent, so a plain load inside a kernel may return an older value of a
//    word: under the invariant an old value is still a vertex of the same
//    component and no lower than the truth, so a stale read costs a round,
//    never correctness.  No kernel loops on a value another workgroup writes:
//    every loop has a bound known at launch, nothing retries, nothing waits.
//    k_cc_check raises a flag unless every face has three equal labels and
//    L[L[v]] == L[v] everywhere; at that fixed point L[v] is the lowest index
//    of v's component.  The host launches rounds in batches and reads the flag
//    once per batch.
//  * Ids, counts, compaction: every order comes from an exclusive scan over
//    ballots (the scheme of mesh.hip's surface nets).  The atomics are integer
//    atomicMin / atomicAdd / atomicOr, whose results do not depend on order.
#include "rn_common.h"

#define MC_BLK 1024        // items per counting block: 16 wave chunks
#define MC_CHUNKS (MC_BLK / 64)
#define MC_HEAD 8          // int64 words at the front of the workspace

namespace {

enum { H_BAD = 0, H_OPEN = 1, H_ROOTS = 2, H_KEPT_V = 3, H_KEPT_F = 4 };

// A scan index over n flagged items, nb = ceil(n / 1024):
//   off  [nb + 1] int64  per block: flagged count -> rank of its first
//   bits [16 nb] u64     per 64-item chunk: the ballot of the flags
//   pre  [16 nb] u16     per chunk: flagged items of the block's earlier chunks
// 168 B per 1024 items.  The rank of a flagged item is three small reads.
struct ScanIdx {
    int64_t* off; uint64_t* bits; uint16_t* pre;
    uint32_t n, nb;
};

__device__ __forceinline__ uint64_t mc_below(int lane) { return (1ull << lane) - 1ull; }

__device__ __forceinline__ bool mc_flag(const ScanIdx& s, uint32_t i) {
    return (s.bits[i >> 6] >> (i & 63)) & 1;
}

__device__ __forceinline__ int64_t mc_rank(const ScanIdx& s, uint32_t i) {
    return s.off[i >> 10] + s.pre[i >> 6] + __popcll(s.bits[i >> 6] & mc_below(i & 63));
}

__device__ __forceinline__ bool mc_face_ok(const int32_t* faces, uint32_t f, uint32_t V,
                                           int32_t& a, int32_t& b, int32_t& c) {
    a = faces[3 * (uint64_t)f]; b = faces[3 * (uint64_t)f + 1]; c = faces[3 * (uint64_t)f + 2];
    return (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;
}

struct RootPred {          // vertex v is the root of its component
    const int32_t* L;
    __device__ bool operator()(uint32_t v) const { return L[v] == (int32_t)v; }
};
struct KeepVertex {
    const int32_t* label; const uint8_t* keep; uint32_t C;
    __device__ bool operator()(uint32_t v) const {
        const uint32_t c = (uint32_t)label[v];
        return c < C && keep[c] != 0;
    }
};
struct KeepFace {          // a face goes with the component of its vertices
    const int32_t* faces; const int32_t* label; const uint8_t* keep; uint32_t V, C;
    __device__ bool operator()(uint32_t f) const {
        int32_t a, b, c;
        if (!mc_face_ok(faces, f, V, a, b, c)) return false;
        const uint32_t k = (uint32_t)label[a];
        return k < C && keep[k] != 0;
    }
};

// the flags of a scan index: per chunk the ballot, per block the count
template <typename Pred>
__global__ void __launch_bounds__(256)
k_mc_flags(ScanIdx s, Pred pred) {
    __shared__ int sCnt[MC_CHUNKS];
    const int lane = rn_lane(), wave = threadIdx.x / RN_WAVE;
    const uint32_t b = blockIdx.x;
    for (int it = 0; it < MC_CHUNKS / 4; ++it) {
        const int ch = it * 4 + wave;
        const uint32_t i = b * MC_BLK + ch * 64 + lane;
        const bool on = i < s.n && pred(i);
        const uint64_t m = __ballot(on);
        if (lane == 0) { s.bits[(uint64_t)b * MC_CHUNKS + ch] = m; sCnt[ch] = __popcll(m); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int ch = 0; ch < MC_CHUNKS; ++ch) {
            s.pre[(uint64_t)b * MC_CHUNKS + ch] = (uint16_t)run;
            run += sCnt[ch];
        }
        s.off[b] = run;
    }
}

// exclusive scan of the per-block counts in place, one block per index (a
// fixed order); off[nb] and *tot = the total
__global__ void __launch_bounds__(1024)
k_mc_scan(ScanIdx s0, int64_t* tot0, ScanIdx s1, int64_t* tot1) {
    __shared__ int64_t sPart[1024];
    const ScanIdx& s = blockIdx.x ? s1 : s0;
    int64_t* v = s.off;
    const int64_t nb = s.nb;
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    int64_t acc = 0;
    for (int64_t j = 0; j < per; ++j) { const int64_t q = t * per + j; if (q < nb) acc += v[q]; }
    sPart[t] = acc;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {           // Hillis-Steele, inclusive
        const int64_t x = t >= off ? sPart[t - off] : 0;
        __syncthreads();
        sPart[t] += x;
        __syncthreads();
    }
    int64_t run = t ? sPart[t - 1] : 0;
    for (int64_t j = 0; j < per; ++j) {
        const int64_t q = t * per + j;
        if (q < nb) { const int64_t x = v[q]; v[q] = run; run += x; }
    }
    if (t == 1023) { v[nb] = sPart[1023]; *(blockIdx.x ? tot1 : tot0) = sPart[1023]; }
}

// ---- labelling --------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_cc_init(int32_t* L, uint32_t V) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < V) L[v] = (int32_t)v;
}

__global__ void __launch_bounds__(256)
k_cc_validate(const int32_t* faces, uint32_t F, uint32_t V, int64_t* head) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    int32_t a, b, c;
    const bool bad = f < F && !mc_face_ok(faces, f, V, a, b, c);
    if (__ballot(bad) != 0 && rn_lane() == 0)
        atomicOr((unsigned long long*)&head[H_BAD], 1ull);
}

// hook: the lowest of a face's three labels onto its vertices and onto the
// vertices those labels name.  A label equal to the lowest needs no store:
// the word it was read from can only have decreased since.
__global__ void __launch_bounds__(256)
k_cc_hook(const int32_t* faces, uint32_t F, uint32_t V, int32_t* L) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int32_t v[3];
    if (!mc_face_ok(faces, f, V, v[0], v[1], v[2])) return;
    int32_t l[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) l[j] = L[v[j]];
    // labels are vertex indices by construction; the test keeps a caller's
    // bad `root` (restart == 0) from being dereferenced
    if ((uint32_t)l[0] >= V || (uint32_t)l[1] >= V || (uint32_t)l[2] >= V) return;
    const int32_t m = min(l[0], min(l[1], l[2]));
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (l[j] > m) { atomicMin(&L[v[j]], m); atomicMin(&L[l[j]], m); }
}

// jump: L[v] = L[L[L[v]]], two fixed steps, by atomicMin so that a stale read
// can never raise a label
__global__ void __launch_bounds__(256)
k_cc_jump(int32_t* L, uint32_t V) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t l = L[v];
    if ((uint32_t)l >= V) return;
    int32_t t = L[l];
    if ((uint32_t)t < V) { const int32_t t2 = L[t]; if ((uint32_t)t2 < V) t = min(t, t2); }
    if (t < l) atomicMin(&L[v], t);
}

// the fixed point, and the number of roots it has
__global__ void __launch_bounds__(256)
k_cc_check(const int32_t* faces, uint32_t F, uint32_t V, const int32_t* L, int64_t* head) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool open = false, root = false;
    if (i < F) {
        int32_t a, b, c;
        if (mc_face_ok(faces, i, V, a, b, c)) { const int32_t la = L[a]; open = la != L[b] || la != L[c]; }
    }
    if (i < V) {
        const int32_t l = L[i];
        open |= (uint32_t)l >= V || L[(uint32_t)l < V ? l : 0] != l;
        root = l == (int32_t)i;
    }
    const uint64_t mo = __ballot(open), mr = __ballot(root);
    if (rn_lane() == 0) {
        if (mo) atomicOr((unsigned long long*)&head[H_OPEN], 1ull);
        if (mr) atomicAdd((unsigned long long*)&head[H_ROOTS], (unsigned long long)__popcll(mr));
    }
}

// one add per wave where the whole wave counts into one component (the usual
// case: neighbours in index are neighbours in space), one per lane otherwise
__device__ __forceinline__ void mc_count(int64_t* cnt, bool on, int32_t id) {
    const uint64_t act = __ballot(on);
    if (act == 0) return;
    const int first = __builtin_ctzll(act);
    const int32_t id0 = __builtin_amdgcn_readlane(id, first);
    const uint64_t same = __ballot(on && id == id0);
    if (on && id != id0) atomicAdd((unsigned long long*)&cnt[id], 1ull);
    if (rn_lane() == first) atomicAdd((unsigned long long*)&cnt[id0], (unsigned long long)__popcll(same));
}

// label[v] = the rank of v's root among the roots; the components' sizes
__global__ void __launch_bounds__(256)
k_cc_label(const int32_t* L, uint32_t V, ScanIdx roots, int64_t C, int32_t* label,
           int64_t* n_vertices) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    int32_t id = 0;
    if (v < V) {
        const uint32_t r = (uint32_t)L[v];
        const int64_t k = r < V && mc_flag(roots, r) ? mc_rank(roots, r) : -1;
        on = k >= 0 && k < C;
        id = on ? (int32_t)k : -1;
        label[v] = id;
    }
    mc_count(n_vertices, on, id);
}

__global__ void __launch_bounds__(256)
k_cc_facecount(const int32_t* faces, uint32_t F, uint32_t V, const int32_t* label, int64_t C,
               int64_t* n_faces) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    int32_t id = 0;
    if (f < F) {
        int32_t a, b, c;
        if (mc_face_ok(faces, f, V, a, b, c)) { id = label[a]; on = id >= 0 && id < C; }
    }
    mc_count(n_faces, on, id);
}

// ---- compaction -------------------------------------------------------------
struct EmitArgs {
    const float* vertices; const float* normals; const uint8_t* colors; const int32_t* faces;
    float* out_vertices; float* out_normals; uint8_t* out_colors; int32_t* out_faces;
    int64_t cap_v, cap_f;
};

__global__ void __launch_bounds__(256)
k_mc_emit_vertices(ScanIdx vi, EmitArgs e) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= vi.n || !mc_flag(vi, v)) return;
    const int64_t id = mc_rank(vi, v);
    if (id >= e.cap_v) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        e.out_vertices[3 * id + d] = e.vertices[3 * (uint64_t)v + d];
        if (e.normals) e.out_normals[3 * id + d] = e.normals[3 * (uint64_t)v + d];
        if (e.colors) e.out_colors[3 * id + d] = e.colors[3 * (uint64_t)v + d];
    }
}

__global__ void __launch_bounds__(256)
k_mc_emit_faces(ScanIdx vi, ScanIdx fi, EmitArgs e) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= fi.n || !mc_flag(fi, f)) return;
    const int64_t id = mc_rank(fi, f);
    if (id >= e.cap_f) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        // a kept face's vertices are in range and kept (KeepFace, KeepVertex)
        const uint32_t v = (uint32_t)e.faces[3 * (uint64_t)f + j];
        e.out_faces[3 * id + j] = v < vi.n && mc_flag(vi, v) ? (int32_t)mc_rank(vi, v) : -1;
    }
}

// ---- host -------------------------------------------------------------------
size_t idx_bytes(uint32_t nb) {
    return ((size_t)nb + 1) * sizeof(int64_t) + (size_t)nb * MC_CHUNKS * (sizeof(uint64_t) + sizeof(uint16_t));
}

struct Work { int64_t* head; ScanIdx v, f; };

int work_fill(Work& w, const char* who, int64_t V, int64_t F, void* work) {
    RN_CHECK_ARG_AS(who, V >= 1 && F >= 0 && V < ((int64_t)1 << 31) && F < ((int64_t)1 << 31),
                    "bad counts (1 <= V < 2^31, 0 <= F < 2^31)");
    char* p = (char*)work;
    w.head = (int64_t*)p;               p += MC_HEAD * sizeof(int64_t);
    ScanIdx* s[2] = {&w.v, &w.f};
    const int64_t n[2] = {V, F};
    for (int q = 0; q < 2; ++q) {
        s[q]->n = (uint32_t)n[q];
        s[q]->nb = (uint32_t)((n[q] + MC_BLK - 1) / MC_BLK);
        s[q]->off = (int64_t*)p;        p += ((size_t)s[q]->nb + 1) * sizeof(int64_t);
        s[q]->bits = (uint64_t*)p;      p += (size_t)s[q]->nb * MC_CHUNKS * sizeof(uint64_t);
    }
    for (int q = 0; q < 2; ++q) {       // the 2-byte tables last: everything before is 8-aligned
        s[q]->pre = (uint16_t*)p;       p += (size_t)s[q]->nb * MC_CHUNKS * sizeof(uint16_t);
    }
    return 0;
}

inline uint32_t blocks256(int64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace

extern "C" {

int rn_mesh_work_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes) {
    RN_CHECK_ARG(bytes, "null pointer");
    Work w{};
    if (work_fill(w, __func__, n_vertices, n_faces, nullptr)) return 1;
    *bytes = (int64_t)(MC_HEAD * sizeof(int64_t) + idx_bytes(w.v.nb) + idx_bytes(w.f.nb));
    return 0;
}

int rn_mesh_label(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* root,
                  void* work, int32_t rounds, int32_t restart, void* stream) {
    RN_CHECK_ARG(root && work && (faces || n_faces == 0), "null pointer");
    RN_CHECK_ARG(rounds >= 0 && rounds <= 1024, "bad rounds (0 .. 1024)");
    Work w{};
    if (work_fill(w, __func__, n_vertices, n_faces, work)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t V = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    if (restart) {
        RN_CHECK_HIP(hipMemsetAsync(w.head, 0, MC_HEAD * sizeof(int64_t), st), "memset");
        k_cc_init<<<blocks256(V), 256, 0, st>>>(root, V);
        if (F) k_cc_validate<<<blocks256(F), 256, 0, st>>>(faces, F, V, w.head);
    } else {
        RN_CHECK_HIP(hipMemsetAsync(w.head + H_OPEN, 0, 2 * sizeof(int64_t), st), "memset");
    }
    for (int r = 0; r < rounds && F; ++r) {
        k_cc_hook<<<blocks256(F), 256, 0, st>>>(faces, F, V, root);
        k_cc_jump<<<blocks256(V), 256, 0, st>>>(root, V);
    }
    k_cc_check<<<blocks256(V > F ? V : F), 256, 0, st>>>(faces, F, V, root, w.head);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                       const int32_t* root, void* work, int64_t n_components, int32_t* label,
                       int64_t* comp_vertices, int64_t* comp_faces, void* stream) {
    RN_CHECK_ARG(root && work && label && comp_vertices && comp_faces && (faces || n_faces == 0),
                 "null pointer");
    RN_CHECK_ARG(n_components >= 1 && n_components <= n_vertices, "bad n_components (1 .. V)");
    Work w{};
    if (work_fill(w, __func__, n_vertices, n_faces, work)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t V = (uint32_t)n_vertices, F = (uint32_t)n_faces;
    RN_CHECK_HIP(hipMemsetAsync(comp_vertices, 0, sizeof(int64_t) * n_components, st), "memset");
    RN_CHECK_HIP(hipMemsetAsync(comp_faces, 0, sizeof(int64_t) * n_components, st), "memset");
    k_mc_flags<<<w.v.nb, 256, 0, st>>>(w.v, RootPred{root});
    k_mc_scan<<<1, 1024, 0, st>>>(w.v, w.head + H_ROOTS, w.v, w.head + H_ROOTS);
    k_cc_label<<<blocks256(V), 256, 0, st>>>(root, V, w.v, n_components, label, comp_vertices);
    if (F) k_cc_facecount<<<blocks256(F), 256, 0, st>>>(faces, F, V, label, n_components, comp_faces);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_mesh_compact_count(const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                          const int32_t* label, const uint8_t* keep, int64_t n_components,
                          void* work, void* stream) {
    RN_CHECK_ARG(label && keep && work && (faces || n_faces == 0), "null pointer");
    RN_CHECK_ARG(n_components >= 1 && n_components <= n_vertices, "bad n_components (1 .. V)");
    Work w{};
    if (work_fill(w, __func__, n_vertices, n_faces, work)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t V = (uint32_t)n_vertices, C = (uint32_t)n_components;
    k_mc_flags<<<w.v.nb, 256, 0, st>>>(w.v, KeepVertex{label, keep, C});
    if (w.f.nb) k_mc_flags<<<w.f.nb, 256, 0, st>>>(w.f, KeepFace{faces, label, keep, V, C});
    k_mc_scan<<<2, 1024, 0, st>>>(w.v, w.head + H_KEPT_V, w.f, w.head + H_KEPT_F);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_mesh_compact_emit(const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                         const void* work, const float* vertices, const float* normals,
                         const uint8_t* colors, int64_t kept_vertices, int64_t kept_faces,
                         float* out_vertices, float* out_normals, uint8_t* out_colors,
                         int32_t* out_faces, void* stream) {
    RN_CHECK_ARG(work && vertices && (faces || n_faces == 0), "null pointer");
    RN_CHECK_ARG(kept_vertices >= 0 && kept_vertices <= n_vertices && kept_faces >= 0 &&
                 kept_faces <= n_faces, "bad kept counts");
    RN_CHECK_ARG((kept_vertices == 0 || (out_vertices && (!normals || out_normals) &&
                                         (!colors || out_colors))) &&
                 (kept_faces == 0 || out_faces), "null output");
    Work w{};
    if (work_fill(w, __func__, n_vertices, n_faces, const_cast<void*>(work))) return 1;
    hipStream_t st = (hipStream_t)stream;
    EmitArgs e{vertices, normals, colors, faces, out_vertices, out_normals, out_colors, out_faces,
               kept_vertices, kept_faces};
    if (kept_vertices) k_mc_emit_vertices<<<blocks256(n_vertices), 256, 0, st>>>(w.v, e);
    if (kept_faces) k_mc_emit_faces<<<blocks256(n_faces), 256, 0, st>>>(w.v, w.f, e);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
