// Mesh export for gfx950: the density lattice of a trained model and the
// naive surface-nets extraction of its iso-surface (radnerf_amd/mesh.py).
//  * k_density_lattice: sigma on a regular lattice of points, the weighted sum
//    of the live sub-NeRFs' MNGP.density.  The sub-NeRFs share the hash grid
//    (one xyz_encoder per MNGP), so a tile's 32 points are encoded ONCE and
//    only the geo MLP (8 fragments, 8 KB per sub-NeRF, in LDS) runs per
//    sub-NeRF; the points come from the lattice index, there is no xyz buffer.
//  * k_sn_classify / k_sn_scan / k_sn_emit: one vertex per sign-changing cell,
//    one quad per sign-changing interior lattice edge, numbered by exclusive
//    scans in ascending lattice order -- no atomic decides an order, the
//    output is a function of the lattice alone.  The rules are stated in
//    include/radnerf.h (rn_surface_count) and restated in numpy by
//    tests/mesh_ref.py.
// Cells are indexed by their lowest corner's POINT index p = i + px (j + py k)
// (px = nx + 1 points per row): ascending p over the cells is ascending
// c = i + nx (j + ny k), so one scan over the points numbers both the
// vertices (cells) and the quads (3 p + a).
#include "rn_field.h"
#include "rn_march.h"
#pragma clang fp contract(off)

#define ML_KMAX 16         // sub-NeRFs of one MNGP (the gate's rows)
#define ML_LDS_K 8         // geo fragments resident in LDS at a time (8 KB each)
#define ML_GEO_HALFS (8 * RN_FRAG_HALFS)

#define SN_BLK 1024        // lattice points per counting block: 16 wave chunks
#define SN_CHUNKS (SN_BLK / 64)

namespace {

struct LatticeArgs {
    uint32_t px, py;               // points per row / per column (n + 1)
    int64_t n;                     // lattice points (< 2^31)
    float lo[3], step[3];
    int n_live;
    int32_t idx[ML_KMAX];          // the live sub-NeRFs, ascending
    float w[ML_KMAX];              // and their weights
    float* out;
};

// the occupancy mask of rn_density_lattice_masked: the live sub-NeRFs' own
// bitfields, in the order of LatticeArgs.idx, and the march's grid
struct MaskArgs {
    const uint8_t* bits[ML_KMAX];
    int cascades, grid_size;
    float scale;
};

// bit q set: the point's cell is set in live sub-NeRF q's bitfield.  The cell
// is the one march_step (rn_march.h) queries for the position, the dt term
// dropped.
__device__ __forceinline__ uint32_t lattice_live(const MaskArgs& m, int n_live, float x, float y,
                                                 float z) {
    const int mip = rn_mip_from_pos(x, y, z, m.cascades);
    const float mbi = mip_bound_inv(mip, m.scale);
    const float gm1 = m.grid_size - 1.0f;
    const int nx = (int)rn_clampf(0.5f * fmaf(x, mbi, 1.0f) * m.grid_size, 0.0f, gm1);
    const int ny = (int)rn_clampf(0.5f * fmaf(y, mbi, 1.0f) * m.grid_size, 0.0f, gm1);
    const int nz = (int)rn_clampf(0.5f * fmaf(z, mbi, 1.0f) * m.grid_size, 0.0f, gm1);
    const uint32_t g3 = (uint32_t)m.grid_size * m.grid_size * m.grid_size;
    const uint32_t idx = mip * g3 + rn_morton3d(nx, ny, nz);
    uint32_t live = 0;
    for (int q = 0; q < n_live; ++q)
        live |= (uint32_t)((m.bits[q][idx >> 3] >> (idx & 7)) & 1) << q;
    return live;
}

// acc = w_0 sigma_0, then acc + w_k sigma_k for the live k ascending.  More
// than ML_LDS_K live sub-NeRFs run in groups: a later group encodes the
// points again and continues from the stored sum (the same additions).
__global__ void __launch_bounds__(512)
k_density_lattice(FieldArgs a, LatticeArgs g) {
    extern __shared__ __attribute__((aligned(16))) rn_half sWl[];   // [<= ML_LDS_K][8 geo frags]
    __shared__ LvTab sT;
    lv_stage(sT, a.gm);
    const int64_t n_tiles = (g.n + 31) / 32;
    const int waves = blockDim.x / RN_WAVE;
    const int lane = rn_lane(), c = lane & 31, h = lane >> 5;
    const __amdgpu_buffer_rsrc_t rs = rn_rsrc(a.grid, a.grid_bytes);
    for (int kb = 0; kb < g.n_live; kb += ML_LDS_K) {
        const int ke = min(g.n_live, kb + ML_LDS_K);
        __syncthreads();                                   // the previous group's tiles are done
        for (int q = kb; q < ke; ++q)
            rn_block_copy16(sWl + (size_t)(q - kb) * ML_GEO_HALFS,
                            a.frags + (size_t)g.idx[q] * FIELD_FRAGS * RN_FRAG_HALFS,
                            8 * RN_FRAG_BYTES);
        __syncthreads();
        for (int64_t tile = (int64_t)blockIdx.x * waves + threadIdx.x / RN_WAVE; tile < n_tiles;
             tile += (int64_t)gridDim.x * waves) {
            rn_lds_order();
            const int64_t i = tile * 32 + c;
            const bool valid = i < g.n;
            const uint32_t p = valid ? (uint32_t)i : 0u;
            const uint32_t row = p / g.px, pi = p - row * g.px;
            const uint32_t pk = row / g.py, pj = row - pk * g.py;
            // point i of an axis: lo + (float)i * step, a multiply then an add
            const float x = g.lo[0] + (float)pi * g.step[0];
            const float y = g.lo[1] + (float)pj * g.step[1];
            const float z = g.lo[2] + (float)pk * g.step[2];
            const float ux = unit_coord(x, a.xyz_min[0], a.extent[0]);
            const float uy = unit_coord(y, a.xyz_min[1], a.extent[1]);
            const float uz = unit_coord(z, a.xyz_min[2], a.extent[2]);
            half8 e0, e1;
            encode_lane(a, sT, rs, h, ux, uy, uz, valid, e0, e1);
            // geo layer 1 is the same for every sub-NeRF only in its input:
            // the weights differ, so the whole geo MLP runs per sub-NeRF
            float acc = (kb && valid && h == 0) ? g.out[p] : 0.f;
            for (int q = kb; q < ke; ++q) {
                const rn_half* sW = sWl + (size_t)(q - kb) * ML_GEO_HALFS;
                f32x16 a0 = rn_zero16(), a1 = rn_zero16();
                a0 = rn_mfma(rn_frag(sW, 0), e0, a0); a0 = rn_mfma(rn_frag(sW, 1), e1, a0);
                a1 = rn_mfma(rn_frag(sW, 2), e0, a1); a1 = rn_mfma(rn_frag(sW, 3), e1, a1);
                half8 h1[4];
                rn_acc_to_frags<true>(a0, h1[0], h1[1]);
                rn_acc_to_frags<true>(a1, h1[2], h1[3]);
                f32x16 gg = rn_zero16();
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) gg = rn_mfma(rn_frag(sW, 4 + qq), h1[qq], gg);
                const float t = g.w[q] * expf(gg[8]);
                acc = q == 0 ? t : acc + t;
            }
            if (valid && h == 0) g.out[p] = acc;
        }
    }
}

// k_density_lattice with the occupancy mask, a kernel of its own (the unmasked
// one carries no mask argument and no test of one): sigma_k counts as 0 where
// sub-NeRF k's bitfield is clear.  A tile that is dead for the whole group
// skips the encode and the MLPs, a sub-NeRF dead on the whole tile its MLP;
// both tests are ballots, wave-uniform, so no divergence surrounds the MFMAs.
// A live point's terms are the unmasked kernel's, added in its order.
__global__ void __launch_bounds__(512)
k_density_lattice_masked(FieldArgs a, LatticeArgs g, MaskArgs m) {
    extern __shared__ __attribute__((aligned(16))) rn_half sWl[];   // [<= ML_LDS_K][8 geo frags]
    __shared__ LvTab sT;
    lv_stage(sT, a.gm);
    const int64_t n_tiles = (g.n + 31) / 32;
    const int waves = blockDim.x / RN_WAVE;
    const int lane = rn_lane(), c = lane & 31, h = lane >> 5;
    const __amdgpu_buffer_rsrc_t rs = rn_rsrc(a.grid, a.grid_bytes);
    for (int kb = 0; kb < g.n_live; kb += ML_LDS_K) {
        const int ke = min(g.n_live, kb + ML_LDS_K);
        __syncthreads();                                   // the previous group's tiles are done
        for (int q = kb; q < ke; ++q)
            rn_block_copy16(sWl + (size_t)(q - kb) * ML_GEO_HALFS,
                            a.frags + (size_t)g.idx[q] * FIELD_FRAGS * RN_FRAG_HALFS,
                            8 * RN_FRAG_BYTES);
        __syncthreads();
        for (int64_t tile = (int64_t)blockIdx.x * waves + threadIdx.x / RN_WAVE; tile < n_tiles;
             tile += (int64_t)gridDim.x * waves) {
            rn_lds_order();
            const int64_t i = tile * 32 + c;
            const bool valid = i < g.n;
            const uint32_t p = valid ? (uint32_t)i : 0u;
            const uint32_t row = p / g.px, pi = p - row * g.px;
            const uint32_t pk = row / g.py, pj = row - pk * g.py;
            // point i of an axis: lo + (float)i * step, a multiply then an add
            const float x = g.lo[0] + (float)pi * g.step[0];
            const float y = g.lo[1] + (float)pj * g.step[1];
            const float z = g.lo[2] + (float)pk * g.step[2];
            const uint32_t live = valid ? lattice_live(m, g.n_live, x, y, z) : 0u;
            const uint32_t grp = (live >> kb) & ((1u << (ke - kb)) - 1u);
            if (__builtin_amdgcn_ballot_w64(grp != 0) == 0) {          // a dead tile
                if (kb == 0 && valid && h == 0) g.out[p] = 0.f;
                continue;
            }
            const float ux = unit_coord(x, a.xyz_min[0], a.extent[0]);
            const float uy = unit_coord(y, a.xyz_min[1], a.extent[1]);
            const float uz = unit_coord(z, a.xyz_min[2], a.extent[2]);
            half8 e0, e1;
            encode_lane(a, sT, rs, h, ux, uy, uz, valid, e0, e1);
            // geo layer 1 is the same for every sub-NeRF only in its input:
            // the weights differ, so the whole geo MLP runs per sub-NeRF
            float acc = (kb && valid && h == 0) ? g.out[p] : 0.f;
            for (int q = kb; q < ke; ++q) {
                const bool on = (live >> q) & 1;
                float sg = 0.f;
                if (__builtin_amdgcn_ballot_w64(on) != 0) {
                    const rn_half* sW = sWl + (size_t)(q - kb) * ML_GEO_HALFS;
                    f32x16 a0 = rn_zero16(), a1 = rn_zero16();
                    a0 = rn_mfma(rn_frag(sW, 0), e0, a0); a0 = rn_mfma(rn_frag(sW, 1), e1, a0);
                    a1 = rn_mfma(rn_frag(sW, 2), e0, a1); a1 = rn_mfma(rn_frag(sW, 3), e1, a1);
                    half8 h1[4];
                    rn_acc_to_frags<true>(a0, h1[0], h1[1]);
                    rn_acc_to_frags<true>(a1, h1[2], h1[3]);
                    f32x16 gg = rn_zero16();
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) gg = rn_mfma(rn_frag(sW, 4 + qq), h1[qq], gg);
                    sg = on ? expf(gg[8]) : 0.f;
                }
                const float t = g.w[q] * sg;
                acc = q == 0 ? t : acc + t;
            }
            if (valid && h == 0) g.out[p] = acc;
        }
    }
}

// ---------------------------------------------------------------------------
// Surface nets.  Workspace (rn_surface_work_bytes), nb = ceil(points / 1024):
//   tot  [2] int64       vertices, quads (what the host reads, once)
//   voff [nb + 1] int64  per block: vertex count -> first vertex id
//   qoff [nb + 1] int64  per block: quad count -> first quad id
//   bits [16 nb][4] u64  per 64-point chunk: ballots of "cell active" and of
//                        "edge along a emits a quad", a = 0, 1, 2
//   pre  [16 nb][2] u16  per chunk: vertices / quads of the block's earlier chunks
// 592 B per 1024 points = 0.58 B per lattice point.  The id of the vertex of
// the cell at point p is voff[p >> 10] + pre[p >> 6][0] + popcount(bits[p >> 6][0]
// below lane p & 63): any cell's id is three small reads, no per-cell table.
// ---------------------------------------------------------------------------
struct SurfArgs {
    const float* s;
    const float* w;                // rn_surface_count_valid: the observation counts, else null
    uint32_t nx, ny, nz, px, py;   // cells per axis; points per row / column
    uint32_t n_pts, nb;
    float iso;
    float lo[3], step[3];
    int64_t* tot; int64_t* voff; int64_t* qoff;
    uint64_t* bits; uint16_t* pre;
    int64_t cap_v, cap_q;          // rows the outputs hold
    float* vertices; float* normals; int32_t* faces;
};

__device__ __forceinline__ bool sn_inside(float v, float iso) { return v >= iso; }   // NaN: outside

__device__ __forceinline__ void sn_coords(const SurfArgs& u, uint32_t p, uint32_t& pi, uint32_t& pj,
                                          uint32_t& pk) {
    const uint32_t row = p / u.px;
    pi = p - row * u.px;
    pk = row / u.py;
    pj = row - pk * u.py;
}

// the 8 corners of the cell at (pi, pj, pk); a coordinate past the lattice is
// clamped to its last point (such a cell is never active, such an edge never
// emits: the value is loaded and not used)
__device__ __forceinline__ void sn_corners(const SurfArgs& u, uint32_t pi, uint32_t pj, uint32_t pk,
                                           float* v) {
    const uint32_t x1 = min(pi + 1, u.nx), y1 = min(pj + 1, u.ny), z1 = min(pk + 1, u.nz);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t x = (q & 1) ? x1 : pi, y = (q & 2) ? y1 : pj, z = (q & 4) ? z1 : pk;
        v[q] = u.s[x + u.px * (y + u.py * z)];
    }
}

// VALID: every corner of the cell at (pi, pj, pk) is observed (w > 0; NaN is
// not).  A cell past the lattice clamps as sn_corners does: it is never active.
__device__ __forceinline__ bool sn_cell_valid(const SurfArgs& u, uint32_t pi, uint32_t pj,
                                              uint32_t pk) {
    const uint32_t x1 = min(pi + 1, u.nx), y1 = min(pj + 1, u.ny), z1 = min(pk + 1, u.nz);
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t x = (q & 1) ? x1 : pi, y = (q & 2) ? y1 : pj, z = (q & 4) ? z1 : pk;
        ok &= u.w[x + u.px * (y + u.py * z)] > 0.f;
    }
    return ok;
}

// 1. classify every lattice point: is its cell active, which of its three
// edges emit a quad; per chunk the ballots, per block the counts.  VALID
// (rn_surface_count_valid): a cell with an unobserved corner is not active, an
// edge with such a cell among its four emits nothing; the four cells of an
// interior edge lie inside the lattice, and the branch runs only at a sign
// change.  Every other line is the same code for both.
template <bool VALID>
__global__ void __launch_bounds__(256)
k_sn_classify(SurfArgs u) {
    __shared__ int sCnt[SN_CHUNKS][2];
    const int lane = rn_lane(), wave = threadIdx.x / RN_WAVE;
    const uint32_t b = blockIdx.x;
    for (int it = 0; it < SN_CHUNKS / 4; ++it) {
        const int ch = it * 4 + wave;
        const uint32_t p = b * SN_BLK + ch * 64 + lane;
        bool cell = false, qa[3] = {false, false, false};
        if (p < u.n_pts) {
            uint32_t P[3];
            sn_coords(u, p, P[0], P[1], P[2]);
            float v[8];
            sn_corners(u, P[0], P[1], P[2], v);
            bool in[8], any = false, all = true;
#pragma unroll
            for (int q = 0; q < 8; ++q) { in[q] = sn_inside(v[q], u.iso); any |= in[q]; all &= in[q]; }
            const uint32_t n[3] = {u.nx, u.ny, u.nz};
            cell = P[0] < n[0] && P[1] < n[1] && P[2] < n[2] && any && !all;
            if (VALID && cell) cell = sn_cell_valid(u, P[0], P[1], P[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int bb = (a + 1) % 3, cc = (a + 2) % 3;
                qa[a] = in[0] != in[1 << a] && P[a] < n[a] && P[bb] >= 1 && P[bb] < n[bb] &&
                        P[cc] >= 1 && P[cc] < n[cc];
                if (VALID && qa[a]) {
                    uint32_t Q[3] = {P[0], P[1], P[2]};
                    bool ok = sn_cell_valid(u, Q[0], Q[1], Q[2]);
                    Q[bb] -= 1; ok = ok && sn_cell_valid(u, Q[0], Q[1], Q[2]);
                    Q[cc] -= 1; ok = ok && sn_cell_valid(u, Q[0], Q[1], Q[2]);
                    Q[bb] += 1; ok = ok && sn_cell_valid(u, Q[0], Q[1], Q[2]);
                    qa[a] = ok;
                }
            }
        }
        const uint64_t m0 = __ballot(cell), m1 = __ballot(qa[0]), m2 = __ballot(qa[1]),
                       m3 = __ballot(qa[2]);
        if (lane == 0) {
            uint64_t* w = u.bits + ((uint64_t)b * SN_CHUNKS + ch) * 4;
            w[0] = m0; w[1] = m1; w[2] = m2; w[3] = m3;
            sCnt[ch][0] = __popcll(m0);
            sCnt[ch][1] = __popcll(m1) + __popcll(m2) + __popcll(m3);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int w = threadIdx.x;
        int run = 0;
        for (int ch = 0; ch < SN_CHUNKS; ++ch) {
            u.pre[((uint64_t)b * SN_CHUNKS + ch) * 2 + w] = (uint16_t)run;
            run += sCnt[ch][w];
        }
        (w ? u.qoff : u.voff)[b] = run;
    }
}

// 2. exclusive scans of the per-block counts in place (block 0: vertices,
// block 1: quads; one block each, a fixed order): v[nb] and tot[] = the total
__global__ void __launch_bounds__(1024)
k_sn_scan(SurfArgs u) {
    __shared__ int64_t sPart[1024];
    int64_t* v = blockIdx.x ? u.qoff : u.voff;
    const int64_t nb = u.nb;
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
    if (t == 1023) { v[nb] = sPart[1023]; u.tot[blockIdx.x] = sPart[1023]; }
}

__device__ __forceinline__ uint64_t sn_below(int lane) { return (1ull << lane) - 1ull; }

// the vertex id of the (active) cell at point p
__device__ __forceinline__ int64_t sn_vertex_id(const SurfArgs& u, uint32_t p) {
    const uint32_t ch = p >> 6;
    return u.voff[p >> 10] + u.pre[(uint64_t)ch * 2] +
           __popcll(u.bits[(uint64_t)ch * 4] & sn_below(p & 63));
}

// the vertex of the active cell at (pi, pj, pk): mean of the edge crossings,
// and the normal from the summed edge differences
__device__ __forceinline__ void sn_vertex(const SurfArgs& u, const uint32_t* P, int64_t vid) {
    float v[8];
    sn_corners(u, P[0], P[1], P[2], v);
    float sum[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int r0 = a == 0 ? 1 : 0, r1 = a == 2 ? 1 : 2;   // the remaining axes, lower / higher
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q0 = ((e & 1) << r0) | ((e >> 1) << r1), q1 = q0 | (1 << a);
            const float s0 = v[q0], s1 = v[q1];
            g[a] = g[a] + (s1 - s0);
            if (sn_inside(s0, u.iso) != sn_inside(s1, u.iso)) {
                float t = (u.iso - s0) / (s1 - s0);
                t = fminf(fmaxf(t, 0.f), 1.f);             // NaN -> 0
                sum[a] = sum[a] + t;
                sum[r0] = sum[r0] + (float)(e & 1);
                sum[r1] = sum[r1] + (float)(e >> 1);
                cnt = cnt + 1.f;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float pos = (float)P[d] + sum[d] / cnt;
        u.vertices[3 * vid + d] = u.lo[d] + pos * u.step[d];
    }
    if (u.normals) {
        const float nrm = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        const bool ok = isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && nrm > 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) u.normals[3 * vid + d] = ok ? -g[d] / nrm : 0.f;
    }
}

// 3. emit: vertices (and normals) of the active cells, two triangles per quad
__global__ void __launch_bounds__(256)
k_sn_emit(SurfArgs u) {
    const int lane = rn_lane(), wave = threadIdx.x / RN_WAVE;
    const uint32_t b = blockIdx.x;
    const int64_t v0 = u.voff[b], q0 = u.qoff[b];
    for (int it = 0; it < SN_CHUNKS / 4; ++it) {
        const uint32_t ch = b * SN_CHUNKS + it * 4 + wave;
        const uint64_t* w = u.bits + (uint64_t)ch * 4;
        const uint64_t m0 = w[0], m1 = w[1], m2 = w[2], m3 = w[3];
        if ((m0 | m1 | m2 | m3) == 0) continue;            // wave-uniform
        const uint32_t p = ch * 64 + lane;
        const uint64_t lt = sn_below(lane);
        uint32_t P[3];
        sn_coords(u, p, P[0], P[1], P[2]);
        if ((m0 >> lane) & 1) {
            const int64_t vid = v0 + u.pre[(uint64_t)ch * 2] + __popcll(m0 & lt);
            if (vid < u.cap_v) sn_vertex(u, P, vid);
        }
        const uint32_t own = (uint32_t)((m1 >> lane) & 1) | (uint32_t)((m2 >> lane) & 1) << 1 |
                             (uint32_t)((m3 >> lane) & 1) << 2;
        if (!own) continue;
        const int64_t qb = q0 + u.pre[(uint64_t)ch * 2 + 1] + __popcll(m1 & lt) + __popcll(m2 & lt) +
                           __popcll(m3 & lt);
        const bool in = sn_inside(u.s[p], u.iso);
        const uint32_t stride[3] = {1u, u.px, u.px * u.py};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!((own >> a) & 1)) continue;
            const int64_t qid = qb + __popc(own & ((1u << a) - 1u));
            if (qid >= u.cap_q) continue;
            const uint32_t sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];
            // the four cells round the edge, (b, c) offsets (-1,-1) (0,-1) (0,0) (-1,0)
            const int32_t c0 = (int32_t)sn_vertex_id(u, p - sb - sc);
            const int32_t c1 = (int32_t)sn_vertex_id(u, p - sc);
            const int32_t c2 = (int32_t)sn_vertex_id(u, p);
            const int32_t c3 = (int32_t)sn_vertex_id(u, p - sb);
            // P inside: the surface faces +a, (v0, v1, v2, v3); else (v0, v3, v2, v1)
            const int32_t e1 = in ? c1 : c3, e3 = in ? c3 : c1;
            int32_t* f = u.faces + 6 * qid;
            f[0] = c0; f[1] = e1; f[2] = c2;
            f[3] = c0; f[4] = c2; f[5] = e3;
        }
    }
}

// sizes and the workspace's sections; status 1 for a bad lattice
int sn_fill(SurfArgs& u, const char* who, const float* sigma, int32_t nx, int32_t ny, int32_t nz,
            void* work) {
    RN_CHECK_ARG_AS(who, nx >= 1 && ny >= 1 && nz >= 1, "bad sizes (cells per axis >= 1)");
    const int64_t n_pts = ((int64_t)nx + 1) * ((int64_t)ny + 1) * ((int64_t)nz + 1);
    RN_CHECK_ARG_AS(who, n_pts < ((int64_t)1 << 31), "lattice of 2^31 points or more");
    u.s = sigma;
    u.nx = nx; u.ny = ny; u.nz = nz; u.px = nx + 1; u.py = ny + 1;
    u.n_pts = (uint32_t)n_pts;
    u.nb = (uint32_t)((n_pts + SN_BLK - 1) / SN_BLK);
    char* w = (char*)work;
    u.tot = (int64_t*)w;            w += 2 * sizeof(int64_t);
    u.voff = (int64_t*)w;           w += ((size_t)u.nb + 1) * sizeof(int64_t);
    u.qoff = (int64_t*)w;           w += ((size_t)u.nb + 1) * sizeof(int64_t);
    u.bits = (uint64_t*)w;          w += (size_t)u.nb * SN_CHUNKS * 4 * sizeof(uint64_t);
    u.pre = (uint16_t*)w;           w += (size_t)u.nb * SN_CHUNKS * 2 * sizeof(uint16_t);
    return 0;
}

// both lattice entries: `bitfields` null is the unmasked launch
int lattice_launch(const char* who, int32_t nx, int32_t ny, int32_t nz, const float* lo,
                   const float* step, const float* weights, int32_t n_models, const void* grid_f16,
                   const uint32_t* level_offset, const uint32_t* level_hsize,
                   const uint32_t* level_res, const float* level_scale, const float* xyz_min,
                   const float* extent, const void* frags, const void* const* bitfields,
                   int32_t cascades, int32_t grid_size, float scale, float* sigma, void* stream) {
    RN_CHECK_ARG_AS(who, nx >= 1 && ny >= 1 && nz >= 1 && n_models >= 1 && n_models <= ML_KMAX,
                    "bad sizes (cells per axis >= 1, n_models <= 16)");
    const int64_t n = ((int64_t)nx + 1) * ((int64_t)ny + 1) * ((int64_t)nz + 1);
    RN_CHECK_ARG_AS(who, n < ((int64_t)1 << 31), "lattice of 2^31 points or more");
    RN_CHECK_ARG_AS(who, lo && step && weights && grid_f16 && level_offset && level_hsize &&
                    level_res && level_scale && xyz_min && extent && frags && sigma, "null pointer");
    FieldArgs a{};
    fill_args(a, xyz_min, extent, level_offset, level_hsize, level_res, level_scale);
    a.grid = (const rn_half*)grid_f16; a.frags = (const rn_half*)frags;
    LatticeArgs g{};
    g.px = nx + 1; g.py = ny + 1; g.n = n; g.out = sigma;
    for (int d = 0; d < 3; ++d) { g.lo[d] = lo[d]; g.step[d] = step[d]; }
    for (int k = 0; k < n_models; ++k)
        if (weights[k] != 0.f) { g.idx[g.n_live] = k; g.w[g.n_live] = weights[k]; ++g.n_live; }
    MaskArgs m{};
    if (bitfields) {
        // Morton codes hold 10 bits per axis; a cascade's bits fill whole bytes
        RN_CHECK_ARG_AS(who, cascades >= 1 && cascades <= 32 && grid_size >= 2 && grid_size <= 1024 &&
                        (grid_size & (grid_size - 1)) == 0 && scale > 0.f,
                        "bad grid (cascades 1 .. 32, grid_size a power of two 2 .. 1024, scale > 0)");
        for (int q = 0; q < g.n_live; ++q) {
            m.bits[q] = (const uint8_t*)bitfields[g.idx[q]];
            RN_CHECK_ARG_AS(who, m.bits[q], "null bitfield");
        }
        m.cascades = cascades; m.grid_size = grid_size; m.scale = scale;
    }
    hipStream_t st = (hipStream_t)stream;
    if (g.n_live == 0) {                                   // the empty sum
        RN_CHECK_HIP_AS(who, hipMemsetAsync(sigma, 0, sizeof(float) * n, st), "memset");
        return 0;
    }
    const int resident = g.n_live < ML_LDS_K ? g.n_live : ML_LDS_K;
    // 8 KB of LDS per resident sub-NeRF: wider blocks keep the waves per CU up
    const int threads = resident <= 4 ? 256 : 512;
    const int waves = threads / RN_WAVE;
    const int64_t tiles = (n + 31) / 32;
    const int blocks = (int)(tiles / waves + 1 < 8192 ? tiles / waves + 1 : 8192);
    const size_t lds = (size_t)resident * 8 * RN_FRAG_BYTES;
    if (bitfields) k_density_lattice_masked<<<blocks, threads, lds, st>>>(a, g, m);
    else k_density_lattice<<<blocks, threads, lds, st>>>(a, g);
    RN_CHECK_LAUNCH_AS(who);
    return 0;
}

// both emit entries
int emit_launch(const char* who, const float* sigma, int32_t nx, int32_t ny, int32_t nz, float iso,
                const float* lo, const float* step, const void* work, int64_t n_vertices,
                int64_t n_quads, float* vertices, float* normals, int32_t* faces, void* stream) {
    RN_CHECK_ARG_AS(who, sigma && work && lo && step, "null pointer");
    RN_CHECK_ARG_AS(who, n_vertices >= 0 && n_quads >= 0 && n_vertices < ((int64_t)1 << 31) &&
                    2 * n_quads < ((int64_t)1 << 31), "bad counts (vertices, triangles < 2^31)");
    RN_CHECK_ARG_AS(who, (n_vertices == 0 || vertices) && (n_quads == 0 || faces), "null output");
    SurfArgs u{};
    if (sn_fill(u, who, sigma, nx, ny, nz, const_cast<void*>(work))) return 1;
    u.iso = iso;
    for (int d = 0; d < 3; ++d) { u.lo[d] = lo[d]; u.step[d] = step[d]; }
    u.cap_v = n_vertices; u.cap_q = n_quads;
    u.vertices = vertices; u.normals = normals; u.faces = faces;
    if (n_vertices == 0 && n_quads == 0) return 0;
    k_sn_emit<<<u.nb, 256, 0, (hipStream_t)stream>>>(u);
    RN_CHECK_LAUNCH_AS(who);
    return 0;
}

}  // namespace

extern "C" {

int rn_density_lattice(int32_t nx, int32_t ny, int32_t nz, const float* lo, const float* step,
                       const float* weights, int32_t n_models, const void* grid_f16,
                       const uint32_t* level_offset, const uint32_t* level_hsize,
                       const uint32_t* level_res, const float* level_scale, const float* xyz_min,
                       const float* extent, const void* frags, float* sigma, void* stream) {
    return lattice_launch(__func__, nx, ny, nz, lo, step, weights, n_models, grid_f16, level_offset,
                          level_hsize, level_res, level_scale, xyz_min, extent, frags, nullptr, 0,
                          0, 0.f, sigma, stream);
}

int rn_density_lattice_masked(int32_t nx, int32_t ny, int32_t nz, const float* lo,
                              const float* step, const float* weights, int32_t n_models,
                              const void* grid_f16, const uint32_t* level_offset,
                              const uint32_t* level_hsize, const uint32_t* level_res,
                              const float* level_scale, const float* xyz_min, const float* extent,
                              const void* frags, const void* const* bitfields, int32_t cascades,
                              int32_t grid_size, float scale, float* sigma, void* stream) {
    RN_CHECK_ARG(bitfields, "null pointer");
    return lattice_launch(__func__, nx, ny, nz, lo, step, weights, n_models, grid_f16, level_offset,
                          level_hsize, level_res, level_scale, xyz_min, extent, frags, bitfields,
                          cascades, grid_size, scale, sigma, stream);
}

int rn_surface_work_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes) {
    RN_CHECK_ARG(bytes, "null pointer");
    SurfArgs u{};
    if (sn_fill(u, __func__, nullptr, nx, ny, nz, nullptr)) return 1;
    *bytes = (int64_t)(2 * sizeof(int64_t) + 2 * ((size_t)u.nb + 1) * sizeof(int64_t) +
                       (size_t)u.nb * SN_CHUNKS * (4 * sizeof(uint64_t) + 2 * sizeof(uint16_t)));
    return 0;
}

int rn_surface_count(const float* sigma, int32_t nx, int32_t ny, int32_t nz, float iso,
                     void* work, void* stream) {
    RN_CHECK_ARG(sigma && work, "null pointer");
    SurfArgs u{};
    if (sn_fill(u, __func__, sigma, nx, ny, nz, work)) return 1;
    u.iso = iso;
    hipStream_t st = (hipStream_t)stream;
    k_sn_classify<false><<<u.nb, 256, 0, st>>>(u);
    k_sn_scan<<<2, 1024, 0, st>>>(u);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_surface_count_valid(const float* phi, const float* w, int32_t nx, int32_t ny, int32_t nz,
                           float iso, void* work, void* stream) {
    RN_CHECK_ARG(phi && w && work, "null pointer");
    SurfArgs u{};
    if (sn_fill(u, __func__, phi, nx, ny, nz, work)) return 1;
    u.w = w;
    u.iso = iso;
    hipStream_t st = (hipStream_t)stream;
    k_sn_classify<true><<<u.nb, 256, 0, st>>>(u);
    k_sn_scan<<<2, 1024, 0, st>>>(u);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_surface_emit(const float* sigma, int32_t nx, int32_t ny, int32_t nz, float iso,
                    const float* lo, const float* step, const void* work, int64_t n_vertices,
                    int64_t n_quads, float* vertices, float* normals, int32_t* faces,
                    void* stream) {
    return emit_launch(__func__, sigma, nx, ny, nz, iso, lo, step, work, n_vertices, n_quads,
                       vertices, normals, faces, stream);
}

int rn_surface_emit_valid(const float* phi, const float* w, int32_t nx, int32_t ny, int32_t nz,
                          float iso, const float* lo, const float* step, const void* work,
                          int64_t n_vertices, int64_t n_quads, float* vertices, float* normals,
                          int32_t* faces, void* stream) {
    // the classification in work carries the observation rules: the emit reads
    // the ballots and the values of active cells, all of whose corners are observed
    RN_CHECK_ARG(w, "null pointer");
    return emit_launch(__func__, phi, nx, ny, nz, iso, lo, step, work, n_vertices, n_quads,
                       vertices, normals, faces, stream);
}

}  // extern "C"
