// Occupancy-grid maintenance kernels + library-wide error/version plumbing.
//
// Reference: models/csrc/raymarching.cu:62-161 (morton3D, morton3D_invert,
// packbits), used by MNGP.update_density_grid (models/networks.py:330-409).
#include "rn_common.h"
#include "rn_sig.h"
#include <stdarg.h>
#include <stdio.h>
#pragma clang fp contract(off)

static thread_local char g_err[512] = {0};

extern "C" void rn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

__global__ void __launch_bounds__(256)
k_morton3d(int64_t n, const int32_t* __restrict__ coords, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (int32_t)rn_morton3d(coords[3 * i], coords[3 * i + 1], coords[3 * i + 2]);
}

__global__ void __launch_bounds__(256)
k_morton3d_invert(int64_t n, const int32_t* __restrict__ idx, int32_t* __restrict__ coords) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = (uint32_t)idx[i];
    coords[3 * i + 0] = rn_morton3d_invert(v >> 0);
    coords[3 * i + 1] = rn_morton3d_invert(v >> 1);
    coords[3 * i + 2] = rn_morton3d_invert(v >> 2);
}

// 16 bytes of bitfield per thread: 128 density cells read as 32 x float4
__global__ void __launch_bounds__(256)
k_packbits(int64_t n_bytes, const float* __restrict__ grid, float thr, uint8_t* __restrict__ bits) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bytes) return;
    const float4* g = reinterpret_cast<const float4*>(grid + 8 * b);
    const float4 lo = g[0], hi = g[1];
    uint8_t v = 0;
    v |= (lo.x > thr) << 0; v |= (lo.y > thr) << 1; v |= (lo.z > thr) << 2; v |= (lo.w > thr) << 3;
    v |= (hi.x > thr) << 4; v |= (hi.y > thr) << 5; v |= (hi.z > thr) << 6; v |= (hi.w > thr) << 7;
    bits[b] = v;
}

// tmp[c, indices] = sigma (networks.py:393-394) with duplicate cells resolved
// by their max, deterministically: sigma >= 0, so the int order of the bits is
// the float order and one integer atomicMax per value suffices
__global__ void __launch_bounds__(256)
k_scatter_max(int64_t n, const int64_t* __restrict__ idx, const float* __restrict__ v,
              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicMax(reinterpret_cast<int*>(out) + idx[i], __float_as_int(fmaxf(v[i], 0.0f)));
}

struct MarkArgs {
    const float* poses;             // (n_cams, 3, 4) c2w, columns right / down / front / eye
    float* const* grids;            // [K] -> (C, G3) density grids
    uint8_t* const* bitfields;      // [K] -> C G3 / 8 bytes
    float* count;                   // (C, G3) share of the cameras that cover the cell
    int32_t* n_culled;              // [C] or NULL
    int n_cams, K, G;
    float fx, fy, cx, cy, w, h, near, scale;
};

// Camera-visibility culling (radnerf.h rn_mark_invisible_cells states the
// operation order).  One thread per Morton cell, a block inside one cascade
// (G^3 is a multiple of 256); the camera index is wave-uniform, so the 12 pose
// floats are uniform loads.  Every camera is visited: the covered count and
// the any-too-near flag both need all of them.  The wave's 64 consecutive
// cells are 8 bitfield bytes: a ballot of the invalid lanes, and lane 8 i
// clears byte i's bits with a plain read-modify-write (no other thread of the
// launch touches that byte).
__global__ void __launch_bounds__(256)
k_mark_invisible(MarkArgs a) {
    const int64_t G3 = (int64_t)a.G * a.G * a.G;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // < C G3 by the grid
    const int c = (int)(e / G3);
    const uint32_t m = (uint32_t)(e - (int64_t)c * G3);
    const float sc = fminf(scalbnf(1.0f, c - 1), a.scale);
    const float hgs = sc / a.G;
    const float gm1 = (float)(a.G - 1);
    const float X0 = (((float)rn_morton3d_invert(m) / gm1) * 2.0f - 1.0f) * (sc - hgs);
    const float X1 = (((float)rn_morton3d_invert(m >> 1) / gm1) * 2.0f - 1.0f) * (sc - hgs);
    const float X2 = (((float)rn_morton3d_invert(m >> 2) / gm1) * 2.0f - 1.0f) * (sc - hgs);
    int n_cov = 0;
    bool near_hit = false;
    for (int cam = 0; cam < a.n_cams; ++cam) {
        const float* P = a.poses + (int64_t)cam * 12;
        const float d0 = X0 - P[3], d1 = X1 - P[7], d2 = X2 - P[11];
        const float xc = (P[0] * d0 + P[4] * d1) + P[8] * d2;
        const float yc = (P[1] * d0 + P[5] * d1) + P[9] * d2;
        const float zc = (P[2] * d0 + P[6] * d1) + P[10] * d2;
        const float px = a.fx * xc + a.cx * zc;
        const float py = a.fy * yc + a.cy * zc;
        const bool in_image = zc > 0.f && px >= 0.f && px < a.w * zc && py >= 0.f && py < a.h * zc;
        n_cov += (in_image && zc >= a.near) ? 1 : 0;
        near_hit = near_hit || (in_image && zc < a.near);
    }
    a.count[e] = (float)n_cov / (float)a.n_cams;
    const bool invalid = !(n_cov > 0 && !near_hit);
    const unsigned long long bal = __ballot(invalid);
    const int lane = rn_lane();
    const uint32_t byte = (uint32_t)(bal >> (lane & 56)) & 0xffu;       // this lane's 8-cell byte
    for (int k = 0; k < a.K; ++k) {
        float* g = a.grids[k] + e;
        const float d = *g;
        *g = invalid ? -1.0f : (d < 0.f ? 0.0f : d);
        if ((lane & 7) == 0 && byte) {
            uint8_t* b = a.bitfields[k] + (e >> 3);
            *b = (uint8_t)(*b & ~byte);
        }
    }
    if (a.n_culled) {
        __shared__ int sN;
        if (threadIdx.x == 0) sN = 0;
        __syncthreads();
        if (lane == 0) atomicAdd(&sN, (int)__popcll(bal));
        __syncthreads();
        if (threadIdx.x == 0 && sN) atomicAdd(a.n_culled + c, sN);
    }
}

}  // namespace

extern "C" {

// ABI history: 2 (round 4) rn_field_bwd_merged takes the page pool of
// fx_mode 4 (binned scatter), its statistics block is named fx_stats;
// rn_grid_bin / rn_grid_sum / rn_grid_binned_fold added.  3 (round 4) the
// fx_stats block grew to 640 B (position-weighted sums wq / we).  4 (round 5)
// binned records are e5m17 (rn_grid_record_encode / _decode), the GbCtl block
// carries a fault word, rn_grid_bin_layout fills 8 values.  5 (round 5) the
// wrap checksums wq / we weight element i by ((i mod 2^24) * 0x9E3779) mod
// 2^32 (a 24-bit multiply), fx_mode 2 refuses grids over 2^24 elements.  6
// (round 5) rn_bwd_plan takes balance_blocks (big chunks a multiple of the
// persistent blocks in number).  7 (round 5) wq / we weight element i by its
// byte offset 4 i; fx_mode 2 takes grids up to 2^28 elements.  8 (round 5)
// rn_bwd_plan can write the level forward's per-position input (prep),
// rn_field_fwd_levels takes prep_ready.  9 (round 6) rn_abi_signatures: the
// per-entry signature table, checked by the binding at load.
int rn_version(void) { return RN_ABI_VERSION; }

const char* rn_abi_signatures(void) { return RN_SIGNATURE_TABLE; }

const char* rn_last_error(void) { return g_err; }

int rn_morton3d(const int32_t* coords, int64_t n, int32_t* indices, void* stream) {
    RN_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return 0;
    RN_CHECK_ARG(coords && indices, "null pointer");
    k_morton3d<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(n, coords, indices);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_morton3d_invert(const int32_t* indices, int64_t n, int32_t* coords, void* stream) {
    RN_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return 0;
    RN_CHECK_ARG(coords && indices, "null pointer");
    k_morton3d_invert<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(n, indices, coords);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_packbits(const float* density_grid, int64_t n_bytes, float density_threshold,
                uint8_t* density_bitfield, void* stream) {
    RN_CHECK_ARG(n_bytes >= 0, "bad size");
    if (n_bytes == 0) return 0;
    RN_CHECK_ARG(density_grid && density_bitfield, "null pointer");
    RN_CHECK_ARG(((uintptr_t)density_grid & 15) == 0, "density_grid must be 16-byte aligned");
    k_packbits<<<nblk(n_bytes, 256), 256, 0, (hipStream_t)stream>>>(n_bytes, density_grid,
                                                                     density_threshold,
                                                                     density_bitfield);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_scatter_max(const int64_t* indices, const float* values, int64_t n, float* out,
                   void* stream) {
    RN_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return 0;
    RN_CHECK_ARG(indices && values && out, "null pointer");
    k_scatter_max<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(n, indices, values, out);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_mark_invisible_cells(const float* poses, int32_t n_cams, float fx, float fy, float cx,
                            float cy, int32_t width, int32_t height, float near_distance,
                            const void* grid_ptrs, const void* bitfield_ptrs, int32_t n_models,
                            int32_t cascades, int32_t grid_size, float scale, float* count_grid,
                            int32_t* n_culled, void* stream) {
    RN_CHECK_ARG(n_models >= 1 && cascades >= 1 && cascades <= 32 && grid_size == 128,
                 "bad sizes (grid_size 128, cascades <= 32)");
    RN_CHECK_ARG(n_cams >= 1 && width >= 1 && height >= 1, "needs a camera and a positive image size");
    RN_CHECK_ARG(poses && grid_ptrs && bitfield_ptrs && count_grid, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n_culled && hipMemsetAsync(n_culled, 0, sizeof(int32_t) * cascades, st) != hipSuccess) {
        rn_set_error("%s: memset failed", __func__);
        return 2;
    }
    MarkArgs a{};
    a.poses = poses; a.grids = (float* const*)grid_ptrs; a.bitfields = (uint8_t* const*)bitfield_ptrs;
    a.count = count_grid; a.n_culled = n_culled;
    a.n_cams = n_cams; a.K = n_models; a.G = grid_size;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.w = (float)width; a.h = (float)height;
    a.near = near_distance; a.scale = scale;
    const int64_t n = (int64_t)cascades * grid_size * grid_size * grid_size;   // a multiple of 256
    k_mark_invisible<<<(int)(n / 256), 256, 0, st>>>(a);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
