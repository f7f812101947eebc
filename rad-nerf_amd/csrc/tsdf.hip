// TSDF fusion for gfx950 (radnerf_amd/tsdf.py): rendered depth images folded
// into a truncated signed distance volume, and vertex colours read back from
// the volume's colour lattice.  include/radnerf.h (rn_tsdf_integrate,
// rn_lattice_colors) states the operation order; tests/tsdf_ref.py restates it
// in numpy.
//  * k_tsdf_integrate: one thread per lattice point, x fastest, so a wave's 64
//    points read and write 256 contiguous bytes of phi and of w (768 of rgb)
//    and project to neighbouring pixels of every camera.  The cameras of the
//    batch are visited in ascending order with the point's state in registers:
//    the volume is read once and written once per launch, and only where some
//    camera observed the point.  The camera index is wave-uniform, so the 12
//    pose floats are uniform loads.  No atomic: a point has one owner.
//  * k_lattice_colors: one thread per vertex, the 8 corners of its cell.
// The valid-aware surface nets that mesh a volume (rn_surface_count_valid /
// rn_surface_emit_valid) are mesh.hip's kernels under a template parameter.
#include "rn_common.h"
#pragma clang fp contract(off)

namespace {

struct TsdfArgs {
    uint32_t px, py, n_pts;         // points per row / per column; points (< 2^31)
    float lo[3], step[3];
    const float* poses;             // (n_cams, 3, 4) c2w, columns right / down / front / eye
    int n_cams, W, H;
    int64_t n_pix;                  // W H
    float fx, fy, cx, cy, wf, hf;
    const float* dirs;              // (n_pix, 3)
    const float* depth;             // (n_cams, n_pix)
    const float* opacity;           // (n_cams, n_pix)
    const float* rgb;               // (n_cams, n_pix, 3) or null
    float trunc, near, opacity_min;
    int carve;
    float* phi; float* w;           // (points)
    float* vrgb; float* wc;         // (points, 3), (points), or null
};

template <bool COLOR>
__global__ void __launch_bounds__(256)
k_tsdf_integrate(TsdfArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.n_pts) return;
    const uint32_t row = p / a.px, pi = p - row * a.px;
    const uint32_t pk = row / a.py, pj = row - pk * a.py;
    const float X0 = a.lo[0] + (float)pi * a.step[0];
    const float X1 = a.lo[1] + (float)pj * a.step[1];
    const float X2 = a.lo[2] + (float)pk * a.step[2];
    float phi = a.phi[p], w = a.w[p];
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, wc = 0.f;
    if (COLOR) {
        c0 = a.vrgb[3 * (size_t)p]; c1 = a.vrgb[3 * (size_t)p + 1]; c2 = a.vrgb[3 * (size_t)p + 2];
        wc = a.wc[p];
    }
    bool seen = false, coloured = false;
    for (int cam = 0; cam < a.n_cams; ++cam) {
        const float* P = a.poses + (int64_t)cam * 12;
        const float d0 = X0 - P[3], d1 = X1 - P[7], d2 = X2 - P[11];
        const float xc = (P[0] * d0 + P[4] * d1) + P[8] * d2;
        const float yc = (P[1] * d0 + P[5] * d1) + P[9] * d2;
        const float zc = (P[2] * d0 + P[6] * d1) + P[10] * d2;
        if (!(zc >= a.near)) continue;
        const float u = floorf((a.fx * xc) / zc + a.cx);
        const float v = floorf((a.fy * yc) / zc + a.cy);
        if (!(u >= 0.f && u < a.wf && v >= 0.f && v < a.hf)) continue;      // NaN: outside
        const int64_t pix = (int64_t)(int)v * a.W + (int)u;                // < n_pix by the test
        const int64_t at = (int64_t)cam * a.n_pix + pix;
        const float o = a.opacity[at];
        float obs = -1.0f;
        bool colour = false;
        if (!(o >= a.opacity_min)) {                                        // a miss (NaN too)
            if (!a.carve) continue;
        } else {
            const float d = a.depth[at] / o;
            const float e0 = a.dirs[3 * pix], e1 = a.dirs[3 * pix + 1], e2 = a.dirs[3 * pix + 2];
            const float n2 = (e0 * e0 + e1 * e1) + e2 * e2;
            const float tv = ((xc * e0 + yc * e1) + zc * e2) / n2;
            const float s = (tv - d) * sqrtf(n2);
            if (!(s <= a.trunc)) continue;                                  // hidden (NaN too)
            obs = fmaxf(s / a.trunc, -1.0f);
            colour = s >= -a.trunc;
        }
        phi = (phi * w + obs) / (w + 1.0f);
        w = w + 1.0f;
        seen = true;
        if (COLOR && colour) {
            const float* q = a.rgb + 3 * at;
            const float wn = wc + 1.0f;
            c0 = (c0 * wc + q[0]) / wn;
            c1 = (c1 * wc + q[1]) / wn;
            c2 = (c2 * wc + q[2]) / wn;
            wc = wn;
            coloured = true;
        }
    }
    if (seen) { a.phi[p] = phi; a.w[p] = w; }
    if (COLOR && coloured) {
        a.vrgb[3 * (size_t)p] = c0; a.vrgb[3 * (size_t)p + 1] = c1; a.vrgb[3 * (size_t)p + 2] = c2;
        a.wc[p] = wc;
    }
}

struct ColorArgs {
    const float* vertices;          // (n, 3)
    int64_t n;
    uint32_t nx, ny, nz, px, py;
    float lo[3], step[3];
    const float* vrgb; const float* wc;
    uint8_t* out;                   // (n, 3)
};

// NaN -> 0, clamp to [0, 255], truncate: rn_quantize_u8's rule (imageout.hip)
__device__ __forceinline__ uint8_t ts_u8(float y) {
    y = y != y ? 0.0f : y;
    y = fminf(fmaxf(y, 0.0f), 255.0f);
    return (uint8_t)(uint32_t)y;
}

__global__ void __launch_bounds__(256)
k_lattice_colors(ColorArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t n[3] = {a.nx, a.ny, a.nz};
    uint32_t c[3];
    float f[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float g = (a.vertices[3 * i + d] - a.lo[d]) / a.step[d];
        const float cf = fminf(fmaxf(floorf(g), 0.0f), (float)(n[d] - 1));   // NaN -> 0
        c[d] = (uint32_t)cf;
        f[d] = fminf(fmaxf(g - cf, 0.0f), 1.0f);                            // NaN -> 0
    }
    float sw = 0.f, acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t x = c[0] + (q & 1), y = c[1] + (q >> 1 & 1), z = c[2] + (q >> 2 & 1);
        const size_t at = x + (size_t)a.px * (y + (size_t)a.py * z);
        const float wx = (q & 1) ? f[0] : 1.0f - f[0];
        const float wy = (q & 2) ? f[1] : 1.0f - f[1];
        const float wz = (q & 4) ? f[2] : 1.0f - f[2];
        const float t = (wx * wy) * wz;
        if (a.wc[at] > 0.f) {
            sw = sw + t;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = acc[k] + t * a.vrgb[3 * at + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        a.out[3 * i + k] = ts_u8((sw > 0.f ? acc[k] / sw : 0.0f) * 255.0f);
}

// sizes of a lattice; status 1 for a bad one
int ts_lattice(const char* who, int32_t nx, int32_t ny, int32_t nz, int64_t* n_pts) {
    RN_CHECK_ARG_AS(who, nx >= 1 && ny >= 1 && nz >= 1, "bad sizes (cells per axis >= 1)");
    *n_pts = ((int64_t)nx + 1) * ((int64_t)ny + 1) * ((int64_t)nz + 1);
    RN_CHECK_ARG_AS(who, *n_pts < ((int64_t)1 << 31), "lattice of 2^31 points or more");
    return 0;
}

}  // namespace

extern "C" {

int rn_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* lo, const float* step,
                      const float* poses, int32_t n_cams, float fx, float fy, float cx, float cy,
                      int32_t width, int32_t height, const float* directions, const float* depth,
                      const float* opacity, const float* rgb, float trunc, float near_distance,
                      float opacity_min, int32_t carve, float* phi, float* w, float* vol_rgb,
                      float* wc, void* stream) {
    int64_t n_pts = 0;
    if (ts_lattice(__func__, nx, ny, nz, &n_pts)) return 1;
    RN_CHECK_ARG(n_cams >= 0 && width >= 1 && height >= 1 &&
                 (int64_t)width * height < ((int64_t)1 << 31),
                 "bad sizes (n_cams >= 0, a positive image of fewer than 2^31 pixels)");
    RN_CHECK_ARG(trunc > 0.f && near_distance >= 0.f && opacity_min > 0.f,
                 "needs trunc > 0, near_distance >= 0, opacity_min > 0");
    RN_CHECK_ARG(lo && step && phi && w, "null pointer");
    RN_CHECK_ARG((vol_rgb != nullptr) == (wc != nullptr), "vol_rgb and wc go together");
    RN_CHECK_ARG(!rgb || vol_rgb, "rgb images need a colour volume (vol_rgb, wc)");
    if (n_cams == 0) return 0;
    RN_CHECK_ARG(poses && directions && depth && opacity, "null pointer");
    TsdfArgs a{};
    a.px = nx + 1; a.py = ny + 1; a.n_pts = (uint32_t)n_pts;
    for (int d = 0; d < 3; ++d) { a.lo[d] = lo[d]; a.step[d] = step[d]; }
    a.poses = poses; a.n_cams = n_cams; a.W = width; a.H = height;
    a.n_pix = (int64_t)width * height;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.wf = (float)width; a.hf = (float)height;
    a.dirs = directions; a.depth = depth; a.opacity = opacity; a.rgb = rgb;
    a.trunc = trunc; a.near = near_distance; a.opacity_min = opacity_min; a.carve = carve != 0;
    a.phi = phi; a.w = w; a.vrgb = vol_rgb; a.wc = wc;
    const uint32_t blocks = (uint32_t)((n_pts + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (rgb) k_tsdf_integrate<true><<<blocks, 256, 0, st>>>(a);
    else k_tsdf_integrate<false><<<blocks, 256, 0, st>>>(a);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_lattice_colors(const float* vertices, int64_t n_vertices, int32_t nx, int32_t ny,
                      int32_t nz, const float* lo, const float* step, const float* vol_rgb,
                      const float* wc, uint8_t* colors, void* stream) {
    int64_t n_pts = 0;
    if (ts_lattice(__func__, nx, ny, nz, &n_pts)) return 1;
    RN_CHECK_ARG(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31), "bad size (vertices < 2^31)");
    if (n_vertices == 0) return 0;
    RN_CHECK_ARG(vertices && lo && step && vol_rgb && wc && colors, "null pointer");
    ColorArgs a{};
    a.vertices = vertices; a.n = n_vertices;
    a.nx = nx; a.ny = ny; a.nz = nz; a.px = nx + 1; a.py = ny + 1;
    for (int d = 0; d < 3; ++d) { a.lo[d] = lo[d]; a.step[d] = step[d]; }
    a.vrgb = vol_rgb; a.wc = wc; a.out = colors;
    k_lattice_colors<<<(uint32_t)((n_vertices + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
