// Validation images (train_ml.py:47-52,238-248): the 8-bit pictures that
// validation_step writes next to its two numbers -- (rgb * 255).astype(uint8),
// depth2img (min-max normalise, colormap) -- and the gate map, on the image
// buffers ImageEvaluator.render_image leaves on the device.
//
// All four are streaming kernels.  A lane takes four consecutive pixels: one
// 16-byte load where the source is dense and aligned (four dword loads
// otherwise), and its 12 output bytes as three dword stores (rn_quantize_u8 is
// per element: four elements, one dword).  The pixels in front of the first
// 4-byte-aligned output address and the n % 4 behind the last whole group are
// written byte by byte by eight lanes of block 0.  Everything is fp32 with
// contraction off, one rounding per operation, so tests/image_out_ref.py's
// numpy restatement gives the same bytes.
#include "rn_common.h"

#include <cmath>

namespace {

constexpr int IO_THREADS = 256;
constexpr int IO_WAVES = IO_THREADS / RN_WAVE;
static_assert(IO_THREADS == 256, "k_colormap_u8 stages one table row per thread");
constexpr int IO_MAX_BLOCKS = RN_METRICS_WORK_BYTES / 8;    // one {min, max} pair per block
constexpr int IO_MAX_MODELS = 16;                           // rn_gate_fwd's bound
constexpr int64_t IO_MAX_N = (int64_t)1 << 40;              // a grid of n / 1024 blocks

// [0, n) as `head` single items, `nq` groups of four from `head` on, and the
// rest (fewer than four) from `tail0` on
struct Split {
    int64_t head, nq, tail0;
};

inline Split split(int64_t n, int64_t head) {
    Split s;
    s.head = head < n ? head : n;
    s.nq = (n - s.head) / 4;
    s.tail0 = s.head + 4 * s.nq;
    return s;
}

inline int grid_for(int64_t nq) {
    const int64_t b = (nq + IO_THREADS - 1) / IO_THREADS;
    return (int)(b < 1 ? 1 : b);
}

// the item of block 0's lanes 0..3 (head) and 4..7 (tail), or -1
__device__ __forceinline__ int64_t edge_item(Split s, int64_t n) {
    if (blockIdx.x != 0 || threadIdx.x >= 8) return -1;
    const int64_t i = threadIdx.x < 4 ? (int64_t)threadIdx.x : s.tail0 + (threadIdx.x - 4);
    if (threadIdx.x < 4) return i < s.head ? i : -1;
    return i < n ? i : -1;
}

// x[(i + k) * stride], k < 4; VEC: stride 1 and x + i on a 16-byte boundary
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ x, int64_t i, int64_t stride,
                                      float (&v)[4]) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(x + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x[(i + k) * stride];
    }
}

// NaN -> 0, clamp to [0, 255], truncate
__device__ __forceinline__ uint32_t to_u8(float y) {
    y = y != y ? 0.0f : y;
    y = fminf(fmaxf(y, 0.0f), 255.0f);
    return (uint32_t)y;
}

// four 24-bit pixels (channel 0 in the low byte) -> 12 bytes at a dword boundary
__device__ __forceinline__ void store_rgb4(uint8_t* __restrict__ dst, int64_t pix,
                                           const uint32_t (&c)[4]) {
    uint32_t* p = reinterpret_cast<uint32_t*>(dst + 3 * pix);
    p[0] = c[0] | (c[1] << 24);
    p[1] = (c[1] >> 8) | (c[2] << 16);
    p[2] = (c[2] >> 16) | (c[3] << 8);
}

__device__ __forceinline__ void store_rgb1(uint8_t* __restrict__ dst, int64_t pix, uint32_t c) {
    dst[3 * pix + 0] = (uint8_t)(c & 0xff);
    dst[3 * pix + 1] = (uint8_t)((c >> 8) & 0xff);
    dst[3 * pix + 2] = (uint8_t)(c >> 16);
}

// ---- min / max over the finite values ------------------------------------------
struct MinMax {
    float mn, mx;
    __device__ __forceinline__ void take(float v) {
        if (isfinite(v)) {
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    __device__ __forceinline__ void merge(float omn, float omx) {
        mn = fminf(mn, omn);
        mx = fmaxf(mx, omx);
    }
};

template <bool VEC>
__global__ void __launch_bounds__(IO_THREADS)
k_minmax_partials(const float* __restrict__ x, int64_t n, int64_t stride, Split s,
                  float2* __restrict__ work) {
    __shared__ float2 wred[IO_WAVES];
    MinMax m = {__builtin_inff(), -__builtin_inff()};
    const int64_t step = (int64_t)gridDim.x * IO_THREADS;
    for (int64_t q = (int64_t)blockIdx.x * IO_THREADS + threadIdx.x; q < s.nq; q += step) {
        float v[4];
        load4<VEC>(x, s.head + 4 * q, stride, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) m.take(v[k]);
    }
    const int64_t e = edge_item(s, n);
    if (e >= 0) m.take(x[e * stride]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        m.merge(__shfl_xor(m.mn, off), __shfl_xor(m.mx, off));
    if (rn_lane() == 0) wred[threadIdx.x / RN_WAVE] = make_float2(m.mn, m.mx);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < IO_WAVES; ++w) m.merge(wred[w].x, wred[w].y);
        work[blockIdx.x] = make_float2(m.mn, m.mx);
    }
}

// out2 = {min, max} of the partials, thread t over its strided share, then a
// fixed tree; {0, 0} when no finite value was seen (also n_part == 0)
__global__ void __launch_bounds__(IO_THREADS)
k_minmax_final(const float2* __restrict__ work, int n_part, float* __restrict__ out2) {
    __shared__ float2 red[IO_THREADS];
    MinMax m = {__builtin_inff(), -__builtin_inff()};
    for (int i = threadIdx.x; i < n_part; i += IO_THREADS) m.merge(work[i].x, work[i].y);
    red[threadIdx.x] = make_float2(m.mn, m.mx);
    __syncthreads();
    for (int off = IO_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float2 a = red[threadIdx.x], b = red[threadIdx.x + off];
            red[threadIdx.x] = make_float2(fminf(a.x, b.x), fmaxf(a.y, b.y));
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool any = red[0].x <= red[0].y;
        out2[0] = any ? red[0].x : 0.0f;
        out2[1] = any ? red[0].y : 0.0f;
    }
}

// ---- (x * 255).astype(uint8) ----------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(IO_THREADS)
k_quantize_u8(const float* __restrict__ src, int64_t n, Split s, uint8_t* __restrict__ dst) {
    const int64_t q = (int64_t)blockIdx.x * IO_THREADS + threadIdx.x;
    if (q < s.nq) {
        const int64_t i = s.head + 4 * q;
        float v[4];
        load4<VEC>(src, i, 1, v);
        *reinterpret_cast<uint32_t*>(dst + i) = to_u8(v[0] * 255.0f) | (to_u8(v[1] * 255.0f) << 8) |
                                                (to_u8(v[2] * 255.0f) << 16) |
                                                (to_u8(v[3] * 255.0f) << 24);
    }
    const int64_t e = edge_item(s, n);
    if (e >= 0) dst[e] = (uint8_t)to_u8(src[e] * 255.0f);
}

// ---- depth2img -------------------------------------------------------------------
__device__ __forceinline__ uint32_t colormap_index(float x, float mn, float den) {
    if (!(den > 0.0f) || !isfinite(x)) return 0;
    const float t = (x - mn) / den;
    return to_u8(t * 255.0f);
}

template <bool VEC>
__global__ void __launch_bounds__(IO_THREADS)
k_colormap_u8(const float* __restrict__ x, int64_t n, int64_t stride, Split s,
              const float* __restrict__ range2, const uint8_t* __restrict__ lut, int swap_rb,
              uint8_t* __restrict__ dst) {
    // the table as 256 packed pixels, channel 0 of the output in the low byte
    __shared__ uint32_t slut[256];
    {
        const int t = threadIdx.x;
        const uint32_t a = lut[3 * t + (swap_rb ? 2 : 0)], b = lut[3 * t + 1],
                       c = lut[3 * t + (swap_rb ? 0 : 2)];
        slut[t] = a | (b << 8) | (c << 16);
    }
    __syncthreads();
    const float mn = range2[0], den = range2[1] - mn;
    const int64_t q = (int64_t)blockIdx.x * IO_THREADS + threadIdx.x;
    if (q < s.nq) {
        const int64_t i = s.head + 4 * q;
        float v[4];
        load4<VEC>(x, i, stride, v);
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = slut[colormap_index(v[k], mn, den)];
        store_rgb4(dst, i, c);
    }
    const int64_t e = edge_item(s, n);
    if (e >= 0) store_rgb1(dst, e, slut[colormap_index(x[e * stride], mn, den)]);
}

// ---- gate map ----------------------------------------------------------------------
// One pixel's K gates arrive one after the other (k ascending): the blend
// acc_c = g_0 p_0c, then acc_c + g_k p_kc, and the first maximal gate.
struct GatePixel {
    float a0, a1, a2, best;
    int k, arg;
    __device__ __forceinline__ void reset() {
        a0 = a1 = a2 = 0.0f;
        best = -__builtin_inff();
        k = arg = 0;
    }
    __device__ __forceinline__ void take(float g, const float (*pal)[3]) {
        const float p0 = g * pal[k][0], p1 = g * pal[k][1], p2 = g * pal[k][2];
        a0 = k == 0 ? p0 : a0 + p0;
        a1 = k == 0 ? p1 : a1 + p1;
        a2 = k == 0 ? p2 : a2 + p2;
        if (g > best) {             // a NaN never wins, a tie keeps the first
            best = g;
            arg = k;
        }
        ++k;
    }
    __device__ __forceinline__ uint32_t colour(int hard, const uint32_t* packed) const {
        if (hard) return packed[arg];
        return to_u8(a0 + 0.5f) | (to_u8(a1 + 0.5f) << 8) | (to_u8(a2 + 0.5f) << 16);
    }
};

template <bool VEC>
__global__ void __launch_bounds__(IO_THREADS)
k_gate_map_u8(const float* __restrict__ gate, int64_t n, int K, Split s,
              const uint8_t* __restrict__ palette, int hard, uint8_t* __restrict__ dst) {
    __shared__ float pal[IO_MAX_MODELS][3];
    __shared__ uint32_t packed[IO_MAX_MODELS];
    if ((int)threadIdx.x < K) {
        const int t = threadIdx.x;
        const uint32_t a = palette[3 * t], b = palette[3 * t + 1], c = palette[3 * t + 2];
        pal[t][0] = (float)a;
        pal[t][1] = (float)b;
        pal[t][2] = (float)c;
        packed[t] = a | (b << 8) | (c << 16);
    }
    __syncthreads();
    GatePixel px;
    const int64_t q = (int64_t)blockIdx.x * IO_THREADS + threadIdx.x;
    if (q < s.nq) {
        // the lane's 4 K floats are contiguous: K loads of four, pixel after pixel
        const int64_t i = s.head + 4 * q;
        const float* g = gate + i * K;
        uint32_t c[4] = {0, 0, 0, 0};
        int p = 0;
        px.reset();
        for (int j = 0; j < K; ++j) {
            float v[4];
            load4<VEC>(g, 4 * j, 1, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                px.take(v[e], pal);
                if (px.k == K) {
                    const uint32_t col = px.colour(hard, packed);
                    c[0] = p == 0 ? col : c[0];
                    c[1] = p == 1 ? col : c[1];
                    c[2] = p == 2 ? col : c[2];
                    c[3] = p == 3 ? col : c[3];
                    ++p;
                    px.reset();
                }
            }
        }
        store_rgb4(dst, i, c);
    }
    const int64_t e = edge_item(s, n);
    if (e >= 0) {
        px.reset();
        for (int k = 0; k < K; ++k) px.take(gate[e * K + k], pal);
        store_rgb1(dst, e, px.colour(hard, packed));
    }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// pixels in front of the first dword boundary of a 3-byte-per-pixel output:
// dst + 3 h = 0 (mod 4) for h = dst mod 4
inline int64_t rgb_head(const uint8_t* dst) { return (int64_t)((uintptr_t)dst & 3); }

}  // namespace

extern "C" {

int rn_minmax_finite(const float* x, int64_t n, int64_t stride, void* work, float* out2,
                     void* stream) {
    RN_CHECK_ARG(n >= 0 && n <= IO_MAX_N, "bad sizes");
    RN_CHECK_ARG(stride >= 1, "stride must be at least 1 (in elements)");
    RN_CHECK_ARG(n == 0 || stride <= (INT64_MAX >> 3) / n, "n * stride is out of range");
    RN_CHECK_ARG(out2 && (n == 0 || (x && work)), "null pointer");
    RN_CHECK_ARG(aligned(x, 4) && aligned(work, 8) && aligned(out2, 4), "misaligned pointer");
    int blocks = 0;
    if (n > 0) {
        // dense: the elements in front of the first 16-byte boundary go to the head
        const bool vec = stride == 1;
        const Split s = split(n, vec ? (int64_t)((4 - (((uintptr_t)x >> 2) & 3)) & 3) : 0);
        // 4 groups per thread and pass before the grid is capped
        const int64_t nb = (s.nq + 4 * IO_THREADS - 1) / (4 * IO_THREADS);
        blocks = (int)(nb < 1 ? 1 : (nb < IO_MAX_BLOCKS ? nb : IO_MAX_BLOCKS));
        if (vec)
            k_minmax_partials<true><<<blocks, IO_THREADS, 0, (hipStream_t)stream>>>(
                x, n, stride, s, (float2*)work);
        else
            k_minmax_partials<false><<<blocks, IO_THREADS, 0, (hipStream_t)stream>>>(
                x, n, stride, s, (float2*)work);
    }
    k_minmax_final<<<1, IO_THREADS, 0, (hipStream_t)stream>>>((const float2*)work, blocks, out2);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_quantize_u8(const float* src, int64_t n, uint8_t* dst, void* stream) {
    RN_CHECK_ARG(n >= 0 && n <= IO_MAX_N, "bad sizes");
    if (n == 0) return 0;
    RN_CHECK_ARG(src && dst, "null pointer");
    RN_CHECK_ARG(aligned(src, 4), "misaligned pointer");
    // one byte per element: the head runs up to dst's first dword boundary
    const Split s = split(n, (int64_t)((4 - ((uintptr_t)dst & 3)) & 3));
    if (aligned(src + s.head, 16))
        k_quantize_u8<true><<<grid_for(s.nq), IO_THREADS, 0, (hipStream_t)stream>>>(src, n, s, dst);
    else
        k_quantize_u8<false><<<grid_for(s.nq), IO_THREADS, 0, (hipStream_t)stream>>>(src, n, s,
                                                                                     dst);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_colormap_u8(const float* x, int64_t n, int64_t stride, const float* range2,
                   const uint8_t* lut, int32_t swap_rb, uint8_t* dst, void* stream) {
    RN_CHECK_ARG(n >= 0 && n <= IO_MAX_N, "bad sizes");
    RN_CHECK_ARG(stride >= 1, "stride must be at least 1 (in elements)");
    RN_CHECK_ARG(n == 0 || stride <= (INT64_MAX >> 3) / n, "n * stride is out of range");
    if (n == 0) return 0;
    RN_CHECK_ARG(x && range2 && lut && dst, "null pointer");
    RN_CHECK_ARG(aligned(x, 4) && aligned(range2, 4), "misaligned pointer");
    const Split s = split(n, rgb_head(dst));
    if (stride == 1 && aligned(x + s.head, 16))
        k_colormap_u8<true><<<grid_for(s.nq), IO_THREADS, 0, (hipStream_t)stream>>>(
            x, n, stride, s, range2, lut, swap_rb, dst);
    else
        k_colormap_u8<false><<<grid_for(s.nq), IO_THREADS, 0, (hipStream_t)stream>>>(
            x, n, stride, s, range2, lut, swap_rb, dst);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_gate_map_u8(const float* gate, int64_t n, int32_t n_models, const uint8_t* palette,
                   int32_t hard, uint8_t* dst, void* stream) {
    RN_CHECK_ARG(n >= 0 && n <= IO_MAX_N, "bad sizes");
    RN_CHECK_ARG(n_models >= 1 && n_models <= IO_MAX_MODELS, "n_models must be 1..16");
    if (n == 0) return 0;
    RN_CHECK_ARG(gate && palette && dst, "null pointer");
    RN_CHECK_ARG(aligned(gate, 4), "misaligned pointer");
    const Split s = split(n, rgb_head(dst));
    // a group's 4 K floats start 16 K bytes after the one before: all aligned or none
    if (aligned(gate + s.head * n_models, 16))
        k_gate_map_u8<true><<<grid_for(s.nq), IO_THREADS, 0, (hipStream_t)stream>>>(
            gate, n, n_models, s, palette, hard, dst);
    else
        k_gate_map_u8<false><<<grid_for(s.nq), IO_THREADS, 0, (hipStream_t)stream>>>(
            gate, n, n_models, s, palette, hard, dst);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
