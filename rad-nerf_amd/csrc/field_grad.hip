// Epilogues of the merged backward's grid-gradient forms (rn_gradform.h) for
// gfx950: what runs before and after k_field_bwd_merged (field.hip)
// when the hash-grid gradient is accumulated as integers instead of tcnn's
// fp32 atomics (models/networks.py:300-328 -> tinycudann GridEncoding backward).
//
// Work decomposition: grid-stride passes over the samples (k_seed_max) or over
// the gradient table, four elements per thread (k_fx_esum, k_fx_fold,
// k_igrad_to_f32); the per-level bookkeeping is one wave (k_fx_check).
//
// Kernels:
//  * k_seed_max + k_seed_scale: the integer form's scale from the step's seeds.
//  * k_igrad_to_f32: its fold into grid_grad.
//  * k_fx_esum + k_fx_check + k_fx_fold: the fixed-point form's wrap check, redo
//    flag, next scales and fold (k_fx_check also serves the binned form).
// Entries: rn_seed_scale, rn_igrad_to_f32, rn_grid_fx_fold, rn_fx_check_binned.
#include "rn_field.h"
#include "rn_bin.h"
#include "rn_gradform.h"
#pragma clang fp contract(off)

namespace {

// Integer-mode scale: 2^(26 - e) with 2^(e-1) <= M < 2^e, M the largest
// backward seed of the step (|dL/dsigma * sigma|, |dL/drgb|), so a seed-sized
// contribution is ~2^26 units; larger ones carry exactly.
__global__ void __launch_bounds__(256)
k_seed_max(const int32_t* __restrict__ seg_base, const int32_t* __restrict__ seg_count,
           const float* __restrict__ sigma, const float* __restrict__ dsigma,
           const float* __restrict__ drgb, uint32_t* __restrict__ mbits) {
    const int k = blockIdx.y;
    const int64_t base = seg_base[k], n = seg_count[k];
    float mx = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = base + i;
        mx = fmaxf(mx, fabsf(dsigma[s] * sigma[s]));
        mx = fmaxf(mx, fmaxf(fabsf(drgb[3 * s]), fmaxf(fabsf(drgb[3 * s + 1]), fabsf(drgb[3 * s + 2]))));
    }
    mx = rn_wave_max(mx);
    if (rn_lane() == 0 && mx > 0.f && isfinite(mx)) atomicMax(mbits, __float_as_uint(mx));
}

__global__ void k_seed_scale(const uint32_t* __restrict__ mbits, float* __restrict__ scale) {
    const float m = __uint_as_float(*mbits);
    float sc = 1.0f;
    if (m > 0.f) {
        int e;
        frexpf(m, &e);                   // m = f * 2^e, f in [0.5, 1)
        sc = scalbnf(1.0f, max(-100, min(100, 26 - e)));
    }
    *scale = sc;
}

// grid_grad += (carry * 2^32 + lo) / scale; lo = carry = 0 for the next step
__global__ void __launch_bounds__(256)
k_igrad_to_f32(int64_t n, int32_t* __restrict__ lo, int32_t* __restrict__ carry,
               const float* __restrict__ scale, float* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = ((double)carry[i] * 4294967296.0 + (double)lo[i]) / (double)*scale;
    grad[i] += (float)v;
    lo[i] = 0;
    carry[i] = 0;
}

// Exact per-level sum of the int32 entries (int64), for the net-wrap check,
// and the level's largest |entry| in gradient units (the next step's scale
// keeps it in range): from the int32 entries of a fixed-point level, from
// grid_grad for a level that went in as fp32 this step (the first step; an
// upper bound when the caller accumulates several steps into grid_grad).
__global__ void __launch_bounds__(256)
k_fx_esum(GridMeta gm, const float* __restrict__ scale, const int32_t* __restrict__ acc,
          const float* __restrict__ grad, FxStats* __restrict__ st) {
    const int l = blockIdx.y;
    const float sc = scale[l];
    typedef int vi4 __attribute__((ext_vector_type(4)));
    const int64_t e0 = 2 * (int64_t)gm.offset[l], n4 = (2 * (int64_t)gm.hsize[l]) >> 2;
    int64_t s = 0;
    uint64_t ws = 0;                 // sum of entry * fx_weight(element), mod 2^64
    uint32_t mx = 0u;           // fixed point: |int|; fp32 level: |float| bits
    auto uabs = [](int x) { return x < 0 ? 0u - (uint32_t)x : (uint32_t)x; };
    if (sc != 0.f) {
        const vi4* a4 = reinterpret_cast<const vi4*>(acc + e0);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
             i += (int64_t)gridDim.x * blockDim.x) {
            const vi4 v = __builtin_nontemporal_load(a4 + i);
            s += (int64_t)v.x + v.y + v.z + v.w;
            const uint32_t el = (uint32_t)(e0 + 4 * i);
            ws += (uint64_t)((int64_t)v.x * (int64_t)fx_weight(el)) +
                  (uint64_t)((int64_t)v.y * (int64_t)fx_weight(el + 1)) +
                  (uint64_t)((int64_t)v.z * (int64_t)fx_weight(el + 2)) +
                  (uint64_t)((int64_t)v.w * (int64_t)fx_weight(el + 3));
            mx = max(max(mx, max(uabs(v.x), uabs(v.y))), max(uabs(v.z), uabs(v.w)));
        }
    } else {
        const vi4* g4 = reinterpret_cast<const vi4*>(grad + e0);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
             i += (int64_t)gridDim.x * blockDim.x) {
            const vi4 v = __builtin_nontemporal_load(g4 + i);
            mx = max(max(mx, max((uint32_t)v.x & 0x7fffffffu, (uint32_t)v.y & 0x7fffffffu)),
                     max((uint32_t)v.z & 0x7fffffffu, (uint32_t)v.w & 0x7fffffffu));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        ws += __shfl_xor(ws, off);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    }
    // one atomic per block (per-wave atomics on the level words serialised:
    // 107 us for 16k of them)
    __shared__ int64_t sW[4];
    __shared__ uint64_t sWw[4];
    __shared__ uint32_t sM[4];
    const int w = threadIdx.x / RN_WAVE;
    if (rn_lane() == 0) { sW[w] = s; sWw[w] = ws; sM[w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t t = (sW[0] + sW[1]) + (sW[2] + sW[3]);
        const uint64_t tw = (sWw[0] + sWw[1]) + (sWw[2] + sWw[3]);
        if (tw != 0) atomicAdd(reinterpret_cast<unsigned long long*>(st->we + l), tw);
        uint32_t m = max(max(sM[0], sM[1]), max(sM[2], sM[3]));
        if (sc != 0.f) m = __float_as_uint((float)m / sc);     // units -> gradient units
        if (t != 0) atomicAdd(reinterpret_cast<unsigned long long*>(st->esum + l), (unsigned long long)t);
        if (m != 0u && m < 0x7f800000u) atomicMax(st->emax + l, m);
    }
}

// Fixed-point step bookkeeping (one wave): redo flag of this step, the next
// step's per-level scales from this step's largest records, statistics reset.
// Scale 2^(FX_TARGET_BITS - e) with |record| < 2^e: the largest record maps
// to < 2^27 units.  A level whose largest record reached 2^30 units under the
// current scale (8x growth since the step the scale came from), or a
// non-finite one, or whose entries wrapped (entry sum != record sum), sets the
// redo flag: rn_grid_fx_fold then discards the fixed-point sums and the GM_FX_REDO
// launch recomputes the grid gradient in fp32.
// Headroom measured on C3 over 12 Adam steps (tools/fx_diag.py): the largest
// |entry| of a hashed level stays within 2^1.2 of its largest record, so at
// 2^27 units it sits ~2^3 below the int32 range.  A dense (coarse) level's
// entry sums up to hundreds of records, so its scale is also capped by this
// step's largest |entry|: it maps to < 2^29 units (2^2 of headroom for growth;
// the first step's entries are read from the fp32 grid_grad); a dense level
// with no entry measured maps its largest record to < 2^14 units.
// Why these units (round 6; tools/fx_units_probe.py,
// profiles/r06/fxunits/): FusedAdam's eps 1e-15 turns any non-zero gradient
// into an lr-sized step, so an entry below half a unit (flushed to 0) moves
// the update as much as a wrong sign.  C3, 3 Adam steps, largest per-level
// update difference from fp32 (fp32 with the rays reversed: <= 0.07 %):
// 2048 rays 2.66 % at (23, 28, 28) -> 1.14 % at (27, 29, 30); 8192 rays 1.02
// -> 0.38 %; flushed entries 0.031 -> 0.005 %; no step redone in 1,150
// probe and training steps; 1000 training steps end within 0.03 dB of fp32
// either way.  (26, 30, 30) redid one of 1000 training steps (entry cap too
// close to 2^31).
#ifndef FX_TARGET_BITS              // (-D overrides: unit studies, tools/fx_units_probe.py)
#define FX_TARGET_BITS 27
#endif
#ifndef FX_ENTRY_BITS
#define FX_ENTRY_BITS 29
#endif
#define FX_DENSE_FIRST_BITS 14
#ifndef FX_GROWTH_BITS
#define FX_GROWTH_BITS 30
#endif
#define FX_GROWTH_UNITS ((float)(1u << FX_GROWTH_BITS))   // 2^30
// Binned mode (ctl != NULL, rn_grid_binned_fold): records are e5m17 (rn_bin.h),
// summed exactly in int64, so there is no entry cap and no wrap check; the
// largest record maps to < 2^GB_TARGET_BITS = 2^38 units (256x headroom below
// 2^46, the first value e5m17 cannot hold: a record that reaches it sets the
// redo flag -- the bar is exact, every record below it is representable), and
// so does a pool overflow (the walk ran out of pages) or a fault word the bin
// pass set (inputs out of range).
__global__ void __launch_bounds__(64)
k_fx_check(uint32_t hashed_mask, const float* __restrict__ scale_cur,
           float* __restrict__ scale_next, FxStats* __restrict__ stats,
           int32_t* __restrict__ redo, const GbCtl* __restrict__ ctl, uint32_t pool_pages) {
    const int l = threadIdx.x;
    uint32_t* vmax = stats->vmax;
    const bool binned = ctl != nullptr;
    // pool overflow, or inputs the bin pass refused (GbCtl::fault)
    bool bad = binned && l == 0 && (ctl->pool_next > pool_pages || ctl->fault != 0u);
    const float growth = binned ? GB_GROWTH_UNITS : FX_GROWTH_UNITS;
    if (l < RN_L) {
        // net wrap of an int32 entry: the entries' exact sum differs from the
        // records' exact sum (by a multiple of 2^32)
        // (and the position-weighted sums: opposite wraps cancel only in the plain one)
        if (!binned && scale_cur[l] != 0.f &&
            (stats->esum[l] != stats->qsum[l] || stats->we[l] != stats->wq[l]))
            bad = true;
        stats->esum[l] = 0;
        stats->qsum[l] = 0;
        stats->we[l] = 0;
        stats->wq[l] = 0;
        const uint32_t vb = vmax[l];
        const float sc = scale_cur[l];
        const uint32_t em = stats->emax[l];
        float nx = sc;                                   // no records this step: keep
        if (vb >= 0x7f800000u) {                         // inf / NaN record
            nx = 0.f;
            bad = bad || sc != 0.f;
        } else if (vb != 0u) {
            const float v = __uint_as_float(vb);
            bad = bad || (sc != 0.f && v * sc >= growth);
            int e;
            frexpf(v, &e);                               // v < 2^e
            int bits = (binned ? GB_TARGET_BITS : FX_TARGET_BITS) - e;
            if (binned) {
                // int64 sums: no entry cap
            } else if (em != 0u) {                       // the largest entry stays < 2^29 units
                int ee;
                frexpf(__uint_as_float(em), &ee);
                bits = min(bits, FX_ENTRY_BITS - ee);
            } else if (!((hashed_mask >> l) & 1u)) {     // dense level, no entry measured
                bits = FX_DENSE_FIRST_BITS - e;
            }
            nx = scalbnf(1.0f, max(-126, min(126, bits)));
        }
        scale_next[l] = nx;
        vmax[l] = 0u;
        stats->emax[l] = 0u;
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(bad);
    if (l == 0) *redo = b ? 1 : 0;
}

// grid_grad += acc * 2^-e_l over the fixed-point levels' entries (elements
// [e0, e1), 16-B aligned), acc = 0; with the redo flag set the sums are only
// cleared (the fp32 redo adds the step's gradient instead).
__global__ void __launch_bounds__(256)
k_fx_fold(int64_t e0, int64_t e1, GridMeta gm, const float* __restrict__ scale,
          int32_t* __restrict__ acc, float* __restrict__ grad, const int32_t* __restrict__ redo) {
    __shared__ uint32_t sOff[RN_L];
    __shared__ float sInv[RN_L];
    if (threadIdx.x < RN_L) {
        sOff[threadIdx.x] = gm.offset[threadIdx.x];
        const float sc = scale[threadIdx.x];
        sInv[threadIdx.x] = sc != 0.f ? 1.0f / sc : 0.f;     // exact: powers of two
    }
    __syncthreads();
    const bool discard = *redo != 0;
    const int64_t n4 = (e1 - e0) >> 2;
    typedef int vi4 __attribute__((ext_vector_type(4)));
    vi4* a4 = reinterpret_cast<vi4*>(acc + e0);
    float4* g4 = reinterpret_cast<float4*>(grad + e0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        const vi4 v = __builtin_nontemporal_load(a4 + i);
        if ((v.x | v.y | v.z | v.w) == 0) continue;
        __builtin_nontemporal_store(vi4{0, 0, 0, 0}, a4 + i);
        if (discard) continue;
        const uint32_t ent = (uint32_t)((e0 + 4 * i) >> 1);
        int l = 0;
#pragma unroll
        for (int k = 1; k < RN_L; ++k) l = ent >= sOff[k] ? k : l;
        const float inv = sInv[l];
        float4 g = g4[i];
        g.x += (float)v.x * inv; g.y += (float)v.y * inv;
        g.z += (float)v.z * inv; g.w += (float)v.w * inv;
        g4[i] = g;
    }
}

}  // namespace

extern "C" {

int rn_seed_scale(const int32_t* seg_base, const int32_t* seg_count, int32_t n_models,
                  const float* sigma, const float* dL_dsigma, const float* dL_drgb,
                  uint32_t* work, float* scale, void* stream) {
    RN_CHECK_ARG(n_models >= 1, "bad sizes");
    RN_CHECK_ARG(seg_base && seg_count && sigma && dL_dsigma && dL_drgb && work && scale,
                 "null pointer");
    hipStream_t st = (hipStream_t)stream;
    RN_CHECK_HIP(hipMemsetAsync(work, 0, sizeof(uint32_t), st), "memset");
    k_seed_max<<<dim3(256, n_models), 256, 0, st>>>(seg_base, seg_count, sigma, dL_dsigma,
                                                     dL_drgb, work);
    RN_CHECK_LAUNCH();
    k_seed_scale<<<1, 1, 0, st>>>(work, scale);
    RN_CHECK_LAUNCH();
    return 0;
}

int rn_grid_fx_fold(const uint32_t* level_offset, const uint32_t* level_hsize,
                    const uint32_t* level_res, int32_t* fx_acc, const float* fx_scale_cur,
                    float* fx_scale_next, uint32_t* fx_vmax, int32_t* fx_redo, float* grid_grad,
                    void* stream) {
    RN_CHECK_ARG(level_offset && level_hsize && level_res && fx_acc && fx_scale_cur &&
                 fx_scale_next && fx_vmax && fx_redo && grid_grad, "null pointer");
    RN_CHECK_ARG(fx_scale_cur != fx_scale_next, "scale_cur and scale_next must differ");
    GridMeta gm{};
    uint32_t hashed = 0;
    for (int l = 0; l < RN_L; ++l) {
        gm.offset[l] = level_offset[l]; gm.hsize[l] = level_hsize[l]; gm.res[l] = level_res[l];
        const uint64_t r = level_res[l];
        if (r * r * r > (uint64_t)level_hsize[l]) hashed |= 1u << l;
        RN_CHECK_ARG(level_offset[l] % 8 == 0, "level offsets must be multiples of 8 entries");
    }
    hipStream_t st = (hipStream_t)stream;
    FxStats* stats = reinterpret_cast<FxStats*>(fx_vmax);
    k_fx_esum<<<dim3(128, RN_L), 256, 0, st>>>(gm, fx_scale_cur, fx_acc, grid_grad, stats);
    k_fx_check<<<1, 64, 0, st>>>(hashed, fx_scale_cur, fx_scale_next, stats, fx_redo, nullptr, 0u);
    RN_CHECK_LAUNCH();
    {   // every level (dense ones go fixed point from their second step)
        const int64_t e0 = 2 * (int64_t)level_offset[0];
        const int64_t e1 = 2 * ((int64_t)level_offset[RN_L - 1] + level_hsize[RN_L - 1]);
        RN_CHECK_ARG(e1 % 4 == 0, "table size must be a multiple of 2 entries");
        const int64_t n4 = (e1 - e0) / 4;
        const int nb = (int)std::min<int64_t>(2048, (n4 + 255) / 256);
        k_fx_fold<<<nb > 0 ? nb : 1, 256, 0, st>>>(e0, e1, gm, fx_scale_cur, fx_acc, grid_grad,
                                                    fx_redo);
        RN_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"

int rn_fx_check_binned(const float* fx_scale_cur, float* fx_scale_next, uint32_t* fx_stats,
                       int32_t* fx_redo, const void* ctl, uint32_t pool_pages, void* stream) {
    k_fx_check<<<1, 64, 0, (hipStream_t)stream>>>(0u, fx_scale_cur, fx_scale_next,
                                                  reinterpret_cast<FxStats*>(fx_stats), fx_redo,
                                                  (const GbCtl*)ctl, pool_pages);
    RN_CHECK_LAUNCH();
    return 0;
}

extern "C" {

int rn_igrad_to_f32(int64_t n, int32_t* igrad_lo, int32_t* igrad_carry, const float* scale,
                    float* grid_grad, void* stream) {
    RN_CHECK_ARG(n >= 0, "bad size");
    if (n == 0) return 0;
    RN_CHECK_ARG(igrad_lo && igrad_carry && scale && grid_grad, "null pointer");
    k_igrad_to_f32<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(n, igrad_lo, igrad_carry, scale,
                                                                   grid_grad);
    RN_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
