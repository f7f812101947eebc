// The forms in which the merged backward accumulates the hash-grid gradient
// (GM_*) and their argument blocks, shared by field.hip (k_field_bwd_merged's
// row-lane walk issues them) and field_grad.hip (their epilogue kernels: the
// integer form's scale and fold, the fixed-point form's checks and fold).
#pragma once
#include "rn_field.h"
#include "rn_bin.h"
#pragma clang fp contract(off)

namespace {

// How the merged backward accumulates the grid gradient: k_field_bwd_merged's
// and the walk's GM template argument.  rn_field_bwd_merged's public fx_mode
// takes the same values (0 and 2-5; GM_INT is selected by igrad_lo), and
// fused.py names them alike.
enum : int {
    GM_F32 = 0,        // fp32 atomics
    GM_INT = 1,        // exact integer with carries (IntGrad)
    GM_FX = 2,         // fixed point for the levels with a scale (FxGrad)
    GM_FX_REDO = 3,    // fp32 redo of a flagged fixed-point / binned step
    GM_BIN = 4,        // binned: page records (rn_bin.h)
    GM_BIN_F32 = 5,    // binned, the even streams' levels (0-7) by fp32 atomics
};
// has per-level scales (FxGrad::scale; a zero scale = fp32 atomics for the level)
constexpr bool gm_has_scales(int gm) { return gm >= GM_FX; }
// appends page records to the pool instead of issuing atomics
constexpr bool gm_pages(int gm) { return gm == GM_BIN || gm == GM_BIN_F32; }
// the even streams are fp32 at compile time (no page code for them)
constexpr bool gm_even_f32(int gm) { return gm == GM_BIN_F32; }

// Exact integer accumulation of the grid gradient (IG mode).  Each record
// value v becomes q = rint(v * 2^scale_exp) (int64), added as a 32-bit low
// word with a returning atomic; the high word plus any signed overflow of the
// low word (read from the returned old value) goes to a parallel carry array,
// so every entry holds carry * 2^32 + low exactly: sums are order-independent
// (bitwise reproducible) and u32 atomics run 28 % faster than f32 at the
// memory side (profiles/r01/atomic_probe.json).  A carry add is rare.
struct IntGrad {
    __amdgpu_buffer_rsrc_t lo, carry;   // int32 [entries][2] each (built in the kernel)
    float scale;                        // 2^scale_exp (loaded from scale_ptr)
    int32_t* lo_ptr; int32_t* carry_ptr; const float* scale_ptr;
    uint32_t bytes;
    __amdgpu_buffer_rsrc_t fx;          // fixed-point mode (GM_FX): FxGrad::acc
    // binned mode (GM_BIN, rn_bin.h): the page pool the walk appends to
    GbCtl* ctl; uint32_t* page_meta; uint64_t* pages; uint32_t pool_pages;
};

// Fixed-point accumulation of the hashed levels' grid gradient (GM_FX, the
// default of the merged backward).  A record v of level l is added as the
// int32 rint(v * 2^e_l) with a NON-returning u32 atomic into `acc` (same
// layout as grid_grad): the memory side serves u32 adds at 26.6 G requests/s
// against 20.9 for f32 (profiles/r01/atomic_probe.json), and the sums are
// exact, so these levels' gradients are bitwise reproducible.  e_l comes from
// the previous step's largest record of the level (rn_grid_fx_fold): that
// record maps to < 2^27 units (2^23 until round 6; FX_TARGET_BITS, field_grad.hip),
// leaving 2^4 max-size records of headroom per entry (an entry of a hashed
// level takes ~77 records per C3 step, of mixed sign, and its largest sum
// stays within 2^1.2 of the largest record).  The kernel records this step's
// largest |record| per level; when it reaches 2^30 units (8x growth) or is not
// finite, rn_grid_fx_fold discards the fixed-point sums and the GM_FX_REDO launch
// redoes the grid scatter in fp32.
// The first step of a workspace (scale 0) uses fp32 atomics and measures the
// records; the dense levels (few requests, but entries that sum hundreds of
// records) go fixed point from then on with a scale capped by their largest
// entry (k_fx_check).
// An int32 entry can still wrap with every record under 2^30 units (many
// same-sign records on one entry); the kernel therefore also sums each
// level's integer records exactly (int64), and rn_grid_fx_fold sums the
// level's int32 entries exactly: a wrapped entry makes the two differ by a
// multiple of 2^32, which sets the redo flag too.  (A float sum of the
// records is not enough: its rounding reached 2^31 on trained grids.)
struct FxStats {           // rn_grid_fx_fold / rn_field_bwd_merged fx_stats block
    uint32_t vmax[RN_L];   // largest |record| this step (float bits, atomicMax)
    uint32_t emax[RN_L];   // largest |entry| this step, gradient units (float bits; rn_grid_fx_fold)
    int64_t qsum[RN_L];    // sum of the issued integer records
    int64_t esum[RN_L];    // sum of the int32 entries (rn_grid_fx_fold)
    uint64_t wq[RN_L];     // sum of record * fx_weight(element), mod 2^64
    uint64_t we[RN_L];     // sum of entry * fx_weight(element), mod 2^64 (rn_grid_fx_fold)
};
static_assert(sizeof(FxStats) == RN_FX_STATS_BYTES, "FxStats layout (include/radnerf.h)");

// weight of grid-gradient element i (an int32 of the fixed-point table) in the
// position-weighted checksums: its byte offset 4 i, which the walk's issue
// already holds (no multiply on the issue path).  Wraps of +-2^32 on two
// different elements a, b move the weighted sum by 2^34 (a - b) mod 2^64,
// which is 0 only for a = b mod 2^30: never on a table of at most 2^28
// elements (rn_field_bwd_merged refuses fixed point for larger ones).  (Any
// injective weight is linear in the same way for three or more wraps: round
// 5's odd multiplier, (i mod 2^24) * 0x9E3779, cancelled exactly when
// sum(+-i) = 0 mod 2^32, like this one.)  The weights are < 2^30, so the
// walk adds q * w with one signed 32 x 32 -> 64 mad.
__host__ __device__ __forceinline__ uint32_t fx_weight(uint32_t i) { return 4u * i; }

struct FxGrad {
    int32_t* acc;              // int32 [entries][2]
    const float* scale;        // [RN_L] 2^e_l, 0 = fp32 atomics for the level
    uint32_t* vmax;            // FxStats::vmax
    int64_t* qsum;             // FxStats::qsum
    uint64_t* wq;              // FxStats::wq
    const int32_t* redo;       // GM_FX_REDO: the launch runs only when *redo != 0
    __amdgpu_buffer_rsrc_t rs; // over acc (built in the kernel)
};

}  // namespace
