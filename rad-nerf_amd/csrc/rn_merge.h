// What the chunk plan hands to the merged kernels: the plan's arrays
// (MergeArgs) and the chunk descriptor's layout.  Written by k_bwd_chunks
// (field_plan.hip), read by k_field_fwd_merged (field_fwd_merged.hip) and
// k_field_bwd_merged (field.hip).
#pragma once
#include <stdint.h>

#define MB_KMAX 8          // sub-NeRFs a plan (and the merged kernels) can hold
#define CH_DESC 20         // chunk descriptor ints (80 B, 16-B aligned)

// Chunk descriptor: the chunk's rays [r0, r1), two spare words, then per model
// k the first sample and the sample count of the chunk's rays.
constexpr int CH_R0 = 0, CH_R1 = 1;
constexpr int ch_first(int k) { return 4 + k; }
constexpr int ch_count(int k) { return 4 + MB_KMAX + k; }
static_assert(ch_count(MB_KMAX - 1) < CH_DESC && CH_DESC % 4 == 0, "chunk descriptor layout");

namespace {

struct MergeArgs {
    const int32_t* mstart;   // [B + 1] first merged position of ray r; [B] = total
    const int32_t* perm;     // [total] merged position -> sample index
    const int32_t* desc;     // [n_chunks][CH_DESC] chunk descriptors (above)
    int32_t* queue;          // [0] bwd ticket, [1] n_chunks, [2] fwd ticket (rn_bwd_plan)
    float* scratch;          // [gridDim.x][rows_cap][MB_ROW]
    float* park;             // [gridDim.x][K][BWD_WAVES][32][64]
    int32_t n_rays, n_models, rows_cap;
};

}  // namespace
