/*
 * radnerf.h — C ABI of librn.so, the MI355X (gfx950) Rad-NeRF hot path.
 *
 * Every entry point takes plain device pointers + sizes + a hipStream_t passed
 * as `void*`, launches asynchronously on that stream and returns
 *   0 = ok, 1 = invalid argument, 2 = launch failure
 * (rn_last_error() returns a thread-local message).  No torch types appear in
 * any signature.  Each function cites the reference interface it replaces
 * (paths relative to thu-nics/Rad-NeRF).  The Python binding that mirrors the
 * reference's `vren` module lives in rad-nerf_amd/radnerf_amd/vren.py; see
 * INTEGRATION.md for the ctypes/pybind stubs a maintainer would add.
 */
#ifndef RADNERF_H
#define RADNERF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RN_ABI_VERSION 9   /* rn_version(): bumped on every incompatible ABI change */
#define RN_FX_STATS_BYTES 640   /* the fx_stats block of rn_field_bwd_merged / rn_grid_fx_fold */
int rn_version(void);
const char* rn_last_error(void);
/* the signature of every rn_* entry of this header, as the library was built:
 * "name:codes;..." with one code per parameter (p pointer, i int32, l int64,
 * u uint64, f float, d double), generated from this file at build time
 * (csrc/gen_sig.py).  A binding compares it with its own argument lists and
 * refuses a library built from another revision of the header. */
const char* rn_abi_signatures(void);
/* ablation switches for kernel studies (tools/ablate.py); 0 = production */
void rn_set_debug_flags(int flags);
/* ablation builds (debug flag 4096): per-phase wave cycles of the merged
 * backward, summed over waves, read and cleared (synchronous) */
int rn_debug_cycles(unsigned long long* out);
/* rn_field_fwd_levels' level groups for studies: byte g = levels (lo nibble,
 * hi nibble) of group g, every level exactly once; 0 = default (g, 15 - g) */
int rn_set_level_pairing(uint64_t pairing);

/* ---- ray / AABB -----------------------------------------------------------
 * replaces vren.ray_aabb_intersect  (models/csrc/binding.cpp:4-16,
 * intersection.cu:25-100).  hits_t (n_rays, max_hits, 2), hits_voxel_idx
 * (n_rays, max_hits) are fully written (-1 = no hit).                       */
int rn_ray_aabb_intersect(const float* rays_o, const float* rays_d, const float* centers,
                          const float* half_sizes, int64_t n_rays, int64_t n_voxels,
                          int32_t max_hits, int32_t* hit_cnt, float* hits_t,
                          int64_t* hits_voxel_idx, void* stream);

/* ---- ray / sphere ------------------------------------------------------------
 * replaces vren.ray_sphere_intersect (binding.cpp:19-31, intersection.cu:103-197):
 * t_near clamped at 0, hits sorted by t_near like torch::sort (-1 slots first). */
int rn_ray_sphere_intersect(const float* rays_o, const float* rays_d, const float* centers,
                            const float* radii, int64_t n_rays, int64_t n_spheres,
                            int32_t max_hits, int32_t* hit_cnt, float* hits_t,
                            int64_t* hits_sphere_idx, void* stream);

/* ---- training ray march ----------------------------------------------------
 * replaces vren.raymarching_train (binding.cpp:60-81, raymarching.cu:166-332)
 * as three deterministic steps: count -> rn_scan_segments -> write.
 * hits_t is the (n_rays, 2) near/far slice, noise (n_rays) in [0,1).       */
int rn_raymarching_train_count(const float* rays_o, const float* rays_d, const float* hits_t,
                               const uint8_t* density_bitfield, int32_t cascades, float scale,
                               float exp_step_factor, const float* noise, int32_t grid_size,
                               int32_t max_samples, int64_t n_rays, int32_t* counts,
                               void* stream);
int rn_raymarching_train_write(const float* rays_o, const float* rays_d, const float* hits_t,
                               const uint8_t* density_bitfield, int32_t cascades, float scale,
                               float exp_step_factor, const float* noise, int32_t grid_size,
                               int32_t max_samples, int64_t n_rays, const int32_t* counts,
                               const int32_t* offsets, int64_t* rays_a, float* xyzs, float* dirs,
                               float* deltas, float* ts, void* stream);

/* RayMarcher.backward (custom_functions.py:102-112, torch_scatter.segment_csr):
 * per rays_a row, dL_drays_o = sum dL_dxyzs, dL_drays_d = sum(dL_dxyzs*ts + dL_ddirs). */
int rn_raymarching_train_bw(const float* dL_dxyzs, const float* dL_ddirs, const float* ts,
                            const int64_t* rays_a, int64_t n_rows, float* dL_drays_o,
                            float* dL_drays_d, void* stream);
/* the same for the fused (model-major, per (model, ray) segment) layout of
 * rn_ml_compact: counts / offsets [K][B]; dL_drays_o / dL_drays_d (B, 3)
 * written (sums over the K sub-NeRFs' samples of each ray).                 */
int rn_ml_march_bw(const int32_t* counts, const int32_t* offsets, int64_t n_rays,
                   int32_t n_models, const float* ts, const float* dL_dxyzs,
                   const float* dL_ddirs, float* dL_drays_o, float* dL_drays_d, void* stream);

/* exclusive scan of counts[n_seg][n_per]; segment k starts at an `align`
 * multiple: seg_base[k], seg_count[k]; meta[0] = aligned end, meta[1] = total.
 * (replaces the atomicAdd slot allocation of raymarching.cu:237-238)         */
int rn_scan_segments(const int32_t* counts, int32_t n_seg, int64_t n_per, int32_t align,
                     int32_t* offsets, int32_t* seg_base, int32_t* seg_count, int32_t* meta,
                     void* stream);

/* ---- test-time march -------------------------------------------------------
 * replaces vren.raymarching_test (binding.cpp:84-106, raymarching.cu:335-454);
 * hits_t (n_rays_total, 2) is advanced in place.                            */
int rn_raymarching_test(const float* rays_o, const float* rays_d, float* hits_t,
                        const int64_t* alive_indices, int64_t n_alive,
                        const uint8_t* density_bitfield, int32_t cascades, float scale,
                        float exp_step_factor, int32_t grid_size, int32_t max_samples,
                        int32_t n_samples, float* xyzs, float* dirs, float* deltas, float* ts,
                        int32_t* n_eff_samples, void* stream);

/* ---- fused multi-sub-NeRF march (ml_rendering.py:47-52 + :174-179) -------
 * AABB + NEAR clamp + jitter + march for K models in one launch; counts and
 * noise are [K][n_rays]; writes compact samples (t, dt, ray).
 * Two-pass form: rn_ml_march_count -> rn_scan_segments -> rn_ml_march_write.
 * Single-pass form: rn_ml_march_count with stage_ts/stage_deltas (K*n_rays*
 * max_samples floats each; slot of (k, r) at (k*n_rays + r)*max_samples) ->
 * rn_scan_segments -> rn_ml_compact.                                       */
int rn_ml_march_count(const float* rays_o, const float* rays_d, const float* center,
                      const float* half_size, float near_distance, const float* noise,
                      const uint8_t* density_bitfields, int64_t bitfield_bytes, int32_t n_models,
                      int32_t cascades, float scale, float exp_step_factor, int32_t grid_size,
                      int32_t max_samples, int64_t n_rays, int32_t* counts, float* stage_ts,
                      float* stage_deltas, void* stream);
int rn_ml_compact(const int32_t* counts, const int32_t* offsets, int64_t n_rays, int32_t n_models,
                  int32_t max_samples, const float* stage_ts, const float* stage_deltas,
                  float* ts, float* deltas, int32_t* ray_of, void* stream);
int rn_ml_march_write(const float* rays_o, const float* rays_d, const float* center,
                      const float* half_size, float near_distance, const float* noise,
                      const uint8_t* density_bitfields, int64_t bitfield_bytes, int32_t n_models,
                      int32_t cascades, float scale, float exp_step_factor, int32_t grid_size,
                      int32_t max_samples, int64_t n_rays, const int32_t* counts,
                      const int32_t* offsets, float* ts, float* deltas, int32_t* ray_of,
                      void* stream);

/* ---- compositing -----------------------------------------------------------
 * replaces vren.composite_train_fw / _bw / composite_test_fw
 * (binding.cpp:109-194, volumerendering.cu:6-286).                          */
int rn_composite_train_fw(const float* sigmas, const float* rgbs, const float* deltas,
                          const float* ts, const int64_t* rays_a, int64_t n_rows,
                          float T_threshold, int64_t* total_samples, float* opacity,
                          float* depth, float* rgb, float* ws, void* stream);
int rn_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                          const float* dL_dws, const float* sigmas, const float* rgbs,
                          const float* ws, const float* deltas, const float* ts,
                          const int64_t* rays_a, int64_t n_rows, const float* opacity,
                          const float* depth, const float* rgb, float T_threshold,
                          float* dL_dsigmas, float* dL_drgbs, void* stream);
int rn_composite_test_fw(const float* sigmas, const float* rgbs, const float* deltas,
                         const float* ts, int64_t n_alive, int32_t n_samples,
                         int64_t* alive_indices, float T_threshold, const int32_t* n_eff_samples,
                         float* opacity, float* depth, float* rgb, void* stream);

/* ---- distortion loss (Mip-NeRF 360 / DVGO-v2) ------------------------------
 * replaces vren.distortion_loss_fw / _bw (binding.cpp:197-231, losses.cu:9-150).
 * fw writes loss[rays_a[n][0]] and the per-sample inclusive scans of ws and
 * ws*ts; bw consumes those scans (losses.py:6-36 DistortionLoss).            */
int rn_distortion_loss_fw(const float* ws, const float* deltas, const float* ts,
                          const int64_t* rays_a, int64_t n_rows, float* loss, float* ws_incl,
                          float* wts_incl, void* stream);
int rn_distortion_loss_bw(const float* dL_dloss, const float* ws_incl, const float* wts_incl,
                          const float* ws, const float* deltas, const float* ts,
                          const int64_t* rays_a, int64_t n_rows, float* dL_dws, void* stream);

/* fused ml path: per-(model, ray) composite + gated combine
 * (ml_rendering.py:41-78 and the bg term of :192-200)                       */
int rn_ml_composite_fw(const float* sigmas, const float* rgbs, const float* deltas,
                       const float* ts, const int32_t* counts, const int32_t* offsets,
                       int64_t n_rays, int32_t n_models, float T_threshold, int32_t* used,
                       float* opacity_k, float* depth_k, float* rgb_k, float* ws, void* stream);
int rn_ml_combine_fw(const float* gate, const float* opacity_k, const float* depth_k,
                     const float* rgb_k, const float* bg, int64_t n_rays, int32_t n_models,
                     float* rgb, float* opacity, float* depth, void* stream);
int rn_ml_combine_bw(const float* dL_drgb, const float* dL_dopacity, const float* opacity_k,
                     const float* rgb_k, const float* bg, int64_t n_rays, int32_t n_models,
                     float* dL_dgate, void* stream);
int rn_ml_composite_bw(const float* dL_drgb, const float* dL_dopacity, const float* dL_ddepth,
                       const float* gate, const float* bg, const float* sigmas,
                       const float* rgbs, const float* deltas, const float* ts,
                       const int32_t* counts, const int32_t* offsets, const float* opacity_k,
                       const float* depth_k, const float* rgb_k, int64_t n_rays,
                       int32_t n_models, float T_threshold, float* dL_dsigmas, float* dL_drgbs,
                       void* stream);
/* the same with the Mip-NeRF 360 distortion loss of every (model, ray) segment
 * in the chain (losses.cu:47-142, losses.py:6-36 DistortionLoss per sub-NeRF
 * as NeRFLoss applies it, losses.py:63-67), without the ws_incl / wts_incl /
 * dL_dws arrays of rn_distortion_loss_fw / _bw:
 * fw also writes dist_k [K][B], the loss of the segment's ws (every other
 *   output is rn_ml_composite_fw's, bit for bit);
 * bw adds the loss's gradient for the seed dL_ddist [K][B] -- or, when that is
 *   NULL, the constant dL_ddist_const for every segment -- to dL_dsigmas, as
 *   VolumeRenderer.backward does with dL_dws (volumerendering.cu:109-151); it
 *   reads the ws and dist_k the forward wrote.  No gradient reaches ts /
 *   deltas (losses.py:36 returns None there).                               */
int rn_ml_composite_dist_fw(const float* sigmas, const float* rgbs, const float* deltas,
                            const float* ts, const int32_t* counts, const int32_t* offsets,
                            int64_t n_rays, int32_t n_models, float T_threshold, int32_t* used,
                            float* opacity_k, float* depth_k, float* rgb_k, float* ws,
                            float* dist_k, void* stream);
int rn_ml_composite_dist_bw(const float* dL_drgb, const float* dL_dopacity,
                            const float* dL_ddepth, const float* dL_ddist, float dL_ddist_const,
                            const float* gate, const float* bg, const float* sigmas,
                            const float* rgbs, const float* deltas, const float* ts,
                            const float* ws, const int32_t* counts, const int32_t* offsets,
                            const float* opacity_k, const float* depth_k, const float* rgb_k,
                            const float* dist_k, int64_t n_rays, int32_t n_models,
                            float T_threshold, float* dL_dsigmas, float* dL_drgbs, void* stream);
/* the same with depth supervision's ray-termination term in the chain: per
 * (model k, ray r) segment the second moment of its weights about the ray's
 * target ray parameter z = target_t[r] ((B) fp32; z <= 0: no measurement),
 *   dvar_k[k][r] = sum over the live samples s (up to the termination sample,
 *                  where ws != 0 can hold) of w_s min((t_s - z)^2, clip^2),
 * exactly 0 for z <= 0 and for an empty segment.  clip > 0 (INFINITY: none);
 * clip2 = clip * clip is one fp32 multiply on the host.
 * fw, per lane over its samples in ascending order (fp32, no contraction):
 *   e = t - z;  phi = fminf(e * e, clip2);  acc = fmaf(w, phi, acc)
 *   then one butterfly sum over the 64 lanes, as for depth_k.  dist_k NULL:
 *   every other output is rn_ml_composite_fw's, bit for bit; dist_k given: it
 *   and every other output are rn_ml_composite_dist_fw's, bit for bit.
 * bw, for the seed gv = dL_ddvar[k][r] ([K][B]): the per-sample seed on w_s is
 *   gw_s = gv * phi_s (phi as above; 0 for z <= 0 and past the termination) and
 *   the segment total of gw w is gv * dvar_k[k][r]; both enter
 *   dL/dsigma_s = delta_s [T_{s+1} gw_s - (total - sum_{j<=s} gw_j w_j)] + the
 *   plain terms, the expression rn_composite_train_bw evaluates for dL_dws; w is
 *   recomputed, ws is not read.  With dist_k and ws given (both or neither;
 *   dL_ddist [K][B] or NULL for the constant dL_ddist_const) the distortion
 *   seed joins as in rn_ml_composite_dist_bw: gw_s = gw_dist_s + gv * phi_s and
 *   total = 2 g dist_k + gv * dvar_k, added in that order.  No gradient reaches
 *   ts, deltas or target_t.                                                   */
int rn_ml_composite_depth_fw(const float* sigmas, const float* rgbs, const float* deltas,
                             const float* ts, const int32_t* counts, const int32_t* offsets,
                             int64_t n_rays, int32_t n_models, float T_threshold, int32_t* used,
                             float* opacity_k, float* depth_k, float* rgb_k, float* ws,
                             const float* target_t, float clip, float* dist_k /*may be NULL*/,
                             float* dvar_k, void* stream);
int rn_ml_composite_depth_bw(const float* dL_drgb, const float* dL_dopacity,
                             const float* dL_ddepth, const float* gate, const float* bg,
                             const float* sigmas, const float* rgbs, const float* deltas,
                             const float* ts, const int32_t* counts, const int32_t* offsets,
                             const float* opacity_k, const float* depth_k, const float* rgb_k,
                             const float* target_t, float clip, const float* dL_ddvar,
                             const float* dvar_k, const float* dL_ddist /*may be NULL*/,
                             float dL_ddist_const, const float* ws /*may be NULL*/,
                             const float* dist_k /*may be NULL*/, int64_t n_rays,
                             int32_t n_models, float T_threshold, float* dL_dsigmas,
                             float* dL_drgbs, void* stream);

/* ---- field: shared hash grid + per-model geo/rgb MLP -----------------------
 * replaces MNGP.forward / tcnn Encoding+Network fwd/bwd
 * (models/networks.py:229-328, custom_functions.py:162-173).
 * Sample input: xyzs/dirs (n_samples, 3) [single model], or, when xyzs is
 * NULL, compact (ts, ray_of) + rays with per-model seg_base/seg_count.
 * level_* (16 entries) and xyz_min/extent (3) are HOST arrays read at launch;
 * frags = packed f16 weights (device).
 * rn_field_bwd ADDS into grid_grad (fp32, tcnn layout) and dw (fp32, K x
 * FIELD_PARAMS); the caller zeroes them when a fresh gradient is wanted.
 * feat_cache (optional, device, 64 B per sample slot = 32 f16 encodings,
 * indexed like the samples): rn_field_fwd writes the hash-grid encoding there
 * and rn_field_bwd reads it instead of re-gathering the grid.  Pass the same
 * buffer and sample layout to both, or NULL to both.                       */
int rn_field_fwd(const float* xyzs, const float* dirs, int64_t n_samples, const float* ts,
                 const int32_t* ray_of, const float* rays_o, const float* rays_d,
                 const int32_t* seg_base, const int32_t* seg_count, int32_t n_models,
                 const void* grid_f16, const uint32_t* level_offset, const uint32_t* level_hsize,
                 const uint32_t* level_res, const float* level_scale, const float* xyz_min,
                 const float* extent, const void* frags, float* sigma, float* rgb,
                 void* feat_cache, int32_t blocks_per_model, void* stream);
int rn_field_bwd(const float* xyzs, const float* dirs, int64_t n_samples, const float* ts,
                 const int32_t* ray_of, const float* rays_o, const float* rays_d,
                 const int32_t* seg_base, const int32_t* seg_count, int32_t n_models,
                 const void* grid_f16, const uint32_t* level_offset, const uint32_t* level_hsize,
                 const uint32_t* level_res, const float* level_scale, const float* xyz_min,
                 const float* extent, const void* frags, const float* dL_dsigma,
                 const float* dL_drgb, float* grid_grad, float* dw, const void* feat_cache,
                 int32_t blocks_per_model, void* stream);

/* ---- merged field backward (fused training path) ------------------------
 * Same gradients as rn_field_bwd over the compact layout of rn_ml_compact,
 * but the hash-grid gradient of the K sub-NeRFs (which share the grid) is
 * scattered in merged per-ray (ray, t) order, so samples of different models
 * on one ray share atomic requests.
 * rn_bwd_plan builds the merged order (mstart [n_rays + 1] i32, perm [total]
 * i32) and the chunk schedule (chunk_first [cap_chunks + 1] i32: head_chunks
 * chunks ramping from ~0 to head_size merged samples, chunk c of
 * [head_size c (c + 1) / (2 head_chunks), head_size (c + 1) (c + 2) / (2
 * head_chunks)) (one per block, so the blocks' walks start staggered; none
 * when the ramp passes 15/16 of the work), then big chunks up to 15/16 of the work, then
 * min_chunk;
 * the big chunks are max_chunk merged samples, or with balance_blocks > 0 a
 * multiple of balance_blocks in number, each of at most max_chunk (every
 * persistent block takes the same number of them);
 * queue [3] i32 = bwd ticket, chunk count, fwd ticket; chunk_desc
 * [cap_chunks][20] i32 = first ray, end ray, 2 pad, first sample [8], count [8]
 * per model, read by the merged kernels with one 80-B load per ticket).  cap_chunks must bound the chunk
 * count: >= head_chunks + total/max_chunk + total/(8*min_chunk) + max_chunk/min_chunk + 3
 * (+ balance_blocks when balancing): the last big chunk can leave up to
 * max_chunk more samples to the min_chunk tail.  A smaller cap
 * truncates the schedule: chunks 0 .. cap_chunks - 1 are those of the full
 * schedule unchanged (the last kept chunk ends where chunk cap_chunks would
 * have begun, chunk_first[cap_chunks] is that ray, and no chunk exceeds
 * max_chunk + n_models * max_samples samples); the rays from there on are in
 * no chunk, so their samples are neither computed by rn_field_fwd_merged nor
 * scattered by rn_field_bwd_merged.  queue[1] == cap_chunks is the only sign
 * of a truncated plan (a cap that is exactly the chunk count reads the same).
 * mstart, perm and prep do not depend on the cap.  With prep (optional, [total] x 4 f32)
 * it also writes each merged position's (unit x, y, z, sample id as i32 bits)
 * for rn_field_fwd_levels (then called with prep_ready = 1): rays_o, rays_d
 * (device) and xyz_min, extent (host, 3 f32 each) are needed only then.
 * rn_field_bwd_merged runs `blocks` persistent blocks pulling chunks; each
 * stages 80-B rows in its scratch slice (scratch: blocks x scratch_rows x 20
 * f32, scratch_rows >= max_chunk + n_models * max_samples) and parks per-model
 * dW accumulators in park (blocks x n_models x 16384 f32).
 * Replaces, with rn_field_bwd, the backward of the tcnn modules called at
 * models/networks.py:300-328 (autograd sums the K sub-NeRFs' gradients into
 * the shared xyz_encoder's).                                               */
int rn_bwd_plan(const int32_t* counts, const int32_t* offsets, const int32_t* seg_base,
                const int32_t* seg_count, const float* ts, int64_t n_rays, int32_t n_models,
                int32_t head_chunks, int32_t head_size, int32_t max_chunk, int32_t min_chunk,
                int32_t balance_blocks, int32_t cap_chunks, int32_t* mstart, int32_t* perm,
                int32_t* chunk_first, int32_t* chunk_desc, int32_t* queue, const float* rays_o,
                const float* rays_d, const float* xyz_min, const float* extent, float* prep,
                void* stream);
int rn_field_bwd_merged(const float* ts, const int32_t* ray_of, const float* rays_o,
                        const float* rays_d, const int32_t* seg_base, const int32_t* seg_count,
                        const int32_t* mstart, const int32_t* perm,
                        const int32_t* chunk_desc, int32_t* queue, int64_t n_rays,
                        int32_t n_models, int32_t max_samples,
                        const void* grid_f16, const uint32_t* level_offset,
                        const uint32_t* level_hsize, const uint32_t* level_res,
                        const float* level_scale, const float* xyz_min, const float* extent,
                        const void* frags, const float* dL_dsigma, const float* dL_drgb,
                        float* grid_grad, float* dw, const void* feat_cache, float* scratch,
                        int64_t scratch_rows, float* park, int32_t max_chunk, int32_t blocks,
                        int32_t* igrad_lo, int32_t* igrad_carry, const float* igrad_scale,
                        int32_t* fx_acc, const float* fx_scale, uint32_t* fx_stats,
                        const int32_t* fx_redo, int32_t fx_mode, void* gb_ctl,
                        uint32_t* gb_page_meta, uint64_t* gb_pages, int32_t gb_pool_pages,
                        void* stream);

/* Fixed-point accumulation of the grid gradient (fx_mode 2, the fused
 * renderer's default; needs the encoding cache).  fx_acc: int32, one
 * per grid_grad element, zero on entry; fx_scale [16] f32 per level: 2^e_l, or
 * 0 for fp32 atomics into grid_grad (the first step); fx_stats: the
 * RN_FX_STATS_BYTES (640-B) per-level statistics block, zero before the first
 * step: u32 vmax[16] (the kernel atomic-maxes the bits of each level's largest
 * |record|), u32 emax[16] (rn_grid_fx_fold: the level's largest |int32 entry|),
 * i64 qsum[16] (the exact sum of each level's integer records), i64 esum[16]
 * (rn_grid_fx_fold: the exact sum of the level's int32 entries), u64 wq[16]
 * and we[16] (the same sums with each element i weighted by its byte offset
 * 4 i, mod 2^64; fixed point needs a grid of at most 2^28 gradient elements,
 * so the weight is injective below 2^30).
 * Each record goes in as rint(v * 2^e_l) with non-returning u32 atomics (the
 * memory side serves them ~27 % faster than f32 adds), so those levels'
 * gradients are order-independent and bitwise reproducible.
 * rn_grid_fx_fold then (1) sets *fx_redo when a level's largest record reached
 * 2^30 units or was not finite, or when the level's entry sum differs from its
 * record sum, plain or weighted (an int32 entry wrapped: many same-sign
 * records; two opposite wraps cancel only in the plain sum), writes the
 * next step's scales
 * (2^(27 - e), |record| < 2^e, capped so the largest entry stays < 2^29 units;
 * a dense level's first fixed-point step 2^(14 - e)) to fx_scale_next and clears
 * the statistics, (2) adds fx_acc * 2^-e_l into grid_grad (skipped when *fx_redo)
 * and re-zeroes fx_acc.  The caller then launches rn_field_bwd_merged with
 * fx_mode 3 and the same fx_scale (fp32 redo of the fixed-point levels' grid
 * scatter, no dW): it returns at once unless *fx_redo is set; and swaps
 * fx_scale_cur / fx_scale_next for the next step.
 * fx_mode 0: fp32 atomics (and the optional igrad_* integer mode).
 * fx_mode 4: binned (rn_grid_bin below): the fixed-point records (e5m17, the
 * largest < 2^38 units) are appended to the gb_* page pool (gb_ctl is reset
 * by the call) instead of atomically added; rn_grid_binned_fold then bins
 * and sums them into grid_grad (fx_acc unused).  A level whose fx_scale is 0
 * goes in by fp32 atomics into grid_grad instead (the renderer zeroes the
 * coarse levels', FusedMLRenderer.bin_f32_levels).
 * fx_mode 5: fx_mode 4 with levels 0-7 by fp32 atomics whatever their scale
 * (the walk's even streams compiled without page code; round 6).            */
int rn_grid_fx_fold(const uint32_t* level_offset, const uint32_t* level_hsize,
                    const uint32_t* level_res, int32_t* fx_acc, const float* fx_scale_cur,
                    float* fx_scale_next, uint32_t* fx_vmax, int32_t* fx_redo, float* grid_grad,
                    void* stream);

/* Binned ("store and sum") grid-gradient scatter, passes 2 and 3
 * (scatter.hip, formats in csrc/rn_bin.h).  Pass 1 is rn_field_bwd_merged
 * with fx_mode 4: it appends each level's fixed-point records (u64: entry
 * index 20 bits, two 22-bit e5m17 features, rn_grid_record_encode) to 64-KB
 * pages of a pool instead of issuing memory-side atomics.  ctl: the 128-B
 * GbCtl block (u32 pages taken, u32 pages per level [16], u32 fault bits:
 * 1 a page meta with a level >= 16 or more than 8192 records, 2 a record
 * index outside its level, 4 a level list past the pool, 8 a page id or run
 * outside the pool / page -- refused, never followed; then u32 sum_fault:
 * the sum passes' bit 8, sticky -- rn_field_bwd_merged zeroes only the first
 * 72 B each step, so a caller reads it back to learn that a sum pass, which
 * runs after the step's redo decision, skipped a run), zero before pass 1;
 * page_meta [pool_pages] u32 (level | count << 8); pages_in / pages_out
 * [pool_pages][8192] u64; desc
 * [pool_pages][256] u32; level_pages [16][pool_pages] u32.
 * rn_grid_bin sorts each page by slice of its level (level_hsize [16]: a
 * slice is the smallest power of two >= 64 entries that cuts the level into
 * <= 128 slices, 4096 at most) in LDS into pages_out and writes each slice's
 * run (start | count << 16) to desc and the page to its level's list.
 * rn_grid_sum (one workgroup per slice, 64 KB of LDS; the same level_hsize)
 * adds the slice's runs of every page of its level into int64
 * accumulators (exact, order-free) and then grid_grad += acc * 2^-e_l
 * (fx_scale) for every touched entry; it returns at once when *redo != 0.
 * Replaces the hash-grid parameter gradient of the tcnn GridEncoding
 * backward behind models/networks.py:300-328.                              */
/* timing studies (debug bit 21): k_grid_sum per-phase wave cycles, read and
 * reset (synchronous): [0..3] phases, [4] waves, [5] run groups, [6] / [7]
 * earliest start / latest end (s_memrealtime ticks, 100 MHz) */
int rn_debug_gb_cycles(unsigned long long* out);
int rn_grid_bin_layout(int32_t* out);   /* host: page records, bins per page, slice
                                          entries, ctl bytes, index bits, value bits,
                                          mantissa bits, target bits (out [8]) */
int rn_grid_slice_bits(const uint32_t* level_hsize, int32_t* out);   /* host: log2 of each
                                          level's slice size (out [16]) */
/* host: a record value x (gradient * 2^e_l) as the walk stores it, e5m17:
 * bits [0, 17) a two's-complement mantissa m, [17, 22) an exponent e, value
 * m * 2^e (e = 0 and m = rint(x) below 2^15; else |m| in [2^14, 2^15]), and
 * back (decode: the exact int64 value the sum pass adds) */
int rn_grid_record_encode(const float* x, int64_t n, uint32_t* out);
int rn_grid_record_decode(const uint32_t* f, int64_t n, int64_t* out);
int rn_grid_bin(const uint32_t* level_hsize, void* ctl, const uint32_t* page_meta,
                const uint64_t* pages_in, uint64_t* pages_out, uint32_t* desc,
                uint32_t* level_pages, int32_t pool_pages, int32_t blocks, void* stream);
/* rn_grid_bin + the binned redo / scale check (a record at 2^46 units, a
 * non-finite one, a pool overflow or a bin-pass fault sets *fx_redo; next
 * scales 2^(38 - e))
 * + rn_grid_sum, for a fx_mode 4 backward; the caller then launches the
 * fx_mode 3 redo exactly as after rn_grid_fx_fold.                         */
/* the first two steps of rn_grid_binned_fold (bin + check); a caller that
 * overlaps the grid gradient's all-reduce with the sum pass then runs
 * rn_grid_sum over the fine levels, starts their collective, and runs it
 * over the coarse ones (the fx_mode 3 redo may go before the sums: they exit
 * at once when *fx_redo is set) */
int rn_grid_bin_check(const uint32_t* level_hsize, void* ctl, const uint32_t* page_meta,
                      const uint64_t* pages_in, uint64_t* pages_out, uint32_t* desc,
                      uint32_t* level_pages, int32_t pool_pages, const float* fx_scale_cur,
                      float* fx_scale_next, uint32_t* fx_stats, int32_t* fx_redo, void* stream);
int rn_grid_binned_fold(const uint32_t* level_offset, const uint32_t* level_hsize, void* ctl,
                        const uint32_t* page_meta, const uint64_t* pages_in, uint64_t* pages_out,
                        uint32_t* desc, uint32_t* level_pages, int32_t pool_pages,
                        const float* fx_scale_cur, float* fx_scale_next, uint32_t* fx_stats,
                        int32_t* fx_redo, float* grid_grad, void* stream);
/* levels [level_lo, level_hi) only (0, 16: all) */
int rn_grid_sum(const uint32_t* level_offset, const uint32_t* level_hsize, const void* ctl,
                const uint32_t* desc, const uint32_t* level_pages, const uint64_t* pages_out,
                int32_t pool_pages, const float* fx_scale, const int32_t* redo, float* grid_grad,
                int32_t level_lo, int32_t level_hi, void* stream);

/* Fused test-time render (ml_rendering.py:81-155 / rendering.py:113-189,
 * raymarching.cu:335-404, volumerendering.cu:206-286): one wave per ray marches
 * its occupied samples 32 at a time (test-time calc_dt with `cascades`),
 * evaluates them as one MFMA field tile and composites them in the
 * reference's order until T <= T_threshold, the box exit or max_samples.
 * All n_models sub-NeRFs in one launch (gridDim.y); hits_t [n_rays][2] is the
 * near-clamped AABB interval (shared by the sub-NeRFs, as ml_rendering.py:
 * 91-94 computes the same one per sub-NeRF); density_bitfields
 * [n_models][bitfield_bytes]; frags [n_models][46 * 512] f16.  Outputs per
 * (sub-NeRF, ray), without background: opacity / depth [n_models][n_rays],
 * rgb [n_models][n_rays][3], n_samples (marched) [n_models][n_rays].
 * Replaces the host loop's
 * vren.raymarching_test + field + vren.composite_test_fw rounds.          */
int rn_render_test(const float* rays_o, const float* rays_d, const float* hits_t, int64_t n_rays,
                   int32_t n_models, const uint8_t* density_bitfields, int64_t bitfield_bytes,
                   int32_t cascades, float scale, float exp_step_factor, int32_t grid_size,
                   int32_t max_samples, const void* grid_f16, const uint32_t* level_offset,
                   const uint32_t* level_hsize, const uint32_t* level_res,
                   const float* level_scale, const float* xyz_min, const float* extent,
                   const void* frags, float T_threshold, float* opacity, float* depth,
                   float* rgb, int32_t* n_samples, int32_t blocks, void* stream);

/* ---- gate-sparse test-time render --------------------------------------------
 * The reference weights every sub-NeRF's render by the softmax gate
 * (ml_rendering.py:33-36,65-68); Ray_Gate.forward returns a third value,
 * top_k_indices, hard-wired to None (networks.py:1087-1093), so sparse gating
 * was planned there and never built.  These two entries drop the (ray,
 * sub-NeRF) pairs the gate has voted out before they are rendered.
 *
 * rn_gate_select.  gate (n_rays, K) fp32 row-major (rn_gate_fwd's rows), K =
 * n_models <= 16; 0 <= gate_min < 1; 1 <= gate_topk <= K.  Pair (r, i) is LIVE
 * iff gate[r,i] >= gate_min and fewer than gate_topk indices j have gate[r,j] >
 * gate[r,i], or gate[r,j] == gate[r,i] with j < i (rank by gate descending,
 * index ascending).  The first maximal gate of a row is live even below
 * gate_min, so every ray keeps at least one sub-NeRF.  Written:
 *   live (n_rays, K) uint8: 1 / 0;
 *   gate_used (n_rays, K) fp32: gate[r,i] where live, exactly 0.0f otherwise;
 *     with renormalize != 0, gate[r,i] / S_r where live, S_r the fp32 sum of the
 *     row's live gates in index order and the division correctly rounded (a
 *     row whose live gates are all 0 gives 0 / 0);
 *   list [K][n_rays] int32: list[i][0 .. count[i]) are the rays live for
 *     sub-NeRF i in ascending order; the tail is left as it was;  count [K];
 *   the DEAD slots of opacity_k / depth_k [K][n_rays], rgb_k [K][n_rays][3] and
 *     n_samples [K][n_rays] (rn_render_test's layouts) are set to 0; live slots
 *     are left for rn_render_test_list.  All four NULL: no zero-fill.
 * rn_ml_combine_test on the result with gate_used as its gate then adds an
 * exact (0 + bg * 1) * 0 = 0 per dead pair.  Without renormalize the image
 * differs from the dense one by at most the dead gate mass per ray: |d rgb_c|,
 * |d opacity| <= sum over dead i of gate[r,i], plus rounding.
 * List positions are ballot prefixes plus a scan of per-block counts, not
 * arrival-order atomics: every output is a pure function of the arguments.  No
 * host synchronisation.  n_rays == 0 zeroes count.  work: device scratch of
 * RN_GATE_SELECT_WORK_BYTES (4-byte aligned), not shared by calls in flight on
 * different streams.
 *
 * rn_render_test_list: rn_render_test for the listed pairs only.  The
 * arguments and the grid (blocks, n_models) are rn_render_test's; sub-NeRF i
 * renders rays list[i * n_rays + j], j < count[i], count read on the device,
 * where the grid's blocks are also shared out among the sub-NeRFs in
 * proportion to their counts (a sub-NeRF with most rays gets most blocks).
 * A listed pair's opacity, depth, rgb and n_samples are rn_render_test's bits
 * (one per-ray routine serves both kernels), in any list order; pairs not
 * listed are not written; an entry outside [0, n_rays) is skipped.          */
#define RN_GATE_SELECT_WORK_BYTES 65536
int rn_gate_select(const float* gate, int64_t n_rays, int32_t n_models, float gate_min,
                   int32_t gate_topk, int32_t renormalize, uint8_t* live, float* gate_used,
                   int32_t* list, int32_t* count, float* opacity_k /*may be NULL*/,
                   float* depth_k /*may be NULL*/, float* rgb_k /*may be NULL*/,
                   int32_t* n_samples /*may be NULL*/, void* work, void* stream);
int rn_render_test_list(const float* rays_o, const float* rays_d, const float* hits_t,
                        int64_t n_rays, int32_t n_models, const uint8_t* density_bitfields,
                        int64_t bitfield_bytes, int32_t cascades, float scale,
                        float exp_step_factor, int32_t grid_size, int32_t max_samples,
                        const void* grid_f16, const uint32_t* level_offset,
                        const uint32_t* level_hsize, const uint32_t* level_res,
                        const float* level_scale, const float* xyz_min, const float* extent,
                        const void* frags, float T_threshold, float* opacity, float* depth,
                        float* rgb, int32_t* n_samples, const int32_t* list,
                        const int32_t* count, int32_t blocks, void* stream);

/* ---- routed training (opt-in; DESIGN.md §4 "Routed training") ----------------
 * The training step for the (ray, sub-NeRF) pairs rn_gate_select keeps, so the
 * model that is trained is the model the gate-sparse render draws.  A DEAD pair
 * is a pair with sample count 0 and gate_used exactly 0: every kernel after the
 * march already handles pairs without samples (rays that miss the box), so
 * rn_scan_segments, rn_ml_compact, rn_bwd_plan, the field forwards / backwards,
 * the composites and rn_ml_march_bw run unchanged on the counts written here.
 *
 * rn_ml_march_count_list: rn_ml_march_count's arguments, then list [K][n_rays]
 * and count [K] in rn_gate_select's layouts (K = n_models <= 16; count is read
 * on the device, no host read).  The entry first zeroes counts [K][n_rays] on
 * the stream, then marches one wave per listed pair: wave w of the launch takes
 * flat pair w -- the running sum of count[] gives sub-NeRF k, list[k][w - sum]
 * the ray r -- so the live work is dense at the front of the grid and waves past
 * sum(count) leave at once.  Pair (k, r) gets counts[k][r] and the staging slot
 * (k*n_rays + r)*max_samples with rn_ml_march_count's bits (the same AABB test,
 * near clamp, jitter noise[k*n_rays + r] and per-ray march), whatever the order
 * of the list.  A pair not listed keeps count 0 and its staging slot is not
 * written.  An entry outside [0, n_rays) is skipped; count[k] is clamped to
 * [0, n_rays]; a pair listed twice is marched twice with the same result.
 *
 * rn_gate_select_bw: the backward of gate_used = rn_gate_select(gate) with the
 * selection (live) held constant -- the selection itself has no gradient.
 * gate, live as rn_gate_select read / wrote them; dL_dgate_used (n_rays, K) is
 * what rn_ml_combine_bw writes, which is non-zero on dead pairs (bg . dL_drgb)
 * and is masked here.  dL_dgate (n_rays, K), which may be dL_dgate_used itself:
 *   dead pair: exactly 0;
 *   live, renormalize == 0: dL_dgate_used[r,i];
 *   live, renormalize != 0: (d_i - D) / S with S the fp32 sum of the row's live
 *     gates in index order (rn_gate_select's S), u_j = gate_j / S correctly
 *     rounded, D the fp32 sum in index order, from 0, over live j of the rounded
 *     products d_j * u_j, no contraction, the final division correctly rounded;
 *     a row with S == 0 gives 0.
 * One lane per ray, no atomics: a pure function of the arguments.
 *
 * rn_nerf_loss_routed / rn_nerf_loss_routed_det: rn_nerf_loss / rn_nerf_loss_det
 * with gate_used in place of gate and live (n_rays, K) uint8.  A dead pair adds
 * nothing to the depth-mutual sum and gets dL_ddepth = 0; the row's mean depth
 * is sum_k depth * gate_used; the divisor stays B K, so with every pair live
 * and gate_used == gate the results are the dense entries' bit for bit.
 * importance is still the FULL softmax gate's column sums (the reference's
 * gating_importance, the term that keeps the routing balanced), and dL_dgate
 * its seed on the softmax gate -- add it after rn_gate_select_bw.            */
int rn_ml_march_count_list(const float* rays_o, const float* rays_d, const float* center,
                           const float* half_size, float near_distance, const float* noise,
                           const uint8_t* density_bitfields, int64_t bitfield_bytes,
                           int32_t n_models, int32_t cascades, float scale, float exp_step_factor,
                           int32_t grid_size, int32_t max_samples, int64_t n_rays,
                           int32_t* counts, float* stage_ts, float* stage_deltas,
                           const int32_t* list, const int32_t* count, void* stream);
int rn_gate_select_bw(const float* gate, const uint8_t* live, const float* dL_dgate_used,
                      int64_t n_rays, int32_t n_models, int32_t renormalize, float* dL_dgate,
                      void* stream);
int rn_nerf_loss_routed(const float* rgb, const float* target_rgb, const float* opacity,
                        const float* depth, const float* gate_used, const uint8_t* live,
                        const float* importance, int64_t n_rays, int32_t n_models,
                        float lambda_opacity, float lambda_cv, float lambda_dm, float* loss_out,
                        float* dL_drgb, float* dL_dopacity, float* dL_ddepth, float* dL_dgate,
                        void* stream);
int rn_nerf_loss_routed_det(const float* rgb, const float* target_rgb, const float* opacity,
                            const float* depth, const float* gate_used, const uint8_t* live,
                            const float* importance, int64_t n_rays, int32_t n_models,
                            float lambda_opacity, float lambda_cv, float lambda_dm,
                            float* loss_out, float* part, float* dL_drgb, float* dL_dopacity,
                            float* dL_ddepth, float* dL_dgate, void* stream);

/* Exact integer accumulation of the merged backward's grid gradient
 * (optional; igrad_lo == NULL keeps fp32 atomics into grid_grad).  With
 * igrad_lo / igrad_carry (int32, one per grid_grad element, zero on entry) and
 * igrad_scale (device f32, from rn_seed_scale), rn_field_bwd_merged adds each
 * contribution as rint(v * scale) with returning u32 atomics plus exact
 * carries; rn_igrad_to_f32 then adds (carry * 2^32 + lo) / scale into
 * grid_grad and re-zeroes the integer arrays.  Order-independent, so the grid
 * gradient is bitwise reproducible.  rn_seed_scale: scale = 2^(26 - e) for the
 * step's largest seed M in [2^(e-1), 2^e) (work: 1 u32 scratch word).      */
int rn_seed_scale(const int32_t* seg_base, const int32_t* seg_count, int32_t n_models,
                  const float* sigma, const float* dL_dsigma, const float* dL_drgb,
                  uint32_t* work, float* scale, void* stream);
int rn_igrad_to_f32(int64_t n, int32_t* igrad_lo, int32_t* igrad_carry, const float* scale,
                    float* grid_grad, void* stream);

/* Merged forward (fused training path, n_models <= 8): same outputs as
 * rn_field_fwd in compact mode, but blocks take rn_bwd_plan's chunks (queue
 * [2] is the forward's ticket) and evaluate the models' tiles of a chunk
 * interleaved, so the K sub-NeRFs' samples of one ray share cached grid
 * lines.  Replaces the per-sub-NeRF MNGP forward (models/networks.py:300-328
 * via ml_rendering.py:174-179).  With mstart and perm (rn_bwd_plan's merged
 * order) and feat_cache, each chunk is first encoded in merged (ray, t, model)
 * order into feat_cache, then the per-model MLP tiles read it back (NULL,
 * NULL: every tile encodes its own samples).  Outputs are identical.       */
int rn_field_fwd_merged(const float* ts, const int32_t* ray_of, const float* rays_o,
                        const float* rays_d, const int32_t* seg_base, const int32_t* seg_count,
                        const int32_t* chunk_desc, int32_t* queue,
                        int64_t n_rays, int32_t n_models, const void* grid_f16,
                        const uint32_t* level_offset, const uint32_t* level_hsize,
                        const uint32_t* level_res, const float* level_scale,
                        const float* xyz_min, const float* extent, const void* frags,
                        float* sigma, float* rgb, void* feat_cache, const int32_t* mstart,
                        const int32_t* perm, int32_t blocks, int32_t threads, void* stream);

/* Level-partitioned merged forward: the same sigma, rgb and feat_cache as
 * rn_field_fwd_merged with the merged-order encoding (bit-exact), in three
 * launches: the merged order's unit coordinates (prep: 16 B per merged
 * sample; skipped with prep_ready != 0, when rn_bwd_plan wrote them), then
 * the encoding split by level (block b encodes levels g and
 * 15 - g, g = b % 8, of every sample into planes[L * plane_stride + s], one
 * f16x2 per level; blocks go to the XCDs round-robin, so each XCD's L2 holds
 * two levels' tables), then the per-model MLP tiles read the planes.
 * plane_stride > every sample index; enc_blocks a multiple of 8; mlp_blocks of
 * 1024 threads.  xq (optional, 96 int32): [8 g + x] = blocks of group g that
 * ran on XCD x (a probe of the mapping), then u64 [32 + g] / [40 + g] the
 * first start / last end of group g's blocks (s_memrealtime, 100 MHz).  Replaces the same reference path as
 * rn_field_fwd_merged (models/networks.py:300-328 via ml_rendering.py:174-179). */
int rn_field_fwd_levels(const float* ts, const int32_t* ray_of, const float* rays_o,
                        const float* rays_d, const int32_t* seg_base, const int32_t* seg_count,
                        int64_t n_rays, int32_t n_models, const void* grid_f16,
                        const uint32_t* level_offset, const uint32_t* level_hsize,
                        const uint32_t* level_res, const float* level_scale,
                        const float* xyz_min, const float* extent, const void* frags,
                        float* sigma, float* rgb, void* feat_cache, const int32_t* mstart,
                        const int32_t* perm, uint32_t* planes, int64_t plane_stride, void* prep,
                        int32_t prep_ready, int32_t enc_blocks, int32_t mlp_blocks, int32_t* xq,
                        void* stream);

/* ---- ray gate (networks.py:1070-1093) --------------------------------------
 * input row r = (in0[r*stride + 0..2], in1[r*stride + 0..2]): pass x (B,6)
 * as (x, x+3, 6) or rays_o/rays_d as (rays_o, rays_d, 3).  importance (K) is
 * accumulated (zero it first) = gate.sum(0).                                */
int rn_gate_fwd(const float* in0, const float* in1, int32_t stride, int64_t n_rays,
                int32_t n_models, const void* frags, float* gate, float* importance,
                int32_t n_blocks, void* stream);
/* rn_gate_bwd: dL_dinput (optional, (B, 6) fp32, written): the gradient into
 * the gate input cat(in0, in1), as tcnn's Network backward provides when the
 * input requires grad (rays_o / rays_d under --optimize_ext,
 * train_ml.py:90-93); needs dinput_frags (4 transposed W0 fragments,
 * radnerf_amd/layout.py gate_dinput_frag_index).                            */
int rn_gate_bwd(const float* in0, const float* in1, int32_t stride, int64_t n_rays,
                int32_t n_models, const void* frags, const float* dL_dgate, float* dw,
                int32_t n_params, const void* dinput_frags, float* dL_dinput,
                int32_t n_blocks, void* stream);

/* ---- field input gradients and density-only evaluation (field_aux.hip) -----
 * rn_field_dinput: dL/dxyz and dL/ddir (fp32, (N, 3) each, written, indexed
 * like the samples) of MNGP.forward (models/networks.py:300-328: clip, hash
 * grid, d/|d|, SH, MLPs) for the seeds dL_dsigma / dL_drgb -- what tcnn's
 * Encoding / Network backward returns for inputs that require grad
 * (--optimize_ext, train_ml.py:90-93; custom_functions.py:102-112 consumes
 * it).  Same sample modes and arguments as rn_field_fwd/_bwd, plus
 * dinput_frags ([K][4][512] f16: the rgb net's SH columns transposed,
 * radnerf_amd/layout.py field_dinput_frag_index) and the optional encoding
 * cache of the forward.
 * rn_field_density: MNGP.density(x, ind, return_feat) (networks.py:291-309):
 * hash grid + geo MLP of one sub-NeRF (frags of that model); sigma (N) and,
 * if geo_feat is not NULL, h[:, 1:17] (N, 16) fp32 of the f16 values.       */
int rn_field_dinput(const float* xyzs, const float* dirs, int64_t n_samples, const float* ts,
                    const int32_t* ray_of, const float* rays_o, const float* rays_d,
                    const int32_t* seg_base, const int32_t* seg_count, int32_t n_models,
                    const void* grid_f16, const uint32_t* level_offset,
                    const uint32_t* level_hsize, const uint32_t* level_res,
                    const float* level_scale, const float* xyz_min, const float* extent,
                    const void* frags, const void* dinput_frags, const float* dL_dsigma,
                    const float* dL_drgb, const void* feat_cache, float* dL_dxyz,
                    float* dL_ddir, int32_t blocks_per_model, void* stream);
/* Occupancy-grid update on the device (MNGP.update_density_grid,
 * networks.py:375-409, train_ml.py:174-177), all n_models sub-NeRFs and
 * cascades in one call, no host synchronisation.  grid_ptrs / bitfield_ptrs:
 * device arrays of n_models pointers to the (cascades, 128^3) f32 density
 * grids (updated in place) and their bitfields.  all_cells != 0: every cell
 * (the warm-up, networks.py:330-343); else per (sub-NeRF, cascade) the cells
 * hit by 128^3/4 uniform draws and 128^3/4 draws among the cells with
 * density > threshold (networks.py:345-372): cell j is drawn with
 * probability 1 - e^-(1/4 + [occupied] (128^3/4) / n_occupied) (the
 * multinomial counts' Poisson limit), decided by a counter-based hash of
 * `seed` (same seed -> same cells on every rank).  Each drawn cell is
 * evaluated ONCE, at a jittered point of its cell (the reference's index_put
 * keeps one of a cell's draws, networks.py:394), in cell (Morton) order:
 * sigma from the grid + geo MLP (frags: [n_models][46 * 512] f16); then
 * grid = grid < 0 ? grid : max(grid * decay, sampled), packbits at
 * min(mean of the positive cells, threshold) (thr_out [n_models]).
 * Scratch: tmp (the sampled sigma, 0 = not drawn), occ (the drawn-cell list)
 * (n_models * cascades * 128^3 f32 / i32), blk (2 * (n_models * cascades *
 * 128^3 / 1024 + 1) i32), part (n_models * 1024 f32).  cascades <= 32.      */
int rn_density_update_sampled(const void* grid_ptrs, const void* bitfield_ptrs, int32_t n_models,
                              int32_t cascades, int32_t grid_size, float scale,
                              float density_threshold, float decay, uint64_t seed,
                              const void* grid_f16, const uint32_t* level_offset,
                              const uint32_t* level_hsize, const uint32_t* level_res,
                              const float* level_scale, const float* xyz_min, const float* extent,
                              const void* frags, float* tmp, int32_t* occ, int32_t* blk,
                              float* part, float* thr_out, int32_t all_cells,
                              void* stream);
/* rn_density_update_sampled on a grid culled by rn_mark_invisible_cells (same
 * kernels, same arguments, two more).  A cell whose density is negative is
 * never listed: not by the uniform draw, not by the occupied draw, not by the
 * warm-up's "every cell"; its tmp stays 0 and no sigma is evaluated for it.
 * erode != 0 (networks.py:396-398) needs count_grid ((cascades, 128^3) f32,
 * rn_mark_invisible_cells; status 1 without it): the decay of a cell is then
 * clamp(powf(decay, 1.0f / count), 0.1f, 0.95f) instead of decay.  With
 * erode == 0 count_grid may be NULL and is not read, and the density grids,
 * thr_out and bitfields left behind are bit-identical to
 * rn_density_update_sampled's for the same seed, whether or not the grid
 * holds negative cells (those keep their value in both); only tmp at the
 * negative cells differs.                                                    */
int rn_density_update_visible(const void* grid_ptrs, const void* bitfield_ptrs, int32_t n_models,
                              int32_t cascades, int32_t grid_size, float scale,
                              float density_threshold, float decay, uint64_t seed,
                              const void* grid_f16, const uint32_t* level_offset,
                              const uint32_t* level_hsize, const uint32_t* level_res,
                              const float* level_scale, const float* xyz_min, const float* extent,
                              const void* frags, float* tmp, int32_t* occ, int32_t* blk,
                              float* part, float* thr_out, int32_t all_cells,
                              const float* count_grid, int32_t erode, void* stream);
int rn_field_density(const float* xyzs, int64_t n_samples, const void* grid_f16,
                     const uint32_t* level_offset, const uint32_t* level_hsize,
                     const uint32_t* level_res, const float* level_scale, const float* xyz_min,
                     const float* extent, const void* frags, float* sigma, float* geo_feat,
                     void* stream);

/* ---- training-step epilogue ---------------------
 * rn_nerf_loss: losses.py:44-76 (NeRFLoss: rgb MSE, opacity entropy, CV^2 of
 * the gate importance, depth-mutual) fused with its backward.  Inputs are the
 * ml_render outputs rgb (B,3), opacity (B), depth (B,K), gating_code (B,K),
 * gating_importance (K).  loss_out[4] = sums of the four terms (lambdas
 * applied; [0] over B*3, [1] over B, [2] the CV^2 scalar, [3] over B*K):
 * divide by the element counts for the reference's per-term means.  Seeds:
 * the gradients of sum(term.mean()) w.r.t. rgb, opacity, depth and gate.
 * rn_adam: torch.optim.Adam step (train_ml.py:138-153, apex FusedAdam with
 * eps 1e-15) over n fp32 params; optional f16 mirror of params[0, n_f16).
 * The hyper-parameters are doubles: the step constants (1-beta, lr/bc1,
 * sqrt(bc2)) are formed in double on the host, as torch does, then rounded
 * once to fp32.                                                              */
int rn_nerf_loss(const float* rgb, const float* target_rgb, const float* opacity,
                 const float* depth, const float* gate, const float* importance, int64_t n_rays,
                 int32_t n_models, float lambda_opacity, float lambda_cv, float lambda_dm,
                 float* loss_out, float* dL_drgb, float* dL_dopacity, float* dL_ddepth,
                 float* dL_dgate, void* stream);
int rn_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
            double lr, double beta1, double beta2, double eps, int32_t step, float grad_scale,
            void* params_f16, int64_t n_f16, void* stream);

/* ---- deterministic training (opt-in; DESIGN.md §4 "Deterministic training") --
 * Five entries that replace the step's four fp32 sums in arrival order, so the
 * same parameters, inputs and seed give the same bits on one GPU in one
 * process, however the blocks and waves happen to be scheduled.
 * rn_reduce_partials: out[i] = (...((out[i] + part[0][i]) + part[1][i]) + ...
 * + part[n_slots - 1][i]) for i in [0, n); part is [n_slots][n] fp32.  ORDER
 * CONTRACT: plain fp32 adds in ascending slot order starting from the
 * incoming out[i], one thread per i, no atomics, no tree: the result equals
 * that loop bit for bit.  n_slots >= 1, n >= 0 (n == 0: nothing to do).
 * rn_colsum_ordered: out[c] = sum over rows of x[r][c] (x (rows, cols) fp32,
 * cols in 1..16; out written, not accumulated), gate.sum(0) without atomics.
 * The summation tree depends on (rows, cols) alone: tile t of 32 rows is
 * summed row by row (ascending) per column, then the tile sums are added in
 * ascending t, each as ((s_t0 + s_t1) + ...) per lane over tiles t = lane, lane
 * + 64, ..., then the 64 lane sums by a fixed xor butterfly (32, 16, ..., 1).
 * rows == 0 writes zeros.
 * rn_field_bwd_merged_det: rn_field_bwd_merged in the integer-grid form
 * (igrad_lo / igrad_carry / igrad_scale required, see rn_seed_scale) without
 * the fx_* / gb_* arguments.  SCHEDULE CONTRACT: chunk c of rn_bwd_plan's
 * plan is processed by block c mod blocks, and each block takes its chunks in
 * ascending c (queue is only read: [1], the chunk count; no ticket is taken),
 * so what a block sums depends on the plan alone.  dw is replaced by dw_part
 * ([blocks][n_models][9472] fp32): the entry zeroes it on the stream, then
 * block b stores its dW into slot b, every parameter written by exactly one
 * wave, once; a slot (or a model's row) of a block that met no sample of it
 * stays zero.  Sum the slots with rn_reduce_partials(dw_part, blocks,
 * n_models * 9472, dw).  The grid gradient goes to igrad_lo / igrad_carry
 * (exact integer sums, order-free; rn_igrad_to_f32 folds them).
 * rn_gate_bwd_det: rn_gate_bwd's results up to fp32 summation order, with one
 * wave per block (64 threads; tile t of 32 rays goes to block t mod n_blocks):
 * a block's adds run in its wave's program order, and the block stores its
 * whole dW (zeros included) into slot b of gate_part ([n_blocks][n_params]
 * fp32).  Sum with rn_reduce_partials(gate_part, n_blocks, n_params, dw).
 * rn_nerf_loss_det: rn_nerf_loss with the three per-ray sums (loss_out [0],
 * [1], [3]) written as per-block partials into part ([ceil(n_rays / 256)][4]
 * fp32; each block's sum is a fixed xor butterfly per wave, then its four
 * waves in order) and added in block order by one thread per term; loss_out
 * [2] and the four seeds are rn_nerf_loss's, bit for bit.                   */
int rn_reduce_partials(const float* part, int32_t n_slots, int64_t n, float* out, void* stream);
int rn_colsum_ordered(const float* x, int64_t rows, int32_t cols, float* out, void* stream);
int rn_field_bwd_merged_det(const float* ts, const int32_t* ray_of, const float* rays_o,
                            const float* rays_d, const int32_t* seg_base,
                            const int32_t* seg_count, const int32_t* mstart, const int32_t* perm,
                            const int32_t* chunk_desc, const int32_t* queue, int64_t n_rays,
                            int32_t n_models, int32_t max_samples, const void* grid_f16,
                            const uint32_t* level_offset, const uint32_t* level_hsize,
                            const uint32_t* level_res, const float* level_scale,
                            const float* xyz_min, const float* extent, const void* frags,
                            const float* dL_dsigma, const float* dL_drgb, float* grid_grad,
                            float* dw_part, const void* feat_cache, float* scratch,
                            int64_t scratch_rows, float* park, int32_t max_chunk, int32_t blocks,
                            int32_t* igrad_lo, int32_t* igrad_carry, const float* igrad_scale,
                            void* stream);
int rn_gate_bwd_det(const float* in0, const float* in1, int32_t stride, int64_t n_rays,
                    int32_t n_models, const void* frags, const float* dL_dgate, float* gate_part,
                    int32_t n_params, const void* dinput_frags, float* dL_dinput,
                    int32_t n_blocks, void* stream);
int rn_nerf_loss_det(const float* rgb, const float* target_rgb, const float* opacity,
                     const float* depth, const float* gate, const float* importance,
                     int64_t n_rays, int32_t n_models, float lambda_opacity, float lambda_cv,
                     float lambda_dm, float* loss_out, float* part, float* dL_drgb,
                     float* dL_dopacity, float* dL_ddepth, float* dL_dgate, void* stream);

/* rn_get_rays: train_ml.py:84-96 + ray_utils.py:45-70 for a batch of picks.
 * directions (P,3) camera-space; poses (I,3,4) c2w; img_idxs (n) or NULL
 * (one pose); pix_idxs (n) or NULL (directions are per ray).  imgs_d (n,3)
 * (the gate's 'image' input: the pose applied to mean_dir) may be NULL.      */
int rn_get_rays(const float* directions, const float* poses, const int64_t* img_idxs,
                const int64_t* pix_idxs, int64_t n_rays, const float* mean_dir, float* rays_o,
                float* rays_d, float* imgs_d, void* stream);

/* ---- camera pose refinement (--optimize_ext) --------------------------------
 * rn_get_rays_pose: train_ml.py:90-96 + ray_utils.py:73-100 (axisangle_to_R)
 * + ray_utils.py:45-70 for a batch of picks.  Per pick of image n the pose
 * [R0 | T0] = poses[n] is refined by dR[n] (axis-angle) and dT[n], both
 * (I,3): R = A(dR[n]) R0 with A(v) = I + (sin t / t) K + ((1 - cos t) / t^2)
 * K^2, K = skew(v), t = |v| + 1e-7, and T = T0 + dT[n] (the rotation is not
 * applied to the translation).  rays_d = R dir, rays_o = T, imgs_d = R
 * mean_dir.  dR and dT may each be NULL (zero): with both zero the outputs are
 * rn_get_rays'.  img_idxs (n) is required; pix_idxs (n) or NULL (directions
 * are per ray); imgs_d and mean_dir may be NULL together.
 * rn_get_rays_pose_bw: the backward the reference leaves to autograd (the
 * dR / dT parameters of train_ml.py:129-134).  From dL/drays_o, dL/drays_d
 * (n,3) and dL/dimgs_d ((n,3), or NULL together with mean_dir) it writes
 * dL/ddR and dL/ddT, (n_images,3) each: every row is written (zeros for an
 * image without a pick; nothing is accumulated, so no memset is needed), and
 * the sums run in a fixed order without atomics: two calls give the same
 * bits.  dR NULL: the gradient at dR = 0.  n_rays == 0 zeroes the outputs.  */
int rn_get_rays_pose(const float* directions, const float* poses, const float* dR,
                     const float* dT, const int64_t* img_idxs, const int64_t* pix_idxs,
                     int64_t n_rays, const float* mean_dir, float* rays_o, float* rays_d,
                     float* imgs_d, void* stream);
int rn_get_rays_pose_bw(const float* directions, const float* poses, const float* dR,
                        const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays,
                        int64_t n_images, const float* mean_dir, const float* dL_drays_o,
                        const float* dL_drays_d, const float* dL_dimgs_d, float* dL_ddR,
                        float* dL_ddT, void* stream);

/* ---- a training step's inputs from device-resident images --------------------
 * rn_sample_batch: datasets/base.py:23-31 (the batch's image and pixel picks,
 * iid uniform with replacement as np.random.choice, and the target gather) and
 * train_ml.py:84-96,180 (the rays of those picks, the march jitter, the random
 * background) in one launch, one thread per ray.  images: (n_images, n_pix, 3)
 * on the device, uint8 (image_dtype 0; target = (float)v / 255.0f, a division
 * as torch's u8.float() / 255) or fp32 (image_dtype 1; a bit copy); the element
 * offset (img n_pix + pix) 3 is 64-bit.  Outputs: img_idxs, pix_idxs (n_rays)
 * int64 (what rn_get_rays_pose_bw reads), target_rgb, rays_o, rays_d and imgs_d
 * (n_rays,3), noise (n_models, n_rays) or NULL, bg (3) or NULL.  The rays are
 * bit-identical to rn_get_rays' on the same picks when dR and dT are both
 * NULL, and to rn_get_rays_pose's otherwise (dR, dT: NULL or (n_images,3));
 * imgs_d and mean_dir are NULL together.
 * The random stream (part of the interface; all arithmetic is uint64, wrapping):
 *   mix(z): z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;
 *           z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)
 *           (the splitmix64 finaliser)
 *   G = 0x9e3779b97f4a7c15
 *   key = mix(seed * G + ((uint64)rank << 40 | step))
 *   pick i:  z = mix(key + (i + 1) * G);
 *            img = (hi32(z) * n_images) >> 32;  pix = (lo32(z) * n_pix) >> 32
 *   jitter of (model k, ray i):
 *            unit(mix((key ^ 0xd1b54a32d192ed03) + (k * n_rays + i + 1) * G))
 *   background channel c:
 *            unit(mix((key ^ 0x8cb92ba72f3d8dd7) + (c + 1) * G))
 *   unit(z) = float(z >> 40) * 2^-24, in [0, 1)
 * Status 1: step outside [0, 2^40), rank outside [0, 2^24), n_images or n_pix
 * outside [1, 2^32), image_dtype other than 0 / 1, n_models < 1, a missing
 * required pointer, imgs_d and mean_dir not both NULL or both given.
 * n_rays == 0 is a no-op returning 0.  Plain stores, no atomics, no host
 * synchronisation.                                                           */
int rn_sample_batch(const void* images, int32_t image_dtype, int64_t n_images, int64_t n_pix,
                    const float* directions, const float* poses, const float* dR,
                    const float* dT, const float* mean_dir, uint64_t seed, int64_t step,
                    int32_t rank, int64_t n_rays, int32_t n_models, int64_t* img_idxs,
                    int64_t* pix_idxs, float* target_rgb, float* rays_o, float* rays_d,
                    float* imgs_d /*may be NULL*/, float* noise /*may be NULL*/,
                    float* bg /*may be NULL*/, void* stream);

/* ---- error-guided pixel sampling ---------------------------------------------
 * A tiled error map over the training set steers rn_sample_batch's picks to
 * where the loss is, and each ray's seeds are divided by its sampling density,
 * so the gradient stays an unbiased estimate of the uniform batch's.
 * Geometry: images of W x H pixels (pixel index y W + x, as `directions`), a
 * tile edge `tile` in 1..256, tw = ceil(W / tile), th = ceil(H / tile); cell
 * c = (img th + ty) tw + tx, n_cells = n_images th tw < 2^24; edge cells are
 * narrower or shorter: cw(tx) = min(tile, W - tx tile), ch(ty) likewise,
 * n_px(c) = cw ch.  Per cell: emap fp32 (a fresh map is all 1.0), acc_sum
 * uint64 and acc_cnt uint32 (filled between refreshes), w uint32, cdf uint64.
 *
 * rn_guided_weights: w[c] = clamp(rintf(emap[c] * 65536.0f), 1, 2^24) (a NaN
 * clamps to 1), mass[c] = (uint64)w[c] n_px(c), cdf = the inclusive uint64
 * prefix sum of mass in cell order; total = cdf[n_cells - 1] < 2^64.  Integer
 * sums: any scan tree gives these bits.  Three launches on `stream` (block
 * sums, their scan, the cells), no host synchronisation.  work:
 * RN_GUIDED_WORK_BYTES of device scratch (8-byte aligned), not shared by
 * calls in flight on different streams.
 *
 * rn_sample_batch_guided: rn_sample_batch's arguments, outputs and stream,
 * plus cell_idx (n_rays) int32 and ray_weight (n_rays) fp32; n_pix == W H.
 * Per ray i, with key, G, mix and unit as above:
 *   z = mix(key + (i + 1) G)                          (rn_sample_batch's draw)
 *   u = unit(mix((key ^ 0xa0761d6478bd642f) + (i + 1) G))
 *   u < uniform_frac (an fp32 compare): the uniform branch, rn_sample_batch's
 *     picks from z;
 *   else: z2 = mix((key ^ 0xe7037ed1a0b428db) + (i + 1) G), t = mulhi64(z2,
 *     total); c = the smallest cell with cdf[c] > t; j = (t - cdf[c - 1]) /
 *     w[c] (cdf[-1] = 0; j < n_px(c)); the pixel is (y, x) = (ty tile + j /
 *     cw, tx tile + j % cw).
 *   cell_idx = the cell of the picked pixel, in either branch;
 *   ray_weight = (float)(1.0 / ((double)f + (((1.0 - f) (double)w[cell])
 *     (double)N_all) / (double)total)), f = (double)uniform_frac, N_all =
 *     n_images n_pix, the operations doubles in that order: (1 / N_all) / p
 *     for the mixture p = f / N_all + (1 - f) w / total, at most 1 / f.
 * Targets, rays, jitter and background are rn_sample_batch's on these picks.
 * The search runs in two levels (the images' last cdf entries, staged in LDS
 * for up to 20480 images, then the image's cells) and finds the cell a plain
 * binary search over cdf finds.  Status 1 also for tile outside 1..256, W H
 * != n_pix, n_cells >= 2^24, uniform_frac outside [0, 1].
 *
 * rn_guided_epilogue: after the loss kernel, before the backward.  Per ray r:
 * d = rgb[r] - target[r], e = (d0 d0 + d1 d1) + d2 d2 (fp32, no contraction);
 * a finite e adds (uint64)min(rintf(e * 2^20), 2^24) to acc_sum[cell_idx[r]]
 * and 1 to acc_cnt (integer atomics, no return value: order-free and exact;
 * the lanes of a wave that share a cell are summed first and issue one pair),
 * a non-finite e and a cell outside [0, n_cells) add nothing.  Then
 * dL_drgb[r, :], dL_dopacity[r] and dL_ddepth[r, :] ((n_rays, n_models), may
 * be NULL) are multiplied in place by ray_weight[r], one fp32 multiply each.
 * acc_sum / acc_cnt may be NULL together (scale only, cell_idx is not read).
 *
 * rn_guided_refresh: for cells with acc_cnt > 0, mean = (float)(((double)
 * acc_sum * 2^-20) / (double)acc_cnt) and emap = emap + alpha * (mean - emap)
 * (fp32, no contraction); other cells keep their value; both accumulators are
 * zeroed.  alpha in (0, 1].
 * All four: plain and vector stores, no host synchronisation.                */
#define RN_GUIDED_WORK_BYTES 131072
int rn_guided_weights(const float* emap, int64_t n_images, int32_t W, int32_t H, int32_t tile,
                      uint32_t* w, uint64_t* cdf, void* work, void* stream);
int rn_sample_batch_guided(const void* images, int32_t image_dtype, int64_t n_images,
                           int64_t n_pix, const float* directions, const float* poses,
                           const float* dR, const float* dT, const float* mean_dir,
                           uint64_t seed, int64_t step, int32_t rank, int64_t n_rays,
                           int32_t n_models, int64_t* img_idxs, int64_t* pix_idxs,
                           float* target_rgb, float* rays_o, float* rays_d,
                           float* imgs_d /*may be NULL*/, float* noise /*may be NULL*/,
                           float* bg /*may be NULL*/, int32_t W, int32_t H, int32_t tile,
                           float uniform_frac, const uint32_t* w, const uint64_t* cdf,
                           int32_t* cell_idx, float* ray_weight, void* stream);
int rn_guided_epilogue(const float* rgb, const float* target_rgb, const int32_t* cell_idx,
                       const float* ray_weight, int64_t n_rays, int32_t n_models,
                       int64_t n_cells, uint64_t* acc_sum /*may be NULL*/,
                       uint32_t* acc_cnt /*may be NULL*/, float* dL_drgb, float* dL_dopacity,
                       float* dL_ddepth /*may be NULL*/, void* stream);
int rn_guided_refresh(float* emap, uint64_t* acc_sum, uint32_t* acc_cnt, int64_t n_cells,
                      float alpha, void* stream);

/* ---- depth supervision --------------------------------------------------------
 * rn_gather_depth: the target ray parameter of each pick of a batch, one thread
 * per ray, after the picks exist (rn_sample_batch*, or the caller's).  depths:
 * (n_images, n_pix) on the device, uint16 (depth_dtype 0) or fp32 (1); the
 * element offset img n_pix + pix is 64-bit.  With v the raw value as fp32:
 *   kind 0: t = v * scale, one fp32 multiply (the z-depth of a camera whose
 *           directions have z = 1 and are not normalised, ray_utils.py:45-70);
 *   kind 1: Euclidean range: t = (v * scale) / sqrtf((dx dx + dy dy) + dz dz)
 *           with d = directions[pix] ((n_pix, 3), may be NULL for kind 0), the
 *           square root and the division correctly rounded, no contraction.
 * target_t[r] = t when v > 0 and t > 0, else 0 (a raw 0, a negative value, a
 * NaN, a pick outside the maps): 0 means "no measurement" downstream.  Status
 * 1: n_images or n_pix outside [1, 2^32), a dtype or kind other than 0 / 1, a
 * missing pointer.  n_rays == 0 is a no-op.
 *
 * rn_depth_loss: the two depth terms and their seeds, after rn_nerf_loss* and
 * rn_guided_epilogue (it adds into their seeds).  depth, gate (n_rays,
 * n_models): the render's per-model depth and the gate it was combined with
 * (gate_used on a routed step); dvar_k [K][B] (rn_ml_composite_depth_fw) or
 * NULL together with dL_ddvar (mean term only); z = target_t[r], m = z > 0;
 * rw = ray_weight[r], or 1 when ray_weight is NULL; B = n_rays.  Per ray with
 * m (fp32, no contraction, k ascending):
 *   lambda_depth > 0:  mean = sum_k gate[r,k] * depth[r,k];  e = mean - z;
 *     l0 = lambda_depth * (e * e);  s = ((2 lambda_depth / B) * e) * rw;
 *     dL_ddepth[r,k] += s * gate[r,k];  dL_dgate[r,k] += s * depth[r,k]
 *   dvar_k given:  l1 = lambda_depth_var * sum_k gate[r,k] * dvar_k[k][r];
 *     s = (lambda_depth_var / B) * rw (0 without m or with lambda_depth_var
 *     <= 0);  dL_ddvar[k][r] = s * gate[r,k] (written, every ray);
 *     dL_dgate[r,k] += s * dvar_k[k][r]
 * A ray without m adds nothing and gets dL_ddvar = 0.  loss_out[0] = sum l0,
 * loss_out[1] = sum l1 (the caller divides by B; the terms carry no
 * ray_weight), always as ordered sums: per-block partials into part
 * ([ceil(n_rays / 256)][2] fp32; a fixed xor butterfly per wave, then the four
 * waves in order), added in block order by one thread per term, so two calls
 * give the same bits.                                                         */
int rn_gather_depth(const void* depths, int32_t depth_dtype, int64_t n_images, int64_t n_pix,
                    float scale, int32_t kind, const float* directions /*may be NULL*/,
                    const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays,
                    float* target_t, void* stream);
int rn_depth_loss(const float* depth, const float* gate, const float* dvar_k /*may be NULL*/,
                  const float* target_t, const float* ray_weight /*may be NULL*/, int64_t n_rays,
                  int32_t n_models, float lambda_depth, float lambda_depth_var, float* loss_out,
                  float* part, float* dL_ddepth, float* dL_dgate, float* dL_ddvar /*may be NULL*/,
                  void* stream);

/* ---- whole-image validation (train_ml.py:214-250) ---------------------------
 * rn_ml_combine_test: the test-time epilogue of ml_rendering.py:65-68,149-153
 * (background, gate-weighted combine) plus the gated depth of train_ml.py:243,
 * on rn_render_test's outputs as they are (opacity_k / depth_k [K][n_rays],
 * rgb_k [K][n_rays][3], no background).  Per ray b, summed over i = 0..K-1 in
 * that order: rgb = sum g[b,i] (rgb_k[i,b] + bg (1 - op_k[i,b])), opacity =
 * sum g op_k, depth = sum g depth_k.  Results go to row ray0 + b of the
 * image-sized outputs rgb (N,3), opacity (N), depth (N) and, if given,
 * depth_k_out (N,K) (the reference's results['depth']), so a chunk loop fills
 * one image without copies.  gate (n_rays,K); NULL for K = 1 is a gate of
 * exactly 1 (a single NGP).  bg: 3 floats on the device.
 * rn_image_sse: the sum of squared differences of two fp32 arrays, the
 * sum_squared_error of PeakSignalNoiseRatio(data_range=1) (train_ml.py:64-66,
 * 222-224): PSNR = 10 log10(n_elems / sse).  out_sse (one device double) is
 * written; n_elems == 0 writes 0.
 * rn_ssim: StructuralSimilarityIndexMeasure(data_range=1) (train_ml.py:66,
 * 226-231) on (H*W, C) row-major interleaved images, C <= 4: Gaussian window
 * 11 x 11, sigma 1.5, normalised to sum 1; c1 = 0.01^2, c2 = 0.03^2; per pixel
 * (2 mu_p mu_t + c1)(2 s_pt + c2) / ((mu_p^2 + mu_t^2 + c1)(s_pp + s_tt + c2))
 * with s_xy = E[xy] - mu_x mu_y, on the valid windows only: an (H-10, W-10)
 * map per channel.  out_sum (one device double, written) is the sum of the
 * C (H-10)(W-10) values (divide for the score); ssim_map, if given, is the
 * (H-10, W-10, C) fp32 map.  pred == target gives exactly 1 per pixel.  H or
 * W below 11 is an invalid argument.
 * Both metrics sum per-block partials in a fixed order, in double, without
 * atomics: two calls give the same bits.  work: RN_METRICS_WORK_BYTES bytes of
 * device scratch (8-byte aligned), not shared by calls in flight on different
 * streams.                                                                   */
#define RN_METRICS_WORK_BYTES 8192
int rn_ml_combine_test(const float* gate, const float* opacity_k, const float* depth_k,
                       const float* rgb_k, const float* bg, int64_t n_rays, int32_t n_models,
                       int64_t ray0, float* rgb, float* opacity, float* depth,
                       float* depth_k_out /*may be NULL*/, void* stream);
int rn_image_sse(const float* pred, const float* target, int64_t n_elems, void* work,
                 double* out_sse, void* stream);
int rn_ssim(const float* pred, const float* target, int32_t H, int32_t W, int32_t C, void* work,
            double* out_sum, float* ssim_map /*may be NULL*/, void* stream);

/* ---- validation images (train_ml.py:47-52,238-248) --------------------------
 * The 8-bit pictures validation_step saves: (rgb * 255).astype(uint8), the
 * gate-weighted depth through depth2img (min-max normalise, COLORMAP_TURBO),
 * and a picture of the per-ray gating code.  All arithmetic is fp32, every
 * operation rounded on its own.  n == 0 is a valid no-op for all four; invalid
 * arguments give status 1 and nothing is written.  fp32 pointers must be
 * 4-byte aligned; uint8 pointers need no alignment (aligned dense buffers take
 * 16-byte loads, the rest dword loads; the result is the same).
 * rn_minmax_finite: out2 (two device floats) = {min, max} of x[i * stride],
 * i < n, over the finite values only (NaN, +-inf skipped); {0, 0} when there
 * is none (also n == 0).  stride >= 1 in elements, so one column of an (N, K)
 * buffer is read in place.  Per-block partials, then one fixed-order pass, no
 * atomics.  work: RN_METRICS_WORK_BYTES, as the metrics above.
 * rn_quantize_u8: dst[i] = src[i] * 255.0f, NaN -> 0, clamped to [0, 255],
 * truncated toward zero: numpy's astype(uint8) wherever that is defined.
 * rn_colormap_u8: depth2img.  range2 = {mn, mx} is read on the device (what
 * rn_minmax_finite wrote: no host round trip); den = mx - mn.  The index is 0
 * if !(den > 0) or x is not finite; else t = (x - mn) / den (a division),
 * t * 255.0f, NaN -> 0, clamped to [0, 255], truncated.  dst (n, 3) =
 * lut[index]; lut is 256 x 3 uint8 on the device; swap_rb != 0 exchanges
 * channels 0 and 2 of the output (the reference saves cv2's BGR as it is).
 * rn_gate_map_u8: gate (n, n_models) row-major, 1 <= n_models <= 16 (as
 * rn_gate_fwd); palette (n_models, 3) uint8 on the device; dst (n, 3).
 * hard == 0, per channel c: acc = g[0] * (float)p[0][c], then acc = acc +
 * g[k] * (float)p[k][c], k ascending; the byte is acc + 0.5f, NaN -> 0,
 * clamped to [0, 255], truncated.  hard != 0: the palette row of the first
 * maximal gate; a NaN never wins, row 0 if every gate is NaN.                */
int rn_minmax_finite(const float* x, int64_t n, int64_t stride, void* work, float* out2,
                     void* stream);
int rn_quantize_u8(const float* src, int64_t n, uint8_t* dst, void* stream);
int rn_colormap_u8(const float* x, int64_t n, int64_t stride, const float* range2,
                   const uint8_t* lut, int32_t swap_rb, uint8_t* dst, void* stream);
int rn_gate_map_u8(const float* gate, int64_t n, int32_t n_models, const uint8_t* palette,
                   int32_t hard, uint8_t* dst, void* stream);

/* ---- parameter packing (f32 master -> f16 MFMA fragments / f16 grid) ------*/
int rn_pack_f16(const float* src, int64_t src_stride, const int32_t* index, int64_t n,
                int32_t n_models, int64_t dst_stride, void* dst, void* stream);
int rn_to_f16(const float* src, int64_t n, void* dst, void* stream);

/* ---- occupancy grid maintenance (raymarching.cu:62-161, "next" row) -------*/
int rn_morton3d(const int32_t* coords, int64_t n, int32_t* indices, void* stream);
int rn_morton3d_invert(const int32_t* indices, int64_t n, int32_t* coords, void* stream);
int rn_packbits(const float* density_grid, int64_t n_bytes, float density_threshold,
                uint8_t* density_bitfield, void* stream);
/* out[indices[i]] = max(out[indices[i]], values[i]) for non-negative values:
 * the density update's `tmp[c, indices] = density(...)` (networks.py:393-394)
 * with duplicate cells resolved deterministically (the reference's
 * index_put keeps an arbitrary one of them).                                */
int rn_scatter_max(const int64_t* indices, const float* values, int64_t n, float* out,
                   void* stream);
/* Camera-visibility culling of the occupancy grids (upstream ngp_pl's
 * mark_invisible_cells; fills the count_grid that the erode line,
 * networks.py:396-398, divides by).  poses: (n_cams, 3, 4) c2w f32 on the
 * device, camera axes right / down / front (ray_utils.py:8-42); one pinhole
 * fx, fy, cx, cy and width x height for all cameras.  grid_ptrs /
 * bitfield_ptrs, n_models, cascades, grid_size (128), scale: as
 * rn_density_update_sampled.  No host synchronisation; status 1 for null or
 * invalid arguments (n_cams == 0 is one).
 * The operation order is part of the interface.  Everything is fp32, every
 * multiply and add rounded on its own (no fused multiply-add).  With
 * G = grid_size, per cascade c and Morton cell m of inverse Morton
 * coordinates (i_0, i_1, i_2) (rn_morton3d_invert of m, m >> 1, m >> 2):
 *   sc  = min(2^(c-1), scale);  hgs = sc / G
 *   X_a = ((i_a / (G-1)) * 2 - 1) * (sc - hgs)          (the cell centre)
 * and per camera [R | T] (R[i][j] = pose[4 i + j], T_i = pose[4 i + 3]),
 * with d_j = X_j - T_j:
 *   xc = (R[0][0]*d_0 + R[1][0]*d_1) + R[2][0]*d_2
 *   yc, zc: the same with column 1, column 2 of R
 *   px = fx*xc + cx*zc;  py = fy*yc + cy*zc
 *   in_image = zc > 0 && px >= 0 && px < W*zc && py >= 0 && py < H*zc
 *              (W, H = (float)width, (float)height; no division)
 *   covered  = in_image && zc >= near_distance
 *   too_near = in_image && zc <  near_distance
 * count_grid[c][m] = (float)n_covered / (float)n_cams, written for every cell
 * ((cascades, 128^3) f32, Morton order).  A cell is valid iff n_covered > 0
 * and no camera has it too near.  In each of the n_models grids a valid cell
 * keeps a value >= 0 and becomes 0 if it was negative, its bitfield bit is
 * left alone; an invalid cell becomes -1 and its bit is cleared.  The call is
 * idempotent (safe after a checkpoint load).  n_culled (may be NULL):
 * [cascades] i32, zeroed by the call, the number of invalid cells per
 * cascade.                                                                   */
int rn_mark_invisible_cells(const float* poses, int32_t n_cams, float fx, float fy, float cx,
                            float cy, int32_t width, int32_t height, float near_distance,
                            const void* grid_ptrs, const void* bitfield_ptrs, int32_t n_models,
                            int32_t cascades, int32_t grid_size, float scale, float* count_grid,
                            int32_t* n_culled, void* stream);

/* ---- mesh export (mesh.hip; radnerf_amd/mesh.py) ----------------------------
 * A lattice has nx x ny x nz cells, (nx + 1)(ny + 1)(nz + 1) < 2^31 points,
 * x fastest: point (i, j, k) is element i + (nx + 1)(j + (ny + 1) k).  lo and
 * step are 3 host floats each.  No entry synchronises with the host; invalid
 * arguments give status 1 and nothing is written.
 * rn_density_lattice: sigma (points, fp32, written) of the model on the
 * lattice, one launch.  Point i of an axis lies at lo + (float)i * step (a
 * multiply, then an add).  weights: n_models host floats; the value is
 * acc = w_0 sigma_0, then acc = acc + w_k sigma_k for k ascending over the
 * sub-NeRFs with w_k != 0 (the others are not evaluated; none: zeros), where
 * sigma_k is rn_field_density's value at the point for sub-NeRF k (the same
 * clip, encoding, MFMA order and expf).  frags: all n_models <= 16 sub-NeRFs'
 * fragments, as rn_field_fwd.  The sub-NeRFs share the hash grid, so a point
 * is encoded once for all of them.
 * rn_surface_*: naive surface nets of the lattice sigma at the level iso, all
 * arithmetic fp32, every operation rounded on its own.
 *   Inside: sigma[p] >= iso (NaN is outside).  Cell (i, j, k), c = i + nx (j +
 *   ny k), has corner q at offset (q & 1, q >> 1 & 1, q >> 2 & 1) and is active
 *   iff its corners are not all alike.  Active cells are vertices 0 .. V - 1
 *   in ascending c.
 *   Position: over the 12 cell edges in the order axis a = 0, 1, 2 and, within
 *   an axis, e = 0 .. 3 (bit 0 of e on the lower remaining axis, bit 1 on the
 *   higher; the edge runs from corner q0 to q1 = q0 | 1 << a): where the ends
 *   differ in insideness, t = (iso - s0) / (s1 - s0), t = fminf(fmaxf(t, 0),
 *   1) (NaN gives 0); the crossing is q0's offset with component a replaced by
 *   t; crossings are summed in that order and counted.  Lattice position
 *   (i, j, k) + sum / count, world position lo + position * step.
 *   Normal: g_a = the sum over the four a-edges, e = 0 .. 3, of (s1 - s0);
 *   n = -g / sqrtf((gx^2 + gy^2) + gz^2), or (0, 0, 0) when g is not finite or
 *   the norm is not positive: normals point from dense to empty.
 *   Faces: the lattice edge from point P along axis a emits a quad iff its
 *   ends differ in insideness, P_a <= n_a - 1 and, with b = (a + 1) % 3,
 *   c = (a + 2) % 3, 1 <= P_b <= n_b - 1 and 1 <= P_c <= n_c - 1 (boundary
 *   edges emit nothing).  Its four cells share a-coordinate P_a and have
 *   (b, c) offsets v0 (-1, -1), v1 (0, -1), v2 (0, 0), v3 (-1, 0); the quad is
 *   (v0, v1, v2, v3) if P is inside (the surface faces +a), else (v0, v3, v2,
 *   v1); quad (q0, q1, q2, q3) is the triangles (q0, q1, q2), (q0, q2, q3) in
 *   adjacent rows.  Quads are ordered by ascending 3 p + a, p the linear index
 *   of P.
 * Both orders come from exclusive scans, no atomic is used: the same lattice
 * gives the same bits on every call.
 * rn_surface_work_bytes: *bytes (host) = the size of `work` for the lattice,
 * 592 B per 1024 points plus 32 (0.58 B per point); no device work.
 * rn_surface_count: classifies the lattice into work and leaves the counts in
 * its first two int64: work[0] = V, work[1] = the number of quads (F = twice
 * that).  The caller reads them (the only synchronisation of an extraction)
 * and sizes the outputs.
 * rn_surface_emit: after rn_surface_count on the same lattice, iso and work:
 * vertices (n_vertices, 3) fp32, normals (n_vertices, 3) fp32 or NULL, faces
 * (2 n_quads, 3) int32, all written.  n_vertices and n_quads are the rows the
 * outputs hold (rows past them are not written); n_vertices and 2 n_quads
 * must be below 2^31.                                                         */
int rn_density_lattice(int32_t nx, int32_t ny, int32_t nz, const float* lo, const float* step,
                       const float* weights, int32_t n_models, const void* grid_f16,
                       const uint32_t* level_offset, const uint32_t* level_hsize,
                       const uint32_t* level_res, const float* level_scale, const float* xyz_min,
                       const float* extent, const void* frags, float* sigma, void* stream);
int rn_surface_work_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes);
int rn_surface_count(const float* sigma, int32_t nx, int32_t ny, int32_t nz, float iso,
                     void* work, void* stream);
int rn_surface_emit(const float* sigma, int32_t nx, int32_t ny, int32_t nz, float iso,
                    const float* lo, const float* step, const void* work, int64_t n_vertices,
                    int64_t n_quads, float* vertices, float* normals, int32_t* faces,
                    void* stream);

/* ---- mesh clean-up (mesh.hip, mesh_clean.hip; radnerf_amd/mesh.py) ----------
 * rn_density_lattice_masked: rn_density_lattice with the occupancy bitfields
 * as a mask.  bitfields: n_models host pointers to the sub-NeRFs' device
 * bitfields (cascades * grid_size^3 / 8 bytes each, Morton order; read only for
 * w_k != 0); grid_size is a power of two.  sigma_k at a lattice point (x, y, z)
 * counts as exactly 0 when the point's cell in sub-NeRF k's bitfield is clear.
 * The cell is the one the march queries for the position, the dt term dropped:
 *   mip = min(cascades - 1, max(0, e + 1)), frexpf(max(|x|, |y|, |z|), &e)
 *   mbi = 1 / min(2^(mip - 1), scale)
 *   n_c = (int)fmaxf(0, fminf(0.5f * fmaf(c, mbi, 1.0f) * grid_size,
 *                             grid_size - 1))            per axis c = x, y, z
 *   idx = mip * grid_size^3 + morton3d(n_x, n_y, n_z); the bit is idx & 7 of
 *   byte idx >> 3.
 * The value is acc = w_0 s_0, then acc = acc + w_k s_k as rn_density_lattice
 * adds them, with s_k = live ? sigma_k : 0: where every cell is set the result
 * has rn_density_lattice's bits.  A tile of 32 consecutive points that is dead
 * for every live sub-NeRF is written as zeros without being encoded.
 * rn_mesh_*: the connected components of a triangle mesh and the compaction of
 * some of them.  faces: (F, 3) int32 on the device, V vertices, 1 <= V < 2^31,
 * 0 <= F < 2^31.  A face with an index outside [0, V) is never dereferenced:
 * it joins nothing, belongs to no component, is never kept, and raises
 * work[0].  No entry synchronises with the host.
 *   Connectivity: two vertices are connected when some face holds both;
 *   components are the transitive closure; a vertex in no face is a component
 *   of its own.  root[v] is the lowest vertex index of v's component.
 *   Components are numbered 0 .. C - 1 in ascending order of root (an
 *   exclusive scan over the flags root[v] == v); label[v] is the number of
 *   v's component, comp_vertices[c] and comp_faces[c] its sizes, a face
 *   counting for the component of its vertices.
 *   Compaction: keep[c] != 0 keeps component c.  Kept vertices keep their
 *   relative order (new index = the exclusive scan of the kept flags), kept
 *   faces theirs, with indices remapped; normals and colors rows travel with
 *   their vertices.
 * Every order comes from a scan; the atomics used (integer min, add, or) give
 * results that do not depend on order: the same mesh gives the same bits on
 * every call, and label does not depend on the order of the face rows.
 * work: int64 words, work[0] = some face index is out of range, work[1] = the
 * labelling has not converged, work[2] = C, work[3], work[4] = kept vertices,
 * kept faces; the scan tables follow.
 * rn_mesh_work_bytes: *bytes (host) = the size of work, 64 + 168 B per 1024
 * vertices and per 1024 faces; no device work.
 * rn_mesh_label: with restart != 0 sets root[v] = v and work[0]; then `rounds`
 * rounds of (hook: the lowest of a face's three labels onto its vertices and
 * onto the vertices those labels name, by atomicMin; jump: root[v] = the
 * label of the label of root[v], by atomicMin), then one check that writes
 * work[1] (0 iff every face has three equal labels and root[root[v]] ==
 * root[v] everywhere: then root is as defined above) and work[2].  A label only
 * ever decreases to a vertex of the same component, so a stale read costs a
 * round and nothing else; no kernel waits on another workgroup or loops
 * without a bound known at launch.  The caller launches batches (restart = 0
 * after the first) until work[1] == 0.
 * rn_mesh_components: after convergence, n_components = work[2]: label (V)
 * int32, comp_vertices and comp_faces (n_components) int64, all written.
 * rn_mesh_compact_count: marks the kept vertices and faces in work and leaves
 * their numbers in work[3], work[4] for the caller to size the outputs.
 * rn_mesh_compact_emit: after rn_mesh_compact_count on the same mesh and work:
 * out_vertices (kept_vertices, 3) fp32, out_faces (kept_faces, 3) int32, and
 * out_normals fp32 / out_colors uint8 where normals / colors are not NULL;
 * rows past the kept counts given are not written.                            */
int rn_density_lattice_masked(int32_t nx, int32_t ny, int32_t nz, const float* lo,
                              const float* step, const float* weights, int32_t n_models,
                              const void* grid_f16, const uint32_t* level_offset,
                              const uint32_t* level_hsize, const uint32_t* level_res,
                              const float* level_scale, const float* xyz_min, const float* extent,
                              const void* frags, const void* const* bitfields, int32_t cascades,
                              int32_t grid_size, float scale, float* sigma, void* stream);
int rn_mesh_work_bytes(int64_t n_vertices, int64_t n_faces, int64_t* bytes);
int rn_mesh_label(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* root,
                  void* work, int32_t rounds, int32_t restart, void* stream);
int rn_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                       const int32_t* root, void* work, int64_t n_components, int32_t* label,
                       int64_t* comp_vertices, int64_t* comp_faces, void* stream);
int rn_mesh_compact_count(const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                          const int32_t* label, const uint8_t* keep, int64_t n_components,
                          void* work, void* stream);
int rn_mesh_compact_emit(const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                         const void* work, const float* vertices, const float* normals,
                         const uint8_t* colors, int64_t kept_vertices, int64_t kept_faces,
                         float* out_vertices, float* out_normals, uint8_t* out_colors,
                         int32_t* out_faces, void* stream);

/* ---- TSDF fusion (tsdf.hip, mesh.hip; radnerf_amd/tsdf.py) -------------------
 * Rendered depth images folded into a truncated signed distance volume on a
 * lattice (geometry as rn_density_lattice: nx x ny x nz cells, x fastest, point
 * i of an axis at lo + (float)i * step), the surface nets of such a volume, and
 * vertex colours from it.  No entry synchronises with the host or uses an
 * atomic; invalid arguments give status 1 and nothing is written.
 * Volume state per point: phi (points) fp32, the mean of the truncated signed
 * distances observed, POSITIVE INSIDE, in units of trunc (so in [-1, 1]); w
 * (points) fp32, the integer-valued number of observations; optionally vol_rgb
 * (points, 3) fp32 and wc (points) fp32, the mean colour and its count (both
 * or neither).  A fresh volume is all zeros; w == 0 means "never observed".
 * rn_tsdf_integrate: one launch folds n_cams depth images into the volume.
 * poses (n_cams, 3, 4) c2w on the device, axes right / down / front, R[i][j] =
 * pose[4 i + j], T_i = pose[4 i + 3]; one pinhole fx, fy, cx, cy, width x
 * height for all (pixel centres at +0.5, as ray_utils.py:8-42); directions
 * (width * height, 3), the buffer the images were rendered with (it need not
 * be normalised); depth, opacity (n_cams, width * height), the renderer's
 * sum w t and sum w; rgb (n_cams, width * height, 3) or NULL (then vol_rgb and
 * wc are left alone; rgb needs vol_rgb).  trunc > 0, near_distance >= 0,
 * opacity_min > 0.  n_cams == 0 is a valid no-op.
 * The operation order is part of the interface.  Everything is fp32, every
 * operation rounded on its own (no fused multiply-add; divisions and square
 * roots correctly rounded).  The point at X_a = lo_a + (float)i_a * step_a
 * visits the cameras c = 0 .. n_cams - 1 in that order; with d_j = X_j - T_j:
 *   xc = (R[0][0]*d_0 + R[1][0]*d_1) + R[2][0]*d_2
 *   yc, zc: the same with column 1, column 2 of R (as rn_mark_invisible_cells)
 *   next camera unless zc >= near_distance
 *   px = (fx*xc)/zc + cx;  py = (fy*yc)/zc + cy;  u = floorf(px), v = floorf(py)
 *   next camera unless 0 <= u < width and 0 <= v < height (compared as floats:
 *   a NaN is outside);  pix = v * width + u
 *   o = opacity[c][pix]
 *   unless o >= opacity_min (a miss; a NaN too):
 *     carve == 0: next camera;  carve != 0: phi_obs = -1, no colour (free space)
 *   else:
 *     d  = depth[c][pix] / o
 *     e  = directions[pix];  n2 = (e_0*e_0 + e_1*e_1) + e_2*e_2
 *     tv = ((xc*e_0 + yc*e_1) + zc*e_2) / n2
 *     s  = (tv - d) * sqrtf(n2)       (world distance behind the surface)
 *     next camera unless s <= trunc   (hidden: not observed; a NaN too)
 *     phi_obs = fmaxf(s / trunc, -1);  colour iff s >= -trunc
 *   phi = (phi * w + phi_obs) / (w + 1);  w = w + 1
 *   with rgb and colour, per channel k: vol_rgb_k = (vol_rgb_k * wc +
 *   rgb[c][pix][k]) / (wc + 1);  then wc = wc + 1
 * The point's state is read once before and written once after its cameras
 * (not at all where no camera observed it), so any split of the cameras into
 * consecutive launches gives the same bits as one launch.
 * rn_surface_count_valid / rn_surface_emit_valid: rn_surface_count /
 * rn_surface_emit on the lattice phi with the observation counts w, and two
 * more rules: a cell is active only if all 8 of its corners have w > 0 (and
 * are not all alike); a lattice edge emits its quad only if, besides
 * rn_surface_count's conditions, all four cells around it have all corners
 * observed.  Inside, positions, normals, the two orders, work
 * (rn_surface_work_bytes, the same layout) and the counts in work[0], work[1]
 * are rn_surface_*'s; with w > 0 everywhere the output has rn_surface_*'s
 * bits.  rn_surface_emit_valid reads the classification from work (and the
 * values of active cells only); w must be the lattice rn_surface_count_valid
 * classified.
 * rn_lattice_colors: colors (n_vertices, 3) uint8 from the colour lattice.
 * Per vertex and axis a (n_a cells): g = (v_a - lo_a) / step_a (a division),
 * c = fminf(fmaxf(floorf(g), 0), n_a - 1) (NaN gives 0), f = fminf(fmaxf(g -
 * c, 0), 1); corner q = 0 .. 7 of cell c at offset (q & 1, q >> 1 & 1, q >> 2
 * & 1) has the weight t_q = (wx * wy) * wz with w_a = f_a where the offset is
 * 1, else 1 - f_a.  Over the corners with wc > 0, q ascending: sw = sw + t_q,
 * acc_k = acc_k + t_q * vol_rgb[corner][k].  Channel k is acc_k / sw, or 0
 * when sw is not positive, quantised by rn_quantize_u8's rule (times 255.0f,
 * NaN -> 0, clamped to [0, 255], truncated).  n_vertices == 0 is a valid
 * no-op.                                                                      */
int rn_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, const float* lo, const float* step,
                      const float* poses, int32_t n_cams, float fx, float fy, float cx, float cy,
                      int32_t width, int32_t height, const float* directions, const float* depth,
                      const float* opacity, const float* rgb, float trunc, float near_distance,
                      float opacity_min, int32_t carve, float* phi, float* w, float* vol_rgb,
                      float* wc, void* stream);
int rn_surface_count_valid(const float* phi, const float* w, int32_t nx, int32_t ny, int32_t nz,
                           float iso, void* work, void* stream);
int rn_surface_emit_valid(const float* phi, const float* w, int32_t nx, int32_t ny, int32_t nz,
                          float iso, const float* lo, const float* step, const void* work,
                          int64_t n_vertices, int64_t n_quads, float* vertices, float* normals,
                          int32_t* faces, void* stream);
int rn_lattice_colors(const float* vertices, int64_t n_vertices, int32_t nx, int32_t ny,
                      int32_t nz, const float* lo, const float* step, const float* vol_rgb,
                      const float* wc, uint8_t* colors, void* stream);

/* ---- LPIPS (VGG) (train_ml.py:64-70, --eval_lpips) --------------------------
 * The pieces of the LPIPS distance of the `lpips` package 0.1, net vgg: the
 * input step, VGG16's 3 x 3 convolutions, its 2 x 2 max-pool and the per-tap
 * distance (radnerf_amd/lpips.py composes them).  Activations are f16,
 * (n_img, H, W, C) row-major with the channels innermost; every accumulation
 * is fp32; no entry uses an atomic, so a result is a function of the inputs
 * alone.  Invalid arguments give status 1 and nothing is written; nothing
 * synchronises with the host.
 * rn_lpips_prepare: rgb (n_pix, 3) fp32 -> out_f16 (n_pix, 3) f16.  Per
 * element of channel c, fp32, every operation rounded on its own:
 *   v = min(max(2 x - 1, -1), 1);  y = (v - shift[c]) / scale[c]  (a division)
 * with shift = (-.030, -.088, -.188), scale = (.458, .448, .450) as fp32
 * constants; y is rounded to f16 once.  n_pix == 0 is a valid no-op.
 * rn_conv3x3_relu_f16: out = relu(conv3x3(in) + bias) for n_img images in one
 * launch: stride 1, zero padding 1, in (n_img, H, W, Cin) -> out (n_img, H, W,
 * Cout), both f16.  Per output element the 9 Cin products are summed in fp32
 * (on v_mfma_f32_32x32x16_f16: f16 products are exact, the order is the
 * kernel's), then acc + bias[co] in fp32, max(., 0), one rounding to f16.
 * Cin is 3 (the first layer: its 27-long reduction is padded to 32 inside) or
 * a multiple of 64; Cout is a multiple of 64: no other padding of C exists,
 * the buffers hold exactly Cin and Cout channels per pixel.  bias: Cout fp32.
 * wfrag: the weights as MFMA A-operand fragments of 64 lanes x 8 halfs (1 KiB,
 * lane-linear).  Lane l (r = l & 31, h = l >> 5), element j of fragment
 *   Cin >= 64: ((ct (Cin / 64) + chunk) 9 + tap) 4 + ks
 *              = W[32 ct + r][64 chunk + 16 ks + 8 h + j][tap / 3][tap % 3]
 *   Cin == 3:  2 ct + ks = W[32 ct + r][k % 3][(k / 3) / 3][(k / 3) % 3] with
 *              k = 16 ks + 8 h + j, zero for k >= 27
 * for W (Cout, Cin, 3, 3) (cross-correlation, as torch's conv2d), ct < Cout /
 * 32: 9 Cin Cout halfs (Cin == 3: 32 Cout).  in and wfrag 16-byte aligned (in:
 * 2-byte for Cin == 3), out 8-byte.  in and out must not overlap.
 * rn_maxpool2_f16: in (n_img, H, W, C) -> out (n_img, H / 2, W / 2, C), the
 * maximum of each 2 x 2 block, floor sizes (an odd last row or column is
 * dropped); exact.  H, W >= 2; C a multiple of 8; both 16-byte aligned.
 * rn_lpips_layer: one tap's distance summed over its pixels.  feat0, feat1
 * (n_pix, C) f16, C a multiple of 8, 16-byte aligned; lin_w: C fp32 (the
 * non-negative 1 x 1 `lin` weights).  Per pixel, fp32, every operation rounded
 * on its own: s = sum_c f_c^2, den = sqrt(s) + 1e-10, n_c = f_c / den (a
 * division) for both images, d = sum_c w_c (n0_c - n1_c)^2; a pixel whose
 * features are all zero gives n = 0 / 1e-10 = 0.  The channel sums run in a
 * fixed order (eight interleaved partial sums of every eighth group of 8
 * channels, then a fixed tree).  out_sum (one device double, written) = the
 * sum of d over the pixels: per-block partials added in a fixed order in
 * double (divide by n_pix for the tap's term).  Equal features give exactly
 * 0.  work: RN_METRICS_WORK_BYTES of device scratch, as rn_image_sse.         */
int rn_lpips_prepare(const float* rgb, int64_t n_pix, void* out_f16, void* stream);
int rn_conv3x3_relu_f16(const void* in, const void* wfrag, const float* bias, int32_t n_img,
                        int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* out,
                        void* stream);
int rn_maxpool2_f16(const void* in, int32_t n_img, int32_t H, int32_t W, int32_t C, void* out,
                    void* stream);
int rn_lpips_layer(const void* feat0, const void* feat1, const float* lin_w, int64_t n_pix,
                   int32_t C, void* work, double* out_sum, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RADNERF_H */
