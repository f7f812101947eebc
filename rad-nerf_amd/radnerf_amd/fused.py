"""Fused Rad-NeRF training render: the whole hot path of ml_render
(models/ml_rendering.py:11-78 + :158-202) for all K sub-NeRFs as a fixed
chain of HIP launches with no host synchronisation:

  forward : gate_fwd (side stream) | ml_march_count (single pass, staged)
            -> scan_segments -> ml_compact
            -> field_fwd (all K models, compact samples) -> ml_composite_fw
            -> ml_combine_fw
  backward: ml_combine_bw -> ml_composite_bw -> field_bwd -> gate_bwd

Routed training (opt-in: gate_topk / gate_min / renormalize, DESIGN.md §4
"Routed training") marches and differentiates the gate's live pairs only:

  forward : gate_fwd -> gate_select (side stream) -> ml_march_count_list
            -> ... the same chain, the combine weighted by gate_used
  backward: ml_combine_bw -> gate_select_bw (+ the seed on the softmax gate)
            -> the same chain, the composite backward weighted by gate_used

Sample buffers are sized for the worst case (B*K*max_samples, + alignment),
so sample counts never have to be read back; every kernel consumes the
device-side counts.  Outputs equal the unfused drop-in path (rendering.py)
for the same noise (tests/test_gpu_parity.py).
"""
import collections

import torch

from . import layout as LY
from . import sparse_gate
from ._lib import GATE_SELECT_WORK_BYTES, lib
from .networks import field_ptrs, model_bitfields

MAX_SAMPLES = 1024
NEAR_DISTANCE = 0.01
SEG_ALIGN = 128
FX_STATS_BYTES = 640      # include/radnerf.h RN_FX_STATS_BYTES
# rn_field_bwd_merged's fx_mode, named as csrc/rn_gradform.h's GM_*: fp32 atomics
# (exact integer with the integer triple), fixed point, the fp32 redo of a
# flagged step, binned, binned with levels 0-7 by fp32 atomics ...
GM_F32, GM_FX, GM_FX_REDO, GM_BIN, GM_BIN_F32 = 0, 2, 3, 4, 5
# ... and its tail arguments for a form not in use: the integer triple (lo,
# carry, scale), the fx tuple (acc, scale, stats, redo, fx_mode), the page pool
NO_IG, NO_FX, NO_GB = (None, None, None), (None, None, None, None, GM_F32), (None, None, None, 0)


# GbCtl (csrc/rn_bin.h) words read back after each binned backward: pool_next
# (word 0) ... sum_fault (word 18, sticky across steps)
GB_SUM_FAULT = 18
GB_CTL_READ = GB_SUM_FAULT + 1


def clamp_split(split_level):
    """The binned fold's level cut for the data-parallel hook schedule, in
    [0, 15]: levels [cut, 16) are summed first and handed to
    after_grid_levels, then [0, cut).  0 sums the whole grid at once; 16
    would leave the first sum empty and release the grid before any level
    was summed, so it is clamped to 15."""
    return max(0, min(15, int(split_level)))


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# per (device, stream): forward scratch shared by every workspace (level_buffers)
_LEVEL_SCRATCH = {}


def route_params(fn, G, gate_topk=None, gate_min=0.0, renormalize=False, always=False):
    """The routing of a training step over G gated sub-NeRFs from its three
    arguments (sparse_gate's rule): None for the dense chain -- one sub-NeRF,
    or every pair kept (gate_topk None or G, gate_min 0) without
    renormalisation and `always` off -- else (gate_topk, gate_min,
    renormalize), checked.  ValueError naming the argument and its value;
    touches no library."""
    if G == 1:              # nothing to route: the arguments are accepted and ignored
        return None
    tau, k = sparse_gate.check_params(fn, G, gate_min, gate_topk)
    renorm = bool(renormalize)
    if sparse_gate.is_dense(G, tau, k) and not renorm and not always:
        return None
    return k, tau, renorm


def check_depth_weights(fn, lambda_depth=0.0, lambda_depth_var=0.0, depth_clip=float("inf")):
    """The depth terms' weights and clip: whether any term is on.  ValueError
    naming the argument for a negative or NaN lambda or a clip that is not > 0
    (inf: no clip)."""
    for name, lam in (("lambda_depth", lambda_depth), ("lambda_depth_var", lambda_depth_var)):
        if not float(lam) >= 0.0:
            raise ValueError(f"{fn}: {name} must be >= 0, got {lam!r}")
    if not float(depth_clip) > 0.0:
        raise ValueError(f"{fn}: depth_clip must be > 0 (inf: no clip), got {depth_clip!r}")
    return float(lambda_depth) > 0.0 or float(lambda_depth_var) > 0.0


def check_depth_args(fn, n_rays, target, lambda_depth=0.0, lambda_depth_var=0.0,
                     depth_clip=float("inf"), device=None):
    """The depth supervision of a step from its arguments: whether any term is
    on.  ValueError for what check_depth_weights refuses, a lambda > 0 without
    targets, targets that are not (n_rays,) fp32 or -- with `device`, the rays'
    -- not on it (the kernels take device pointers); any stride is accepted,
    the callers make the targets contiguous.  Touches no library and allocates
    nothing."""
    on = check_depth_weights(fn, lambda_depth, lambda_depth_var, depth_clip)
    if on and target is None:
        raise ValueError(f"{fn}: lambda_depth / lambda_depth_var > 0 need depth targets "
                         "(one ray parameter per ray; <= 0 where there is no measurement)")
    if target is not None:
        if not torch.is_tensor(target) or tuple(target.shape) != (int(n_rays),) \
                or target.dtype != torch.float32:
            raise ValueError(f"{fn}: depth targets must be a ({int(n_rays)},) fp32 tensor, got "
                             f"{tuple(target.shape) if torch.is_tensor(target) else type(target)}"
                             f"{' ' + str(target.dtype) if torch.is_tensor(target) else ''}")
        if device is not None and target.device != torch.device(device):
            raise ValueError(f"{fn}: depth targets must be on the rays' device {device}, got "
                             f"{target.device}")
    return on


class Workspace:
    """Persistent device buffers for one (B, K) configuration."""

    def __init__(self, n_rays, n_models, device, max_samples=MAX_SAMPLES, capacity=None):
        B, K = n_rays, n_models
        self.B, self.K, self.device = B, K, device
        cap = capacity or (B * K * max_samples + SEG_ALIGN * K)
        self.capacity = cap
        f = dict(device=device, dtype=torch.float32)
        i = dict(device=device, dtype=torch.int32)
        self.counts = torch.empty(K, B, **i)
        self.offsets = torch.empty(K, B, **i)
        self.seg = torch.zeros(2 * K + 2, **i)      # seg_base[K] | seg_count[K] | meta[2]
        self.used = torch.empty(K, B, **i)
        self.ts = torch.empty(cap, **f)
        self.deltas = torch.empty(cap, **f)
        self.ray_of = torch.empty(cap, **i)
        self.sigma = torch.empty(cap, **f)
        self.rgb = torch.empty(cap, 3, **f)
        self.ws = torch.empty(cap, **f)
        self.dsigma = torch.empty(cap, **f)
        self.drgb = torch.empty(cap, 3, **f)
        self.opacity_k = torch.empty(K, B, **f)
        self.depth_k = torch.empty(K, B, **f)
        self.rgb_k = torch.empty(K, B, 3, **f)
        self.dgate = torch.empty(B, K, **f)
        # single-pass march staging: max_samples slots per (model, ray)
        self.stage_ts = torch.empty(K * B * max_samples, **f)
        self.stage_dt = torch.empty(K * B * max_samples, **f)
        # field fwd -> bwd encoding cache: 32 f16 per sample slot (64 B)
        self.feat = torch.empty((cap + 31) // 32 * 32, 32, device=device, dtype=torch.float16)
        # merged backward (rn_bwd_plan): per-ray merged starts, merged order, queue head
        self.mstart = torch.empty(B + 1, **i)
        self.perm = torch.empty(cap, **i)
        self.queue = torch.zeros(3, **i)
        self._bwd_scratch = None
        self._chunks = self._chunk_desc = None
        self._dist_k = None         # per-segment distortion loss (distortion steps only)
        self._dvar_k = None         # per-segment depth second moment (depth steps only)
        # allocated by the first backward that needs them: integer-grid and
        # fixed-point state (fx_i: the current scale row), the binned scatter's
        # pool and read-back ring, the deterministic slots, the input gradients
        self._igrad = self._fx = self._bin = self._bin_ring = None
        self.fx_i = self._bin_n = 0
        self.dw_part = self.gate_part = None
        self.gate_dx = self.dxyz = self.ddir = self.drays_o = self.drays_d = None
        self.generation = 0         # forwards run through this workspace (_MLRenderFn)
        self._route = None          # routed steps only (route_buffers)

    def route_buffers(self):
        """rn_gate_select's outputs for a routed step, allocated by the first
        one: live / gate_used (B, K), list (K, B), count (K,) and the
        selection's scratch.  They belong to the workspace generation: the
        backward of a routed forward reads live and gate_used from here."""
        if self._route is None:
            B, K, dev = self.B, self.K, self.device
            self._route = dict(
                live=torch.empty(B, K, device=dev, dtype=torch.uint8),
                gate_used=torch.empty(B, K, device=dev, dtype=torch.float32),
                list=torch.empty(K, B, device=dev, dtype=torch.int32),
                count=torch.zeros(K, device=dev, dtype=torch.int32),
                work=torch.empty(GATE_SELECT_WORK_BYTES, device=dev, dtype=torch.uint8))
        return self._route

    @property
    def dist_k(self):
        """[K][B] distortion loss per (sub-NeRF, ray) segment, written by
        rn_ml_composite_dist_fw and read by its backward; allocated by the
        first distortion step."""
        if self._dist_k is None:
            self._dist_k = torch.empty(self.K, self.B, device=self.device, dtype=torch.float32)
        return self._dist_k

    @property
    def dvar_k(self):
        """[K][B] second moment of each (sub-NeRF, ray) segment's weights about
        the ray's depth target, written by rn_ml_composite_depth_fw and read
        by its backward; allocated by the first depth-supervised step."""
        if self._dvar_k is None:
            self._dvar_k = torch.empty(self.K, self.B, device=self.device, dtype=torch.float32)
        return self._dvar_k

    def chunk_list(self, max_chunk, min_chunk, head_chunks=0, balance_blocks=0):
        """rn_bwd_plan's chunk list, sized for the workspace capacity."""
        # include/radnerf.h's bound (the tail after the last big chunk can
        # hold up to max_chunk more samples in min_chunk pieces)
        cap = (head_chunks + self.capacity // max_chunk + self.capacity // (8 * min_chunk) +
               max_chunk // min_chunk + 3 + balance_blocks)
        if self._chunks is None or self._chunks.numel() < cap + 1:
            self._chunks = torch.empty(cap + 1, device=self.device, dtype=torch.int32)
            self._chunk_desc = torch.empty(cap + 1, 20, device=self.device, dtype=torch.int32)
        return cap, self._chunks

    def level_buffers(self, stream=None):
        """rn_field_fwd_levels' per-level encoding planes (16 x f16x2 per
        sample slot, 64 B) and merged-order unit coordinates (16 B).  They are
        scratch of one forward (written by the encode, read by the MLP
        tiles), so the workspaces of a device share one pair per stream,
        grown to the largest (80 B per slot in every workspace
        was ~40 % of a workspace)."""
        rows = self.feat.shape[0]
        key = (str(self.device), int(stream) if stream is not None else 0)
        cur = _LEVEL_SCRATCH.get(key)
        if cur is None or cur[0].shape[1] < rows:
            cur = (torch.empty(16, rows, device=self.device, dtype=torch.int32),
                   torch.empty(rows, 4, device=self.device, dtype=torch.float32))
            _LEVEL_SCRATCH[key] = cur
        return cur

    def fx_buffers(self, n, device):
        """Fixed-point grid-gradient state (rn_grid_fx_fold): int32 sums (n,
        zero between steps), per-level scales (2, 16) (current / next, swapped
        by fx_i each step; zeros = fp32 until the first step has measured the
        records), the per-level statistics block (FX_STATS_BYTES: record
        maxima, plain and weighted record / entry sums; include/radnerf.h)
        and the redo flag."""
        if self._fx is None or self._fx[0].numel() != n:
            z = dict(device=device, dtype=torch.int32)
            self._fx = (torch.zeros(n, **z), torch.zeros(2, 16, device=device),
                        torch.zeros(FX_STATS_BYTES // 4, **z), torch.zeros(1, **z))
            self.fx_i = 0
        return self._fx

    def bin_pool(self, pages):
        """Page pool of the binned grid-gradient scatter (fx_mode 4,
        rn_grid_binned_fold; csrc/rn_bin.h): control block, page levels /
        fills, the pages (u64 records; the bin pass sorts each page in place),
        per-page slice runs, per-level page lists (a step that overflows the
        pool is redone in fp32; _bin_pool grows it from the counts the
        backwards read back)."""
        b = self._bin
        if b is None or b["pages"] < pages:
            lay = lib().bin_layout()
            i = dict(device=self.device, dtype=torch.int32)
            self._bin = b = dict(
                pages=pages, page=lay["page"],
                ctl=torch.zeros(lay["ctl_bytes"] // 4, **i),
                meta=torch.zeros(pages, **i),
                recs=torch.empty(pages * lay["page"], device=self.device, dtype=torch.int64),
                desc=torch.empty(pages * lay["bins"], **i),
                lpages=torch.empty(16 * pages, **i))
        return b

    def bwd_scratch(self, blocks, max_chunk, max_samples=MAX_SAMPLES):
        """Per-block row scratch and dW park area of rn_field_bwd_merged."""
        rows = max_chunk + self.K * max_samples
        key = (blocks, rows)
        if self._bwd_scratch is None or self._bwd_scratch[0] != key:
            f = dict(device=self.device, dtype=torch.float32)
            self._bwd_scratch = (key, torch.empty(blocks * rows * 20, **f),
                                 torch.empty(blocks * self.K * 8 * 2048, **f))
        return rows, self._bwd_scratch[1], self._bwd_scratch[2]

    @property
    def seg_base(self):
        return self.seg[: self.K]

    @property
    def seg_count(self):
        return self.seg[self.K: 2 * self.K]

    @property
    def meta(self):
        return self.seg[2 * self.K:]

    def n_samples(self):
        """Total marched samples (reads back: diagnostics only)."""
        return int(self.meta[1].item())


class FusedMLRenderer:
    """Owns the workspace and runs the fused forward / backward chains."""

    def __init__(self, model, gating_net, n_rays, device=None, fwd_blocks=None, bwd_blocks=None,
                 capacity=None, deterministic=False):
        """deterministic=True: bitwise-reproducible steps (DESIGN.md §4
        "Deterministic training").  On one GPU in one process the same
        parameters, inputs and seed then give the same gradients, loss terms
        and outputs whatever the order blocks and waves run in: the merged
        backward takes its chunks on a static schedule and writes per-block dW
        slots (rn_field_bwd_merged_det, the integer-grid form), the gate
        backward per-block slots too (rn_gate_bwd_det), both summed in slot
        order (rn_reduce_partials); the gate importance and the loss terms are
        ordered sums (rn_colsum_ordered, rn_nerf_loss_det).  ValueError above 8
        sub-NeRFs or with merged_bwd off (the per-model backward scatters with
        fp32 atomics).  Under data parallelism each rank's local gradient is
        reproducible; the order of the collective's sum is RCCL's."""
        self._deterministic = self._merged_bwd = False
        if deterministic and not 1 <= model.size <= 8:
            # refused before the workspace is allocated
            raise ValueError(self._NO_DET + f" (this model: {model.size} sub-NeRFs)")
        self.model, self.gate = model, gating_net
        self.device = device or model.mlp_params.device
        self.ws = Workspace(n_rays, model.size, self.device, capacity=capacity)
        K = model.size
        self.bitfield_bytes = model_bitfields(model)[0].numel()
        self.fwd_blocks = fwd_blocks or max(1, 2048 // K)
        self.bwd_blocks = bwd_blocks or max(1, 256 // K)
        self.feat_cache = True      # field fwd stores the encoding, bwd skips the re-gather
        # backward scatters the K models' grid gradients merged per ray
        # (rn_field_bwd_merged); False: one model per block (rn_field_bwd)
        # (K = 1 too: its row-lane walk beats the per-model kernel, step 3.60 vs
        # 3.74 ms, profiles/r01/step_variants_k1.json)
        self.merged_bwd = 1 <= model.size <= 8      # rn_field_bwd_merged: K <= 8
        # forward evaluating the K models' tiles of a chunk interleaved
        # (rn_field_fwd_merged, K <= 8; bit-exact with rn_field_fwd).  One
        # block per CU keeps a chunk's rays in that CU's L1, so the second
        # model's corners hit lines the first fetched: C3 1.12 ms vs 1.30 ms
        # before the merged-order encode (tools/fwd_blocks_sweep.py; 2 blocks
        # per CU 1.17, 3 x 4 waves 1.35)
        # (K > 4: the MLP fragments are read from global memory instead of LDS)
        # (K = 1: the per-model kernel, 3.72 vs 3.74 ms per step)
        self.merged_fwd = 1 < model.size <= 8
        # merged forward: encode each chunk in merged (ray, t, model) order
        # first (tiles mixing the sub-NeRFs of a ray stretch share more grid
        # lines: 20.9 vs 28.2 per sample, tools/fwd_lines_sim.py), then the
        # per-model MLP tiles read the encoding cache.  C3: field_fwd 1.095 ->
        # 1.03 ms.  One sub-NeRF has nothing to interleave.
        self.merged_encode = model.size > 1
        self.merged_fwd_blocks = 256
        # 16 waves: with the merged-order encode, C3 step 5.13 ms vs 5.16 at 8
        # (tools/step_variants.py, profiles/r01/step_variants_fwd_shape.json)
        self.merged_fwd_threads = 1024
        # level-partitioned forward (rn_field_fwd_levels): each XCD encodes two
        # levels of every sample, so its L2 holds two levels' tables instead of
        # sixteen; bit-exact with the merged forward (tools/enc_probe.py).
        # bench.py A/B (profiles/r03/lv_*_a1.json): C2 802 -> 853, C3 1098 ->
        # 1139, C4 401 -> 450, C5 513 -> 549 M samples/s.  Needs the plan's
        # merged order (rn_bwd_plan runs with the merged backward or forward).
        self.level_fwd = self.merged_bwd or self.merged_fwd
        # the plan writes the level forward's per-position input (no prep pass)
        self.plan_prep = True
        self.level_enc_blocks = 4096
        self.level_mlp_blocks = 256
        self.merged_blocks = 256
        # chunk of merged samples per queue ticket: 1024 keeps a block's staged
        # rows L2-resident (C3 sweep: 768 3.94, 1024 3.88, 2048 3.92, 4096 4.05,
        # 8192 4.50 ms)
        # Small steps want more, smaller chunks (at least a few per block): C1
        # (K = 1, 1024 rays) 1024 -> 256 is 0.707 -> 0.618 ms per step, C2
        # (K = 1, 8192 rays) 512 = 1024 (tools/step_variants.py, r02)
        rk = n_rays * model.size
        self.max_chunk = 256 if rk <= 1024 else (512 if rk <= 4096 else 1024)
        # with the fixed-point scatter (cheaper requests) longer chunks pay at
        # scale 0.5 with several sub-NeRFs (fewer end-of-chunk ring flushes):
        # C3 step 1024 5.02, 1280 4.94, 1536 4.89, 1792 4.92 ms; K = 8 at
        # scale 16 (C5 per GPU) 1024 12.36, 2048 12.23 ms; K = 4 at scale 16
        # (C4 per GPU) keeps 1024 (3.82 vs 3.92 at 1536); K = 1 (C2) 512-1024
        # within 0.6 % (tools/step_variants.py, profiles/r02/step_variants_fx_chunk.json)
        # Round 5, with the big chunks balanced over the blocks (balance_chunks
        # below): longer chunks pay at K >= 4 (fewer model switches -- park /
        # unpark dW, reload weights -- and ring drains per sample): C5 per GPU
        # 2048 645, 4096 664, 6144 670, 8192 671-675; C4 1024 512, 2048 533,
        # 3072 535, 4096 537, 6144 422; C3 1024 1136, 1536 1158, 2048 1148
        # (profiles/r05/chunk3/); after the walk-step work of late round 5:
        # C5 6144 728, 8192 730, 12288 734.6, 16384 734.2; C4 3072 591, 4096
        # 589, 6144 468; C3 1024 1172, 1536 1182, 2048 1177 (profiles/r05/chunk5/)
        if model.size >= 8 and rk > 4096:
            self.max_chunk = 12288
        elif model.size >= 4 and rk > 4096 and float(model.scale) > 0.5:
            self.max_chunk = 4096
        elif model.size >= 2 and rk > 4096 and float(model.scale) <= 0.5:
            self.max_chunk = 1536
        # exact integer accumulation of the grid gradient (rn_seed_scale +
        # returning u32 atomics with carries + rn_igrad_to_f32): bitwise
        # reproducible grid gradients, but each issue waits for the previous
        # one's return (the compiler's vmcnt(0)): 4.33 vs 3.81 ms on C3, so the
        # default stays fp32 atomics (against today's fixed-point / binned
        # defaults, train steps: C3 4.73 vs 4.21 ms, C5 per GPU 11.65 vs 7.90;
        # tools/deterministic_step.py, profiles/deterministic/)
        self.int_grad = False
        # bitwise-reproducible steps (see __init__); the grid gradient then
        # takes the int_grad form whatever the switches below say
        self.deterministic = bool(deterministic)
        # fixed-point accumulation of the hashed levels' grid gradient (u32
        # adds, scale from the previous step's largest record, fp32 redo on
        # overflow; rn_grid_fx_fold): field_bwd C3 3.76 -> 3.50 ms, C4 per
        # GPU 3.29 -> 2.60, C5 10.54 -> 8.59 (tools/ablate.py, r02).  The
        # first backward of a workspace runs fp32 (no scale yet).  Its
        # bookkeeping (entry sums, check, fold over the whole table: 0.06 ms,
        # + 0.011 ms for the redo launch) is per step, not per sample: at C1's
        # 1024 rays x 1 sub-NeRF fp32 atomics win (494 vs 462 M samples/s),
        # from C2's 8192 rays on fixed point does (C2 800 vs 696, C3 1078 vs
        # 998; tools/gpu/fx_small.sh, profiles/r03/fx_small_r03.jsonl)
        self.grid_fx = rk > 1024
        # binned ("store and sum") scatter of the fixed-point records at scale
        # 16 (fx_mode 4 + rn_grid_binned_fold): the walk appends records to
        # pages with plain stores, a bin pass sorts each page by 4096-entry
        # slice, a sum pass adds each slice in LDS (int64, exact) -- instead
        # of memory-side atomics, which were 45 % of C5's field_bwd
        # (DESIGN §4 "Binned scatter")
        self.grid_bin = self.grid_fx and float(model.scale) > 0.5
        # binned mode: the coarse levels [0, n) go in by fp32 atomics instead
        # of page records.  A coarse record shares its 64-B request with its
        # neighbours (dense levels, the first hashed ones) and the walk hides
        # those atomics, while a page record costs 24 B of bin + sum traffic
        # (round 6, tools/level_bin_probe.py, profiles/r06/level_bin/): all
        # binned -> levels [0, n) fp32: C5 738 -> 763 M samples/s per GPU at
        # n = 9, C4 599 -> 640 at n = 8 (beyond, the atomics bind).  Those
        # levels' sums are then fp32 in arrival order (the fine levels' stay
        # exact int64); exact int64 sums with u64 atomics were measured too
        # and lost to fp32 (16-B entries double the requests of an x-pair;
        # DESIGN §4)
        self.bin_f32_levels = (9 if model.size >= 8 else 8) if self.grid_bin else 0
        # the int32 form's wrap checksums weight gradient element i by 4 i
        # (rn_gradform.h fx_weight), injective up to 2^28 elements: a larger table
        # (none of the reference's configs: 16 levels x 2^19 entries x 2
        # features = 2^24) keeps fp32 atomics unless it is binned (no checksum)
        if not self.grid_bin and model.xyz_encoder.params.numel() > (1 << 28):
            self.grid_fx = False
        # initial pool: records per (ray, sub-NeRF) at scale 16 (C5's replay:
        # 63.5 records x 95 samples; tools/records_sim.py), x 1.15
        self.bin_records_per_pair = 6912
        # the tail's chunks (the last 1/16 of the merged positions; 1/8 until
        # late round 6, where these sweeps ran): small
        # enough for the blocks to finish together, large enough that a
        # chunk's fixed cost -- K model switches (weights, parked dW) and ring
        # flushes -- stays small.  Round 6, interleaved (profiles/r06/minchunk/):
        # C3 256 1182, 384 1189, 512 1188, 768 1179; C5 512 774, 1024 782,
        # 2048 780, 3072 789, 3584 786, 4096 781; C4 512 649, 640 648, 768 642,
        # 1024 651.5, 2048 623; the pinned rank 512 581, 1024 578, 2048 578.
        # (At C5 3072 leaves ~250 tail chunks, at most one per block; the
        # optimum moves with the step's size, so the rule holds from the
        # measured ray counts up.)
        self.min_chunk = 512
        if float(model.scale) > 0.5:
            if model.size >= 8 and n_rays >= 8192:
                # with the 1/16 tail: 1536 791 vs 3072 784 (profiles/r06/tail/)
                self.min_chunk = 1536
            # (K = 4: 1024 won with the 1/8 tail; with 1/16, 512: 658 vs 653)
        # hash levels whose grid gradient goes in by fp32 atomics instead of
        # fixed point (int32 or binned): () = none, every level an exact
        # integer sum (bitwise reproducible).  (3, ..., 8) at C3 brings the
        # per-entry 3-step Adam difference from fp32 from 1.1 % to 0.3 %
        # (levels 3-8 hold most of the int32 form's flushed entries) at the
        # cost of those levels' reproducibility (bench.py
        # --fx-f32-levels)
        self.fx_f32_levels = ()
        # head chunks: the first chunk of each block ramps from ~0 to
        # head_chunk merged samples (rn_bwd_plan), so the blocks' walks start
        # staggered instead of all after one full MLP phase.  Round 6
        # (profiles/r06/headramp/, interleaved): a ramp to max_chunk at scale
        # 0.5, C3 1183.4 -> 1189.2 M samples/s, C2 853.7 -> 862.3, C1 within
        # noise (then 256); at scale 16 a ramp to max_chunk / 2 cost C4 650 ->
        # 617 and C5 773 -> 762 (only ~2 big chunks per block, which get
        # shorter), so none there.  (Head chunks of one size, rounds 2 and 5,
        # changed nothing.)
        self.head_chunk = self.max_chunk if float(model.scale) <= 0.5 and rk > 1024 else 0
        # big chunks a multiple of the persistent blocks in number (rn_bwd_plan
        # balance_blocks): every block takes the same number of them
        self.balance_chunks = True
        # gate backward on this process (pinned.PinnedMLRenderer: rank 0 only),
        # and where: "field" side stream beside field_bwd, "early" side stream
        # beside composite_bw, "main" in line before field_bwd
        self.gate_grad_here = True
        # "early": beside composite_bw, before field_bwd's persistent blocks
        # occupy every CU (beside field_bwd it waited for them: its events
        # spanned 1.3-3.7 ms for a 0.09 ms kernel).  C3 step: early 5.037,
        # field 5.045, main 5.117 ms (tools/step_variants.py, r02)
        self.gate_bwd_at = "early"
        # input gradients (dL/drays_o, dL/drays_d) in backward(): set by
        # _MLRenderFn when the rays require grad (--optimize_ext)
        self.input_grad = False
        # called right after the merged field_bwd launch (stream order), when
        # the MLP gradient is final (data-parallel early all-reduce)
        self.after_field_bwd = None
        # called (stream order) when the grid gradient of levels
        # [grid_split_level, 16) -- the tail of the flat table, the fine hashed
        # levels -- is final, with grid_split_level as argument; the binned
        # fold then sums levels [0, grid_split_level), so a data-parallel
        # caller's collective of the fine levels overlaps it.  With the int32
        # fold (one short pass over every level) it is called with 0 after the
        # fold and the redo launch, when the whole table is final.
        self.after_grid_levels = None
        self.grid_split_level = 8
        # record HIP events around every launch (True) or the named ones (a set)
        self.trace = False
        self.events = {}
        # set as the chain runs: the plan's parameters and whether it wrote the
        # level forward's input, the gate's side stream, fx_f32_levels as a tensor
        self._plan_key = self._side_stream = None
        self._prep_ready = self._dist_forward = False
        self._depth_forward = None
        # measurement and tests only (tools/routed_step.py's all-live overhead
        # leg, the all-live identity test): run the routed launches (selection,
        # list march, routing backward) even when the arguments keep every pair
        # live; the product leaves it off, and such arguments take the dense
        # chain, launch for launch
        self._route_always = False
        # the last forward's routing: None (dense) or (gate_topk, gate_min,
        # renormalize) as checked; the backward follows it
        self._routed = None
        self._f32_idx = (None, None)

    # a layout that cannot supervise depth names the reason here (pinned.py)
    _NO_DEPTH = None

    _NO_DET = ("FusedMLRenderer(deterministic=True) needs the merged backward (1 to 8 sub-NeRFs, "
               "merged_bwd on): the per-model backward scatters the grid gradient and dW with "
               "fp32 atomics in arrival order")

    @property
    def merged_bwd(self):
        return self._merged_bwd

    @merged_bwd.setter
    def merged_bwd(self, on):
        if self._deterministic and not on:
            raise ValueError(self._NO_DET)
        self._merged_bwd = bool(on)

    @property
    def deterministic(self):
        return self._deterministic

    @deterministic.setter
    def deterministic(self, on):
        if on and not self._merged_bwd:
            raise ValueError(self._NO_DET + f" (this renderer: {self.model.size} sub-NeRFs, "
                             f"merged_bwd {self._merged_bwd})")
        self._deterministic = bool(on)

    @property
    def scatter_mode(self):
        """How the next backward accumulates the grid gradient, from the
        switches as they stand: "binned" (page records, bin + sum passes),
        "fixed-point" (int32 atomics + fold), "int-grad" (exact u32 atomics
        with carries) or "fp32-atomics".  grid_fx / grid_bin / int_grad only
        act in the merged backward (_field_bwd): the per-model backward
        (merged_bwd off, the default above 8 sub-NeRFs) always scatters with
        fp32 atomics, whatever they say."""
        if not self.merged_bwd:
            return "fp32-atomics"
        if self.int_grad or self.deterministic:
            return "int-grad"
        if self.grid_fx and self.feat_cache:
            return "binned" if self.grid_bin else "fixed-point"
        return "fp32-atomics"

    def _ev(self, name, L_call, *args, stream=None):
        """Launch through librn; with tracing on (for this kernel), bracket it
        with events on the launch stream (bench.py's per-kernel timing)."""
        if not self.trace or (self.trace is not True and name not in self.trace):
            return L_call(*args)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        L_call(*args)
        b.record(stream)
        self.events.setdefault(name, []).append((a, b))

    def _ev_open(self, name):
        """start one event span over several launches (closed by _ev_close)"""
        if not self.trace or (self.trace is not True and name not in self.trace):
            return None
        a = torch.cuda.Event(enable_timing=True)
        a.record()
        return (name, a)

    def _ev_close(self, span):
        if span is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.events.setdefault(span[0], []).append((span[1], b))

    def _side(self, dev):
        """Side stream for the gate MLP: it runs beside the march (forward) and
        beside field_bwd (backward), joined back before its outputs are used."""
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(dev)
        return self._side_stream

    def _f32_level_index(self, dev):
        key = (tuple(sorted(int(l) for l in self.fx_f32_levels)), str(dev))
        if self._f32_idx[0] != key:
            if any(not 0 <= l < 16 for l in key[0]):
                raise ValueError(f"fx_f32_levels: hash levels are 0..15, got {key[0]}")
            self._f32_idx = (key, torch.tensor(key[0], dtype=torch.int64, device=dev))
        return self._f32_idx[1]

    def kernel_times_ms(self):
        """{kernel: [ms per launch]} of the traced launches (synchronises)."""
        torch.cuda.synchronize()
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in self.events.items()}

    def bitfields(self):
        bf = model_bitfields(self.model)
        if all(b.data_ptr() == bf[0].data_ptr() + i * self.bitfield_bytes for i, b in enumerate(bf)):
            return bf[0]
        self._bf = torch.stack(bf).contiguous()
        return self._bf

    # ------------------------------------------------------------------ forward
    def route_params(self, gate_topk=None, gate_min=0.0, renormalize=False):
        """The routing of a step from its three arguments: None for the dense
        chain (one sub-NeRF, or every pair kept without renormalisation and
        _route_always off), else (gate_topk, gate_min, renormalize) checked.
        ValueError naming the argument and its value; no launch."""
        return route_params("FusedMLRenderer", self.gate.out_dim, gate_topk, gate_min,
                            renormalize, self._route_always)

    def forward(self, rays_o, rays_d, gate_in2, noise, bg, T_threshold=1e-4,
                exp_step_factor=0.0, distortion=False, gate_topk=None, gate_min=0.0,
                renormalize=False, depth_target=None, depth_clip=float("inf")):
        """depth_target ((B,) fp32: the ray parameter at which each ray should
        terminate, <= 0 where there is no measurement): the composite also
        writes each segment's second moment about it, sum w min((t - z)^2,
        depth_clip^2), into ws.dvar_k (rn_ml_composite_depth_fw; every other
        output is the plain kernel's -- with distortion, the distortion
        kernel's), for backward(dL_ddvar=...).
        distortion: the composite also writes each segment's Mip-NeRF 360
        distortion loss into ws.dist_k (rn_ml_composite_dist_fw; every other
        output is the plain kernel's), for backward(dL_ddist=...).
        gate_topk / gate_min / renormalize: routed training -- rn_gate_select's
        rule (sparse_gate) decides which (ray, sub-NeRF) pairs are live; only
        those are marched (a dead pair has no samples), and the render is
        combined with gate_used (ws.route_buffers()), which backward() then
        differentiates.  The returned gate stays the softmax.  The defaults
        keep every pair and run the dense chain."""
        m, g, w, L = self.model, self.gate, self.ws, lib()
        B, K, G = rays_o.shape[0], m.size, g.out_dim     # K rendered here, G gated
        assert B == w.B and noise.shape == (K, B)
        check_depth_args("FusedMLRenderer.forward", B, depth_target, depth_clip=depth_clip,
                         device=rays_o.device)
        routed = self._routed = self.route_params(gate_topk, gate_min, renormalize)
        st = _stream(rays_o.device)
        out_gate = torch.empty(B, G, device=rays_o.device)
        imp = torch.zeros(G, device=rays_o.device)
        side = self._side(rays_o.device)
        main = torch.cuda.current_stream(rays_o.device)
        if G == 1:
            # softmax over one sub-NeRF is exactly 1 (and its gradient exactly
            # 0): single-NGP configs C1 / C2 skip the gate MLP
            out_gate.fill_(1.0)
            imp.fill_(float(B))
            side.wait_stream(main)
        else:
            frags = g.packed_frags()          # (re)packed on the main stream
            side.wait_stream(main)
            self._ev("gate_fwd", L.gate_fwd, rays_o.data_ptr(), gate_in2.data_ptr(), 3, B, G,
                     frags.data_ptr(), out_gate.data_ptr(),
                     None if self.deterministic else imp.data_ptr(),
                     max(1, min(256, (B + 127) // 128)), side.cuda_stream, stream=side)
            if self.deterministic:
                # gate.sum(0) as an ordered sum instead of one atomic per wave
                self._ev("gate_colsum", L.colsum_ordered, out_gate.data_ptr(), B, G,
                         imp.data_ptr(), side.cuda_stream, stream=side)
        rt = None
        if routed is not None:
            # the selection follows the gate on its stream; the march needs the lists
            rt = w.route_buffers()
            self._ev("gate_select", L.gate_select, out_gate.data_ptr(), B, G, routed[1],
                     routed[0], int(routed[2]), rt["live"].data_ptr(),
                     rt["gate_used"].data_ptr(), rt["list"].data_ptr(), rt["count"].data_ptr(),
                     None, None, None, None, rt["work"].data_ptr(), side.cuda_stream,
                     stream=side)
            main.wait_stream(side)
        bits = self.bitfields()
        march = (rays_o.data_ptr(), rays_d.data_ptr(), m.center.data_ptr(),
                 m.half_size.data_ptr(), NEAR_DISTANCE, noise.data_ptr(), bits.data_ptr(),
                 self.bitfield_bytes, K, m.cascades, float(m.scale), float(exp_step_factor),
                 m.grid_size, MAX_SAMPLES, B)
        # single pass: march once into per-(model, ray) staging slots, scan the
        # counts, compact (the two-pass form re-marches every ray instead)
        if rt is None:
            self._ev("march", L.ml_march_count, *march, w.counts.data_ptr(),
                     w.stage_ts.data_ptr(), w.stage_dt.data_ptr(), st)
        else:
            self._ev("march", L.ml_march_count_list, *march, w.counts.data_ptr(),
                     w.stage_ts.data_ptr(), w.stage_dt.data_ptr(), rt["list"].data_ptr(),
                     rt["count"].data_ptr(), st)
        self._ev("scan", L.scan_segments, w.counts.data_ptr(), K, B, SEG_ALIGN,
                 w.offsets.data_ptr(), w.seg_base.data_ptr(), w.seg_count.data_ptr(),
                 w.meta.data_ptr(), st)
        self._ev("compact", L.ml_compact, w.counts.data_ptr(), w.offsets.data_ptr(), B, K,
                 MAX_SAMPLES, w.stage_ts.data_ptr(), w.stage_dt.data_ptr(), w.ts.data_ptr(),
                 w.deltas.data_ptr(), w.ray_of.data_ptr(), st)
        if self.merged_bwd or self.merged_fwd:
            # the plan also writes the level forward's per-position input
            self._plan(st, rays_o, rays_d if self.level_fwd and self.plan_prep else None)
        self._field_fwd(rays_o, rays_d, st)
        comp = (w.sigma.data_ptr(), w.rgb.data_ptr(), w.deltas.data_ptr(),
                w.ts.data_ptr(), w.counts.data_ptr(), w.offsets.data_ptr(), B, K,
                float(T_threshold), w.used.data_ptr(), w.opacity_k.data_ptr(),
                w.depth_k.data_ptr(), w.rgb_k.data_ptr(), w.ws.data_ptr())
        self._dist_forward = bool(distortion)       # dist_k holds this step's losses
        # dvar_k holds this step's moments about (target, clip)
        self._depth_forward = None
        if depth_target is not None:
            depth_target = depth_target.contiguous()
            self._depth_forward = (depth_target, float(depth_clip))
            self._ev("composite_depth_fw", L.ml_composite_depth_fw, *comp,
                     depth_target.data_ptr(), float(depth_clip),
                     w.dist_k.data_ptr() if distortion else None, w.dvar_k.data_ptr(), st)
        elif distortion:
            self._ev("composite_dist_fw", L.ml_composite_dist_fw, *comp, w.dist_k.data_ptr(), st)
        else:
            self._ev("composite_fw", L.ml_composite_fw, *comp, st)
        # per-ray outputs of all G gated sub-NeRFs (here: the K rendered ones;
        # pinned.PinnedMLRenderer gathers them from every rank)
        ok, dk, rk = self._gather_model_outputs()
        rgb = torch.empty(B, 3, device=rays_o.device)
        opacity = torch.empty(B, device=rays_o.device)
        depth = torch.empty(B, G, device=rays_o.device)
        main.wait_stream(side)            # gate output joins here
        out_gate.record_stream(side)
        imp.record_stream(side)
        weights = out_gate if rt is None else rt["gate_used"]
        self._ev("combine_fw", L.ml_combine_fw, weights.data_ptr(), ok.data_ptr(), dk.data_ptr(),
                        rk.data_ptr(), bg.data_ptr(), B, G, rgb.data_ptr(),
                        opacity.data_ptr(), depth.data_ptr(), st)
        return rgb, opacity, depth, out_gate, imp

    def _gather_model_outputs(self):
        """(opacity, depth, rgb) per (sub-NeRF, ray) of every gated sub-NeRF,
        after this step's composite (forward)."""
        return self._model_outputs()

    def _model_outputs(self):
        """The same, as the forward left them (backward)."""
        w = self.ws
        return w.opacity_k, w.depth_k, w.rgb_k

    def _local_cols(self, x):
        """Columns of a (B, G) per-ray tensor that belong to the rendered sub-NeRFs."""
        return x

    def _plan_params(self):
        """rn_bwd_plan's chunk parameters from the switches as they stand:
        (max_chunk, min_chunk, head chunks, head size, balance blocks)."""
        return (self.max_chunk, min(self.min_chunk, self.max_chunk),
                self.merged_blocks if self.head_chunk else 0,
                min(self.head_chunk, self.max_chunk),
                self.merged_blocks if self.balance_chunks else 0)

    def _plan(self, st, rays_o=None, rays_d=None):
        """Merged (ray, t) order + chunk schedule of this step's samples
        (rn_bwd_plan), shared by the merged forward and backward; with the
        rays (forward, level-partitioned encode) also the encode's
        per-position input, so rn_field_fwd_levels skips its prep pass."""
        w, L, m = self.ws, lib(), self.model
        prep = w.level_buffers(st)[1] if rays_d is not None else None
        key = max_chunk, min_chunk, head_n, head, bal = self._plan_params()
        self._cap_chunks, self._chunks = w.chunk_list(max_chunk, min_chunk, head_n, bal)
        self._ev("bwd_plan", L.bwd_plan, w.counts.data_ptr(), w.offsets.data_ptr(),
                 w.seg_base.data_ptr(), w.seg_count.data_ptr(), w.ts.data_ptr(), w.B, w.K,
                 head_n, head, max_chunk, min_chunk, bal, self._cap_chunks,
                 w.mstart.data_ptr(), w.perm.data_ptr(), self._chunks.data_ptr(),
                 w._chunk_desc.data_ptr(), w.queue.data_ptr(),
                 *((None,) * 5 if prep is None else
                   (rays_o.data_ptr(), rays_d.data_ptr(), m._h_min.ctypes.data,
                    m._h_ext.ctypes.data, prep.data_ptr())), st)
        self._plan_key = key
        self._prep_ready = prep is not None

    def _sample_ptrs(self, rays_o, rays_d):
        """The six compact-sample arguments of the field entries."""
        w = self.ws
        return (w.ts.data_ptr(), w.ray_of.data_ptr(), rays_o.data_ptr(), rays_d.data_ptr(),
                w.seg_base.data_ptr(), w.seg_count.data_ptr())

    def _field(self, fwd, rays_o, rays_d, st, grid_grad=None, dw=None):
        return (self._field_fwd(rays_o, rays_d, st) if fwd else
                self._field_bwd(rays_o, rays_d, st, grid_grad, dw))

    def _field_fwd(self, rays_o, rays_d, st):
        m, w, L = self.model, self.ws, lib()
        samples, grid = self._sample_ptrs(rays_o, rays_d), field_ptrs(m)
        out = (w.sigma.data_ptr(), w.rgb.data_ptr())
        feat = w.feat.data_ptr() if self.feat_cache else None
        if self.level_fwd and (self.merged_bwd or self.merged_fwd):
            planes, prep = w.level_buffers(st)
            self._ev("field_fwd", L.field_fwd_levels, *samples, w.B, m.size, *grid, *out,
                     w.feat.data_ptr(), w.mstart.data_ptr(), w.perm.data_ptr(),
                     planes.data_ptr(), planes.shape[1], prep.data_ptr(), int(self._prep_ready),
                     self.level_enc_blocks, self.level_mlp_blocks, None, st)
            self._prep_ready = False
        elif self.merged_fwd:
            order = ((w.mstart.data_ptr(), w.perm.data_ptr())
                     if self.feat_cache and self.merged_encode else (None, None))
            self._ev("field_fwd", L.field_fwd_merged, *samples, w._chunk_desc.data_ptr(),
                     w.queue.data_ptr(), w.B, m.size, *grid, *out, feat, *order,
                     self.merged_fwd_blocks, self.merged_fwd_threads, st)
        else:
            self._ev("field_fwd", L.field_fwd, None, None, 0, *samples, m.size, *grid, *out, feat,
                     self.fwd_blocks, st)

    def _field_bwd(self, rays_o, rays_d, st, grid_grad, dw):
        """One method per form of the grid-gradient scatter (scatter_mode), each
        from its set-up to its epilogue in stream order.  Each calls
        after_field_bwd when the MLP gradient (dW) is final -- a data-parallel
        caller starts the MLP / gate all-reduce there (bench.py) -- and
        after_grid_levels when the grid gradient (or its fine levels) is."""
        m, w, L = self.model, self.ws, lib()
        samples, grid = self._sample_ptrs(rays_o, rays_d), field_ptrs(m)
        feat = w.feat.data_ptr() if self.feat_cache else None
        if not self.merged_bwd:         # per-model backward: fp32 atomics only
            return self._bwd_f32(lambda name: self._ev(
                name, L.field_bwd, None, None, 0, *samples, m.size, *grid, w.dsigma.data_ptr(),
                w.drgb.data_ptr(), grid_grad.data_ptr(), dw.data_ptr(), feat, self.bwd_blocks, st))
        rows, scratch, park = w.bwd_scratch(self.merged_blocks, self.max_chunk)
        if self._plan_key != self._plan_params():
            self._plan(st)      # chunk sizes changed since the forward
        head = (*samples, w.mstart.data_ptr(), w.perm.data_ptr(), w._chunk_desc.data_ptr(),
                w.queue.data_ptr(), w.B, m.size, MAX_SAMPLES, *grid, w.dsigma.data_ptr(),
                w.drgb.data_ptr(), grid_grad.data_ptr())
        tail = (feat, scratch.data_ptr(), rows, park.data_ptr(), self.max_chunk, self.merged_blocks)

        def launch(name, ig=NO_IG, fx=NO_FX, gb=NO_GB, dw_part=None):
            # (dw_part: the deterministic entry, dW into the per-block slots)
            if dw_part is not None:
                self._ev(name, L.field_bwd_merged_det, *head, dw_part.data_ptr(), *tail, *ig, st)
            else:
                self._ev(name, L.field_bwd_merged, *head, dw.data_ptr(), *tail, *ig, *fx, *gb, st)

        form = {"int-grad": self._bwd_int, "fixed-point": self._bwd_fx,
                "binned": self._bwd_binned, "fp32-atomics": self._bwd_f32}[self.scatter_mode]
        form(launch, grid_grad, dw, st)

    @staticmethod
    def _hook(fn, *args):
        if fn is not None:
            fn(*args)

    def _bwd_f32(self, launch, *_):
        """fp32 atomics: dW and the whole grid gradient are final after the launch."""
        launch("field_bwd")
        self._hook(self.after_field_bwd)
        self._hook(self.after_grid_levels, 0)

    def _igrad_buffers(self, grid_grad):
        """Integer-grid state (rn_seed_scale, rn_igrad_to_f32): lo / carry words
        per gradient element (zero between steps), the step's scale and the
        scale's scratch word."""
        w, n_g = self.ws, grid_grad.numel()
        if w._igrad is None or w._igrad[0].numel() != n_g:
            z = dict(device=grid_grad.device, dtype=torch.int32)
            w._igrad = (torch.zeros(n_g, **z), torch.zeros(n_g, **z),
                        torch.ones(1, device=grid_grad.device), torch.zeros(1, **z))
        return w._igrad

    def _bwd_int(self, launch, grid_grad, dw, st):
        """Exact integer grid sums (order-free; int_grad).  Deterministic mode:
        the same with chunk c on block c mod merged_blocks, each block's dW in
        its own slot of ws.dw_part, the slots added into dw in block order."""
        m, w, L = self.model, self.ws, lib()
        lo, carry, scale, work = self._igrad_buffers(grid_grad)
        ig = (lo.data_ptr(), carry.data_ptr(), scale.data_ptr())
        det, slots = self.deterministic, (self.merged_blocks, m.size * LY.FIELD_PARAMS)
        if det and (w.dw_part is None or w.dw_part.shape != slots):
            w.dw_part = torch.empty(*slots, device=grid_grad.device)
        self._ev("seed_scale", L.seed_scale, w.seg_base.data_ptr(), w.seg_count.data_ptr(),
                 m.size, w.sigma.data_ptr(), w.dsigma.data_ptr(), w.drgb.data_ptr(),
                 work.data_ptr(), scale.data_ptr(), st)
        launch("field_bwd", ig=ig, dw_part=w.dw_part if det else None)
        if det:
            self._ev("dw_reduce", L.reduce_partials, w.dw_part.data_ptr(), *slots, dw.data_ptr(),
                     st)
        self._hook(self.after_field_bwd)
        # the grid gradient is final after its conversion into grid_grad
        self._ev("igrad_to_f32", L.igrad_to_f32, grid_grad.numel(), *ig, grid_grad.data_ptr(), st)
        self._hook(self.after_grid_levels, 0)

    def _fx_state(self, grid_grad, n32=0):
        """This step's fixed-point state (ws.fx_buffers; cur / nxt: the current
        and next scale rows).  fx_f32_levels and the binned form's coarse levels
        [0, n32) go in by fp32 atomics this step (a zero scale selects the
        kernel's per-level fp32 path)."""
        w = self.ws
        acc, scales, stats, redo = w.fx_buffers(grid_grad.numel(), grid_grad.device)
        cur, nxt = scales[w.fx_i], scales[1 - w.fx_i]
        if self.fx_f32_levels:
            cur.index_fill_(0, self._f32_level_index(cur.device), 0.0)
        if n32:
            cur[:n32].zero_()
        return acc, cur, nxt, stats, redo

    def _bwd_fx(self, launch, grid_grad, dw, st):
        """Fixed point (int32 atomics): the launch, the fold of the sums into
        grid_grad (or the flag for the fp32 redo) with the next step's scales,
        the redo launch."""
        w, L = self.ws, lib()
        lo, lh, lr, _ = self.model.xyz_encoder.level_ptrs()
        acc, cur, nxt, stats, redo = self._fx_state(grid_grad)
        launch("field_bwd", fx=(acc.data_ptr(), cur.data_ptr(), stats.data_ptr(), None, GM_FX))
        self._hook(self.after_field_bwd)
        self._ev("fx_fold", L.grid_fx_fold, lo, lh, lr, acc.data_ptr(), cur.data_ptr(),
                 nxt.data_ptr(), stats.data_ptr(), redo.data_ptr(), grid_grad.data_ptr(), st)
        # the fp32 redo of a flagged step's grid scatter: exits at once unless
        # the fold / check set the flag (no host synchronisation)
        launch("fx_redo", fx=(None, cur.data_ptr(), None, redo.data_ptr(), GM_FX_REDO))
        self._hook(self.after_grid_levels, 0)
        w.fx_i ^= 1

    def _bwd_binned(self, launch, grid_grad, dw, st):
        """Binned: the walk appends page records; bin the pages and check the
        step (a record past e5m17's range, a pool overflow or a refused input
        flags it for the fp32 redo), run the redo launch (the sums exit when
        flagged, so it can go first), then sum the fine levels, hand them to
        after_grid_levels (their all-reduce overlaps the rest) and sum the
        coarse levels."""
        w, L = self.ws, lib()
        lo, lh, _, _ = self.model.xyz_encoder.level_ptrs()
        n32 = max(0, min(16, int(self.bin_f32_levels)))
        acc, cur, nxt, stats, redo = self._fx_state(grid_grad, n32)
        pool = self._bin_pool(w)
        ctl, meta, recs, desc, lpages = (pool[k].data_ptr() for k in
                                         ("ctl", "meta", "recs", "desc", "lpages"))
        # GM_BIN_F32: levels 0-7 (the walk's even streams) are fp32 by
        # construction, so that walk carries no page code for them
        launch("field_bwd", fx=(None, cur.data_ptr(), stats.data_ptr(), None,
                                GM_BIN_F32 if n32 >= 8 else GM_BIN),
               gb=(ctl, meta, recs, pool["pages"]))
        self._hook(self.after_field_bwd)
        span = self._ev_open("fx_bin")
        L.grid_bin_check(lh, ctl, meta, recs, recs, desc, lpages, pool["pages"], cur.data_ptr(),
                         nxt.data_ptr(), stats.data_ptr(), redo.data_ptr(), st)
        self._ev_close(span)
        # the pages this backward took, read back without a sync (_bin_pool
        # reads it BIN_LAG backwards later): pool_next and the sum passes'
        # sticky fault word (GbCtl)
        seen = self._bin_seen(w)
        seen[0].copy_(pool["ctl"][:GB_CTL_READ], non_blocking=True)
        seen[1].record(torch.cuda.current_stream(grid_grad.device))
        launch("fx_redo", fx=(None, cur.data_ptr(), None, redo.data_ptr(), GM_FX_REDO))
        span = self._ev_open("fx_sum")
        # a split of 16 would hand the whole grid over before any level
        # is summed: the cut lies in [0, 15]
        split = clamp_split(self.grid_split_level) if self.after_grid_levels else 0
        sums = ((split, 16), (0, split)) if split > 0 else ((0, 16),)
        for i, (l0, l1) in enumerate(sums):
            L.grid_sum(lo, lh, ctl, desc, lpages, recs, pool["pages"], cur.data_ptr(),
                       redo.data_ptr(), grid_grad.data_ptr(), l0, l1, st)
            if i == 0 and split > 0:
                self.after_grid_levels(split)
        self._ev_close(span)
        if split == 0:
            self._hook(self.after_grid_levels, 0)
        w.fx_i ^= 1

    # pool growth reads the page count of the binned backward this many
    # backwards back, waiting for it if needed (reading whichever
    # count had arrived made the pool size -- and so which steps after an
    # overflow were binned and which redone in fp32 -- depend on host timing)
    BIN_LAG = 2

    def _bin_seen(self, w):
        """the next of BIN_LAG + 1 pinned (count, event) slots, in turn"""
        ring = w._bin_ring
        if ring is None:
            ring = w._bin_ring = [[torch.zeros(GB_CTL_READ, dtype=torch.int32, pin_memory=True),
                                   None, -1] for _ in range(self.BIN_LAG + 1)]
        slot = ring[w._bin_n % len(ring)]
        slot[1] = torch.cuda.Event()
        slot[2] = w._bin_n
        w._bin_n += 1
        return slot

    def _bin_pool(self, w):
        """The page pool for this backward: sized from the records per (ray,
        sub-NeRF) at first, then grown when the binned backward BIN_LAG
        backwards back took more than 7/8 of it (its count, read back
        asynchronously, is waited for here: a function of the step sequence,
        not of how far the host runs ahead)."""
        lay = lib().bin_layout()
        b = w._bin
        if b is None:
            # every wave keeps one page per level open (2 per wave of each
            # persistent block), so a step fills pages only partly at small sizes
            need = (-(-self.bin_records_per_pair * w.B * w.K // lay["page"]) +
                    2 * 8 * self.merged_blocks)
        else:
            need = b["pages"]
            ring, n = w._bin_ring, w._bin_n - self.BIN_LAG
            if ring is not None and n >= 0:
                slot = ring[n % len(ring)]
                if slot[2] == n and slot[1] is not None:
                    slot[1].synchronize()
                    if int(slot[0][GB_SUM_FAULT]) != 0:
                        raise RuntimeError(
                            "binned grid scatter: a sum pass refused a page run (GbCtl "
                            f"sum_fault {int(slot[0][GB_SUM_FAULT]):#x}) at or before the "
                            f"backward {self.BIN_LAG} steps back; that step's grid gradient "
                            "is incomplete (the page pool or its descriptors were corrupted)")
                    used = int(slot[0][0])
                    if used * 8 > need * 7:      # above 7/8: grow to 1.5x what was used
                        need = used * 3 // 2 + 64
        return w.bin_pool(need)

    # ----------------------------------------------------------------- backward
    def backward(self, rays_o, rays_d, gate_in2, gate, bg, dL_drgb, dL_dopacity, dL_ddepth,
                 dL_dgate_ext=None, T_threshold=1e-4, grid_grad=None, mlp_grad=None,
                 gate_grad=None, dL_ddist=None, dL_ddvar=None, dL_dgate_used=None):
        """Accumulates into grid_grad / mlp_grad / gate_grad (zero-initialised
        by the caller or allocated here) and returns them.  dL_ddist: the seed
        on the per-segment distortion loss of a forward(distortion=True) --
        a [K][B] fp32 tensor, or a number for the same seed on every segment;
        None runs the plain composite backward.  dL_ddvar: the seed on
        ws.dvar_k of a forward(depth_target=...), a [K][B] fp32 tensor
        (rn_ml_composite_depth_bw; with dL_ddist as well, both terms in one
        launch).  dL_dgate_used ((B, G), a routed step): a seed on the gate the
        render was combined with, added before the routing's backward;
        dL_dgate_ext stays the seed on the softmax gate."""
        m, g, w, L = self.model, self.gate, self.ws, lib()
        B, K, G = rays_o.shape[0], m.size, g.out_dim
        dev = rays_o.device
        st = _stream(dev)
        grid_grad = torch.zeros_like(m.xyz_encoder.params) if grid_grad is None else grid_grad
        mlp_grad = torch.zeros_like(m.mlp_params) if mlp_grad is None else mlp_grad
        gate_grad = torch.zeros_like(g.params) if gate_grad is None else gate_grad
        ok, _, rk = self._model_outputs()
        dgate = self._dgate(B, G)
        self._ev("combine_bw", L.ml_combine_bw, dL_drgb.data_ptr(), dL_dopacity.data_ptr(),
                 ok.data_ptr(), rk.data_ptr(), bg.data_ptr(), B, G, dgate.data_ptr(), st)
        if dL_dgate_used is not None:
            dgate.add_(dL_dgate_used)
        if self._routed is not None:
            # through gate_used = select(gate), the selection held constant:
            # dead pairs 0 (combine_bw leaves bg . dL_drgb there), live pairs
            # the renormalisation's gradient; `gate` is the softmax
            rt = w.route_buffers()
            self._ev("gate_select_bw", L.gate_select_bw, gate.data_ptr(), rt["live"].data_ptr(),
                     dgate.data_ptr(), B, G, int(self._routed[2]), dgate.data_ptr(), st)
            gate = rt["gate_used"]      # the composite backward's weights
        if dL_dgate_ext is not None:
            dgate.add_(dL_dgate_ext)
        side = self._side(dev)
        main = torch.cuda.current_stream(dev)

        gate_dx = self._gate_dinput(B, dev) if self.input_grad else None
        gate_dfr = g.packed_dinput_frags() if gate_dx is not None and G > 1 else None
        if gate_dx is not None and not self.gate_grad_here:
            gate_dx.zero_()             # no gate backward on this process

        def gate_bwd(stream):
            if G == 1:              # d softmax over one model = 0: nothing to add
                if gate_dx is not None:
                    gate_dx.zero_()
                return
            frags = g.packed_frags()
            if stream is side:
                side.wait_stream(main)
            n_blk = max(1, min(128, (B + 127) // 128))
            if self.deterministic:
                # one wave per block into the block's slot of ws.gate_part, the
                # slots added into gate_grad in block order, on the gate's stream
                n_par = gate_grad.numel()
                if w.gate_part is None or w.gate_part.shape != (n_blk, n_par):
                    w.gate_part = torch.empty(n_blk, n_par, device=dev)
                self._ev("gate_bwd", L.gate_bwd_det, rays_o.data_ptr(), gate_in2.data_ptr(), 3,
                         B, G, frags.data_ptr(), dgate.data_ptr(), w.gate_part.data_ptr(), n_par,
                         None if gate_dfr is None else gate_dfr.data_ptr(),
                         None if gate_dx is None else gate_dx.data_ptr(), n_blk,
                         stream.cuda_stream, stream=stream)
                self._ev("gate_reduce", L.reduce_partials, w.gate_part.data_ptr(), n_blk, n_par,
                         gate_grad.data_ptr(), stream.cuda_stream, stream=stream)
                return
            self._ev("gate_bwd", L.gate_bwd, rays_o.data_ptr(), gate_in2.data_ptr(), 3, B, G,
                     frags.data_ptr(), dgate.data_ptr(), gate_grad.data_ptr(),
                     gate_grad.numel(), None if gate_dfr is None else gate_dfr.data_ptr(),
                     None if gate_dx is None else gate_dx.data_ptr(),
                     n_blk, stream.cuda_stream, stream=stream)

        # gate backward: it only needs dL/dgate (combine_bw)
        gate_at = self.gate_bwd_at if self.gate_grad_here else None
        if gate_at == "early":          # side stream, beside composite_bw
            gate_bwd(side)
        gate_k = self._local_cols(gate)
        ddepth_k = None if dL_ddepth is None else self._local_cols(dL_ddepth)
        if dL_ddvar is not None:
            if self._depth_forward is None:
                raise RuntimeError("backward(dL_ddvar=...): the forward of this step ran "
                                   "without depth_target")
            if dL_ddist is not None and not self._dist_forward:
                raise RuntimeError("backward(dL_ddist=...): the forward of this step ran "
                                   "without distortion=True")
            assert dL_ddvar.shape == (K, B) and dL_ddvar.dtype == torch.float32 \
                and dL_ddvar.is_contiguous()
            target, clip = self._depth_forward
            seed = torch.is_tensor(dL_ddist)
            if seed:
                assert dL_ddist.shape == (K, B) and dL_ddist.dtype == torch.float32 \
                    and dL_ddist.is_contiguous()
            dist = dL_ddist is not None
            self._ev("composite_depth_bw", L.ml_composite_depth_bw, dL_drgb.data_ptr(),
                     dL_dopacity.data_ptr(), None if ddepth_k is None else ddepth_k.data_ptr(),
                     gate_k.data_ptr(), bg.data_ptr(), w.sigma.data_ptr(), w.rgb.data_ptr(),
                     w.deltas.data_ptr(), w.ts.data_ptr(), w.counts.data_ptr(),
                     w.offsets.data_ptr(), w.opacity_k.data_ptr(), w.depth_k.data_ptr(),
                     w.rgb_k.data_ptr(), target.data_ptr(), clip, dL_ddvar.data_ptr(),
                     w.dvar_k.data_ptr(), dL_ddist.data_ptr() if seed else None,
                     float(dL_ddist) if dist and not seed else 0.0,
                     w.ws.data_ptr() if dist else None, w.dist_k.data_ptr() if dist else None,
                     B, K, float(T_threshold), w.dsigma.data_ptr(), w.drgb.data_ptr(), st)
        elif dL_ddist is None:
            self._ev("composite_bw", L.ml_composite_bw, dL_drgb.data_ptr(), dL_dopacity.data_ptr(),
                     None if ddepth_k is None else ddepth_k.data_ptr(), gate_k.data_ptr(),
                     bg.data_ptr(), w.sigma.data_ptr(), w.rgb.data_ptr(),
                     w.deltas.data_ptr(), w.ts.data_ptr(), w.counts.data_ptr(),
                     w.offsets.data_ptr(), w.opacity_k.data_ptr(), w.depth_k.data_ptr(),
                     w.rgb_k.data_ptr(), B, K, float(T_threshold), w.dsigma.data_ptr(),
                     w.drgb.data_ptr(), st)
        else:
            if not self._dist_forward:
                raise RuntimeError("backward(dL_ddist=...): the forward of this step ran "
                                   "without distortion=True")
            seed = torch.is_tensor(dL_ddist)
            if seed:
                assert dL_ddist.shape == (K, B) and dL_ddist.dtype == torch.float32 \
                    and dL_ddist.is_contiguous()
            self._ev("composite_dist_bw", L.ml_composite_dist_bw, dL_drgb.data_ptr(),
                     dL_dopacity.data_ptr(), None if ddepth_k is None else ddepth_k.data_ptr(),
                     dL_ddist.data_ptr() if seed else None, 0.0 if seed else float(dL_ddist),
                     gate_k.data_ptr(), bg.data_ptr(), w.sigma.data_ptr(), w.rgb.data_ptr(),
                     w.deltas.data_ptr(), w.ts.data_ptr(), w.ws.data_ptr(), w.counts.data_ptr(),
                     w.offsets.data_ptr(), w.opacity_k.data_ptr(), w.depth_k.data_ptr(),
                     w.rgb_k.data_ptr(), w.dist_k.data_ptr(), B, K, float(T_threshold),
                     w.dsigma.data_ptr(), w.drgb.data_ptr(), st)
        if gate_at == "field":          # side stream, beside field_bwd
            gate_bwd(side)
        elif gate_at == "main":         # in line, before field_bwd
            gate_bwd(main)
        self._field_bwd(rays_o, rays_d, st, grid_grad, mlp_grad)
        if self.input_grad:
            self._input_grads(rays_o, rays_d, st)
        if gate_at in ("early", "field"):
            main.wait_stream(side)
            gate_grad.record_stream(side)
            if gate_dx is not None:
                gate_dx.record_stream(side)
        return grid_grad, mlp_grad, gate_grad

    def _gate_dinput(self, B, dev):
        w = self.ws
        if w.gate_dx is None or w.gate_dx.shape[0] != B:
            w.gate_dx = torch.empty(B, 6, device=dev)
        return w.gate_dx

    def _input_grads(self, rays_o, rays_d, st):
        """dL/drays_o, dL/drays_d through the field and the march (the path
        --optimize_ext differentiates, train_ml.py:90-93): rn_field_dinput over
        the compact samples of all K sub-NeRFs, then rn_ml_march_bw sums each
        ray's samples (custom_functions.py:102-112).  The gate's own input
        gradient is in ws.gate_dx ((B, 6): rays_o | second gate input)."""
        m, w, L = self.model, self.ws, lib()
        if w.dxyz is None:
            w.dxyz = torch.empty(w.capacity, 3, device=w.device)
            w.ddir = torch.empty(w.capacity, 3, device=w.device)
            w.drays_o = torch.empty(w.B, 3, device=w.device)
            w.drays_d = torch.empty(w.B, 3, device=w.device)
        self._ev("field_dinput", L.field_dinput, None, None, 0,
                 *self._sample_ptrs(rays_o, rays_d), m.size, *field_ptrs(m),
                 m.packed_dinput_frags().data_ptr(), w.dsigma.data_ptr(), w.drgb.data_ptr(),
                 w.feat.data_ptr() if self.feat_cache else None, w.dxyz.data_ptr(),
                 w.ddir.data_ptr(), self.fwd_blocks, st)
        self._ev("march_bw", L.ml_march_bw, w.counts.data_ptr(), w.offsets.data_ptr(), w.B, m.size,
                 w.ts.data_ptr(), w.dxyz.data_ptr(), w.ddir.data_ptr(), w.drays_o.data_ptr(),
                 w.drays_d.data_ptr(), st)

    def _dgate(self, B, G):
        return self.ws.dgate

    # --------------------------------------------------------------- train step
    def train_step(self, rays_o, rays_d, gate_in2, target_rgb, noise, bg, lambda_opacity=1e-3,
                   lambda_cv_importance=0.0, lambda_depth_mutual=0.0, T_threshold=1e-4,
                   exp_step_factor=0.0, grid_grad=None, mlp_grad=None, gate_grad=None,
                   lambda_distortion=0.0, input_grad=False, gate_topk=None, gate_min=0.0,
                   renormalize=False, target_depth=None, lambda_depth=0.0,
                   lambda_depth_var=0.0, depth_clip=float("inf"), ray_weight=None, guided=None):
        """render -> NeRFLoss -> backward of train_ml.py:179-192 as one launch
        chain: the fused loss kernel writes the backward seeds directly.
        Returns ({term: mean}, (grid_grad, mlp_grad, gate_grad)); gradients are
        accumulated into the given buffers (zero them first).
        lambda_distortion > 0 adds NeRFLoss's distortion term (losses.py:63-67:
        lambda * sum over sub-NeRFs of the per-ray loss's mean) inside the
        composite kernels: the seed is the constant lambda / B per segment.
        input_grad=True also differentiates the rays (rn_field_dinput +
        rn_ml_march_bw and the gate's input gradient, the path --optimize_ext
        needs) and returns a third item (dL/drays_o, dL/drays_d, dL/dgate_in2),
        (B, 3) each: the first sums the march's and the gate's share, the last
        is the gradient of the gate's second input alone (add it to dL/drays_d
        when that input is rays_d).  The last two are views of the workspace:
        use them before the next backward.
        gate_topk / gate_min / renormalize: a routed step (forward()); the
        loss's depth-mutual term then covers the live pairs only, its cv^2
        term still the softmax gate's importance, and last_forward also holds
        gate_used, live and route_count ((K,) int32 on the device: the rays
        routed to each sub-NeRF).
        ray_weight ((B,) fp32): per-ray importance weights of a batch that was
        not drawn uniformly (sampler.GuidedSampler).  One launch between the
        loss and the backward (rn_guided_epilogue) multiplies the seeds on
        rgb, opacity and depth by them, and the distortion seed becomes the
        [K][B] tensor lambda ray_weight / B; dL_dgate from the loss (the cv^2
        term, a batch statistic) stays unweighted, and so do the returned
        terms: they are the means a log compares across runs.  guided: a
        (GuidedSampler, cell_idx) pair; the same launch then records each
        ray's unweighted squared rgb error in the sampler's accumulators.
        ray_weight=None launches nothing extra.
        target_depth ((B,) fp32: the ray parameter each ray should terminate
        at, <= 0 where there is no measurement) with lambda_depth > 0 adds
        terms["depth"] = lambda_depth / B sum_r m_r (sum_k g D - z)^2 (m_r =
        z_r > 0), with lambda_depth_var > 0 terms["depth_var"] = lambda_depth_var
        / B sum_r m_r sum_k g V: V the second moment of each segment's weights
        about z (each (t - z)^2 clipped at depth_clip^2), formed and
        differentiated inside the composite kernels (rn_ml_composite_depth_fw /
        _bw), g the gate the render was combined with.  One launch after the
        loss and the guided epilogue (rn_depth_loss) adds both terms' seeds,
        the gate's included, each multiplied by ray_weight; the terms are
        ordered sums in either mode.  ValueError before any launch for a
        lambda > 0 without targets, targets that are not (B,) fp32, or
        depth_clip <= 0.  Both lambdas 0: nothing is launched or returned
        beyond the step without them."""
        from .losses import fused_depth_loss, fused_nerf_loss
        if guided is not None and ray_weight is None:
            raise ValueError("train_step: guided=(sampler, cell_idx) needs ray_weight")
        depth_on = check_depth_args("train_step", rays_o.shape[0], target_depth, lambda_depth,
                                    lambda_depth_var, depth_clip, device=rays_o.device)
        if depth_on and self._NO_DEPTH:
            raise NotImplementedError(self._NO_DEPTH)
        if depth_on:
            # one contiguous tensor for the composite and the loss: a strided
            # view (a column of an image-shaped map) would be read as if dense
            target_depth = target_depth.detach().contiguous()
            if ray_weight is not None:
                ray_weight = ray_weight.float().contiguous()
        dvar = depth_on and lambda_depth_var > 0
        dist = lambda_distortion > 0
        rgb, opacity, depth, gate, imp = self.forward(
            rays_o, rays_d, gate_in2, noise, bg, T_threshold, exp_step_factor, dist, gate_topk,
            gate_min, renormalize, **(dict(depth_target=target_depth, depth_clip=depth_clip)
                                      if dvar else {}))
        # the step's render, for callers that log it (train_step returns the
        # loss terms and the gradients only)
        self.last_forward = {"rgb": rgb, "opacity": opacity, "depth": depth, "gate": gate,
                             "importance": imp}
        rt = None if self._routed is None else self.ws.route_buffers()
        if rt is not None:
            self.last_forward.update(gate_used=rt["gate_used"], live=rt["live"],
                                     route_count=rt["count"])
        terms, (d_rgb, d_op, d_depth, d_gate) = fused_nerf_loss(
            rgb, target_rgb, opacity, depth, gate if rt is None else rt["gate_used"], imp,
            lambda_opacity, lambda_cv_importance, lambda_depth_mutual, lambda_distortion,
            self.ws.dist_k if dist else None, deterministic=self.deterministic,
            live=None if rt is None else rt["live"])
        d_dist = float(lambda_distortion) / rays_o.shape[0] if dist else None
        if ray_weight is not None:
            from .sampler import guided_epilogue
            gs, cells = (None, None) if guided is None else guided
            guided_epilogue(rgb, target_rgb, cells, ray_weight, d_depth.shape[1],
                            None if gs is None else gs.acc_sum,
                            None if gs is None else gs.acc_cnt, d_rgb, d_op, d_depth)
            if dist:
                d_dist = (ray_weight * d_dist).expand(self.model.size, -1).contiguous()
        extra = {}
        if depth_on:
            # on a routed step the terms' gate is gate_used: its seed goes in
            # before the routing's backward, not with the softmax gate's
            d_gate_used = d_gate if rt is None else torch.zeros_like(d_gate)
            dterms, d_dvar = fused_depth_loss(
                depth, gate if rt is None else rt["gate_used"], self.ws.dvar_k if dvar else None,
                target_depth, ray_weight, lambda_depth, lambda_depth_var, d_depth, d_gate_used)
            terms.update(dterms)
            if dvar:
                extra["dL_ddvar"] = d_dvar
            if rt is not None:
                extra["dL_dgate_used"] = d_gate_used
        if not input_grad:
            grads = self.backward(rays_o, rays_d, gate_in2, gate, bg, d_rgb, d_op, d_depth,
                                  d_gate, T_threshold, grid_grad, mlp_grad, gate_grad, d_dist,
                                  **extra)
            return terms, grads
        saved, self.input_grad = self.input_grad, True
        try:
            grads = self.backward(rays_o, rays_d, gate_in2, gate, bg, d_rgb, d_op, d_depth,
                                  d_gate, T_threshold, grid_grad, mlp_grad, gate_grad, d_dist,
                                  **extra)
        finally:
            self.input_grad = saved
        w = self.ws
        return terms, grads, (w.drays_o + w.gate_dx[:, 0:3], w.drays_d, w.gate_dx[:, 3:6])


class _MLRenderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid_params, mlp_params, gate_params, renderer, rays_o, rays_d, gate_in2,
                noise, bg, T_threshold, esf, distortion=False, route=(None, 0.0, False),
                depth=None):
        # depth: None or (target (B,), clip); the target carries no gradient
        rgb, opacity, depth_out, gate, imp = renderer.forward(
            rays_o, rays_d, gate_in2, noise, bg, T_threshold, esf, distortion, *route,
            **({} if depth is None else dict(depth_target=depth[0], depth_clip=depth[1])))
        # the backward reads this step's samples from the renderer's workspace:
        # stamp it, so a second forward through the same workspace before this
        # backward is caught instead of silently differentiating the wrong step
        renderer.ws.generation += 1
        ctx.generation = renderer.ws.generation
        ctx.renderer = renderer
        ctx.save_for_backward(rays_o, rays_d, gate_in2, gate, bg)
        ctx.T = T_threshold
        ctx.extra = (bool(distortion), depth is not None)
        out = (rgb, opacity, depth_out, gate)
        if distortion:
            # next output: the per-ray distortion loss of every sub-NeRF, (B, K)
            out += (renderer.ws.dist_k.t().contiguous(),)
        if depth is not None:
            # last output: each sub-NeRF's second moment about the target, (B, K)
            out += (renderer.ws.dvar_k.t().contiguous(),)
        return out

    @staticmethod
    def backward(ctx, d_rgb, d_op, d_depth, d_gate, *d_extra):
        rays_o, rays_d, gate_in2, gate, bg = ctx.saved_tensors
        d_extra = list(d_extra)
        d_dist = d_extra.pop(0) if ctx.extra[0] else None
        d_dvar = d_extra.pop(0) if ctx.extra[1] else None
        if ctx.renderer.ws.generation != ctx.generation:
            raise RuntimeError(
                "ml_render_fused: the renderer's workspace was reused by another forward "
                "(same model, gate and batch size) before this backward; run the backward "
                "first, or render the other batch under torch.no_grad()")
        B, K = gate.shape
        dev = rays_o.device
        z = lambda *s: torch.zeros(*s, device=dev)
        d_rgb = z(B, 3) if d_rgb is None else d_rgb.float().contiguous()
        d_op = z(B) if d_op is None else d_op.float().contiguous()
        d_depth = None if d_depth is None else d_depth.float().contiguous()
        d_gate = None if d_gate is None else d_gate.float().contiguous()
        # the kernel's seed layout is [K][B]
        d_dist = None if d_dist is None else d_dist.float().t().contiguous()
        if ctx.extra[1]:
            d_dvar = z(K, B) if d_dvar is None else d_dvar.float().t().contiguous()
        r = ctx.renderer
        need_o, need_d, need_2 = ctx.needs_input_grad[4:7]
        r.input_grad = bool(need_o or need_d or need_2)
        try:
            gg, mg, ag = r.backward(rays_o, rays_d, gate_in2, gate, bg, d_rgb, d_op, d_depth,
                                    d_gate, ctx.T, dL_ddist=d_dist, dL_ddvar=d_dvar)
        finally:
            input_grad, r.input_grad = r.input_grad, False
        do = dd = d2 = None
        if input_grad:
            w = r.ws
            do = w.drays_o + w.gate_dx[:, 0:3] if need_o else None
            dd = w.drays_d.clone() if need_d else None
            d2 = w.gate_dx[:, 3:6].contiguous() if need_2 else None
        return gg, mg, ag, None, do, dd, d2, None, None, None, None, None, None, None


class _GradNotSupported(torch.autograd.Function):
    """Identity on an output the fused chain computes but does not
    differentiate (independent_rgbs, render()'s ws): it stays on the autograd
    graph (anchored to a parameter), and a loss that reaches it raises at
    backward time instead of silently contributing no gradient."""

    @staticmethod
    def forward(ctx, x, anchor, what):
        ctx.what = what
        return x.clone()

    @staticmethod
    def backward(ctx, g, _g_anchor=None):
        raise RuntimeError(
            f"{ctx.what}: the fused training render does not back-propagate through this "
            "output; render with fused=False to differentiate it")


def grad_unsupported(x, anchors, what):
    """x as a graph output whose backward raises (see _GradNotSupported),
    anchored to the first of `anchors` (a tensor or a sequence of them) that
    requires grad; x itself (detached) when autograd is off or none does."""
    if torch.is_tensor(anchors):
        anchors = (anchors,)
    if torch.is_grad_enabled():
        for anchor in anchors:
            if anchor.requires_grad:
                return _GradNotSupported.apply(x, anchor, what)
    return x


_RENDERERS = collections.OrderedDict()
# a workspace holds 1024 sample slots per (ray, sub-NeRF) at ~124 B each (t, dt,
# ray, sigma, rgb, ws, their gradients, staging, the 64-B encoding cache, the
# merged order): ~0.13 GB per 1k rays x sub-NeRFs; the level-partitioned
# forward's planes (80 B per slot) and the binned scatter's page pool are
# shared per device and stream / sized to the records: keep a few workspaces
MAX_RENDERERS = 4


def get_renderer(model, gating_net, n_rays, grad=True, deterministic=False):
    """The cached renderer (and workspace) of (model, gate, batch size).
    Renders without autograd (grad=False) get their own workspace, so a
    logging / validation render between a forward and its backward does not
    overwrite the samples the backward reads.  Least recently used entries
    beyond MAX_RENDERERS are dropped (their workspaces freed).  deterministic:
    FusedMLRenderer(deterministic=True), a renderer of its own."""
    key = (id(model), id(gating_net), n_rays, str(model.mlp_params.device), bool(grad))
    if deterministic:
        key += (True,)
    r = _RENDERERS.get(key)
    if r is None or r.model is not model or r.gate is not gating_net:
        r = FusedMLRenderer(model, gating_net, n_rays, deterministic=bool(deterministic))
        _RENDERERS[key] = r
    _RENDERERS.move_to_end(key)
    while len(_RENDERERS) > MAX_RENDERERS:
        _RENDERERS.popitem(last=False)
    return r


def release_renderers():
    """Drop every cached renderer and its device workspace (and the shared
    forward scratch)."""
    _RENDERERS.clear()
    _LEVEL_SCRATCH.clear()


def ml_render_fused(model, gating_net, rays_o, rays_d, imgs_d, warmup=False, **kwargs):
    """Same result dict as ml_rendering.ml_render (train mode).
    distortion=True adds "distortion": fp32 (B, K), column i the per-ray
    Mip-NeRF 360 distortion loss of sub-NeRF i (DistortionLoss.apply on its
    ws / deltas / ts / rays_a; not gate-weighted, losses.py:63-67), computed
    and differentiated inside the composite kernels.  NeRFLoss(lambda_distortion
    > 0) reads it.  deterministic=True renders through a
    FusedMLRenderer(deterministic=True), a renderer and workspace of its own:
    the backward's gradients are then bitwise reproducible.
    gate_topk= / gate_min= / renormalize=: routed training (FusedMLRenderer.
    forward).  "gating_code" and "gating_importance" stay the softmax gate and
    its column sums, differentiable; "gating_used" (B, K) and "gating_live"
    (B, K) bool are added, values only.  Column i of "depth" is 0 for a dead
    pair and independent_rgbs[i] is the background there.
    depth_target= ((B,) fp32 ray parameters, <= 0: no measurement) /
    depth_clip=: adds "depth_var", fp32 (B, K): column i the second moment of
    sub-NeRF i's weights about the target, sum w min((t - z)^2, clip^2) (not
    gate-weighted), computed and differentiated inside the composite kernels.
    NeRFLoss(lambda_depth_var > 0) reads it."""
    depth_target = kwargs.get("depth_target")
    check_depth_args("ml_render", rays_o.shape[0], depth_target,
                     depth_clip=kwargs.get("depth_clip", float("inf")), device=rays_o.device)
    route = (kwargs.get("gate_topk"), kwargs.get("gate_min", 0.0),
             bool(kwargs.get("renormalize", False)))
    route_params("ml_render", gating_net.out_dim, *route)     # ValueError before any launch
    rays_o, rays_d = rays_o.float().contiguous(), rays_d.float().contiguous()
    second = imgs_d.float().contiguous() if gating_net.type == "image" else rays_d
    B, K, dev = rays_o.shape[0], model.size, rays_o.device
    esf = float(kwargs.get("exp_step_factor", 0.0))
    noise = kwargs.get("noise")
    if noise is None:
        noise = torch.rand(K, B, device=dev)
    if esf == 0:
        bg = torch.ones(3, device=dev)
    elif kwargs.get("random_bg", False):
        bg = torch.rand(3, device=dev)
    else:
        bg = torch.zeros(3, device=dev)
    r = get_renderer(model, gating_net, B, grad=torch.is_grad_enabled(),
                     deterministic=bool(kwargs.get("deterministic", False)))
    distortion = bool(kwargs.get("distortion", False))
    routed = r.route_params(*route) is not None
    fn_args = (model.xyz_encoder.params, model.mlp_params, gating_net.params, r, rays_o, rays_d,
               second, noise.contiguous(), bg, float(kwargs.get("T_threshold", 1e-4)), esf)
    if depth_target is not None:
        outs = _MLRenderFn.apply(*fn_args, distortion, route,
                                 (depth_target.detach().contiguous(),
                                  float(kwargs.get("depth_clip", float("inf")))))
        rgb, opacity, depth, gate = outs[:4]
        dist, dvar = (outs[4] if distortion else None), outs[-1]
    elif distortion:
        rgb, opacity, depth, gate, dist = _MLRenderFn.apply(*fn_args, True, route)
    elif routed:
        rgb, opacity, depth, gate = _MLRenderFn.apply(*fn_args, False, route)
    else:
        rgb, opacity, depth, gate = _MLRenderFn.apply(*fn_args)
    w = r.ws
    # each sub-NeRF's own colour (ml_rendering.py:65,73): values only -- a loss
    # on them raises at backward (the fused backward seeds the combined rgb)
    anchors = (model.mlp_params, model.xyz_encoder.params, gating_net.params)
    singles = [grad_unsupported(w.rgb_k[i] + bg * (1 - w.opacity_k[i])[:, None],
                                anchors, "ml_render independent_rgbs")
               for i in range(K)]
    out = {"rgb": rgb, "independent_rgbs": singles, "depth": depth, "opacity": opacity,
           "gating_code": gate, "gating_importance": gate.sum(0)}
    if distortion:
        out["distortion"] = dist
    if depth_target is not None:
        out["depth_var"] = dvar
    if routed:
        rt = w.route_buffers()
        out["gating_used"] = rt["gate_used"].clone()
        out["gating_live"] = rt["live"].bool()
    return out
