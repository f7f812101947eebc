"""rn_bwd_plan by direct calls, against the host restatement tests/plan_ref.py.

The plan decides which sample every merged forward and backward block
touches: a wrong plan shows as a sample scattered twice, never, or into
another model's rows, not as a rounding error, and the chain tests' relative L2
bars do not see that for one ray.  So every output is compared for equality:

  (a) perm and mstart at K = 1..8 over every family of plan_ref.cases()
      (the two-run merge path, the rank path, the merge tree with odd run
      counts, rays past the LDS slice, ties, empty models and rays);
  (b) the level forward's prep rows at three boxes, one of them off the
      power-of-two path;
  (c) chunk_first, all descriptor words and the queue over five schedules;
  (d) a cap_chunks short of the schedule keeps a prefix of it;
  (e) the renderer's own plan on the scenes of
      test_merged_backward_matches_per_model agrees with the restatement;
  (f) the merged kernels on a step that is all ties.

Every output is exactly sized with a sentinel tail (march_ref.Guarded)."""
import functools

import numpy as np
import pytest
import torch

import plan_ref as R
from march_ref import Guarded
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from radnerf_amd.fused import get_renderer, ml_render_fused

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
CASES = R.cases()
NAMES = [c["name"] for c in CASES]
BOXES = (((-0.5, -0.5, -0.5), (1.0, 1.0, 1.0)),            # scale 0.5
         ((-16.0, -16.0, -16.0), (32.0, 32.0, 32.0)),      # scale 16
         ((-0.5, -1.0, -1.5), (1.0, 2.0, 3.0)))            # not powers of two: the division form
SENTINEL = -7                                              # Guarded's, for integers


def _st(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = R.case(name)
    return R.merged_order(c["counts"], c["offsets"], c["ts"])


@functools.lru_cache(maxsize=None)
def _device_inputs(name, cuda):
    c = R.case(name)
    return {k: torch.tensor(c[k], device=cuda) for k in ("counts", "offsets", "seg_base", "seg_count", "ts")}


def _bounds(c, cfg):
    head_n, head, max_chunk, min_chunk, blocks = cfg
    return R.chunk_bounds(c["total"], head_n, head, max_chunk, min_chunk, blocks)[0]


def _plan(cuda, c, cfg, cap, box=None, prep_null=False):
    """one rn_bwd_plan call into exactly sized guarded buffers -> their checked contents"""
    K, B, total = c["K"], c["B"], c["total"]
    g = _device_inputs(c["name"], cuda)
    out = dict(mstart=Guarded(B + 1, I32, cuda), perm=Guarded(total, I32, cuda),
               first=Guarded(cap + 1, I32, cuda), desc=Guarded((cap, R.DESC), I32, cuda),
               queue=Guarded(3, I32, cuda))
    rays = (None,) * 5
    if box is not None:
        mn, ext = (np.array(v, np.float32) for v in box)
        o, d = (torch.tensor(a, device=cuda) for a in R.box_rays(c, mn, ext))
        out["prep"] = Guarded((total, 4), F32, cuda)
        rays = (o.data_ptr(), d.data_ptr(), mn.ctypes.data, ext.ctypes.data,
                None if prep_null else out["prep"].ptr())
    head_n, head, max_chunk, min_chunk, blocks = cfg
    lib().bwd_plan(g["counts"].data_ptr(), g["offsets"].data_ptr(), g["seg_base"].data_ptr(),
                   g["seg_count"].data_ptr(), g["ts"].data_ptr(), B, K, head_n, head, max_chunk,
                   min_chunk, blocks, cap, out["mstart"].ptr(), out["perm"].ptr(), out["first"].ptr(),
                   out["desc"].ptr(), out["queue"].ptr(), *rays, _st(cuda))
    torch.cuda.synchronize()
    return {k: v.check(f"{c['name']} {k}") for k, v in out.items()}


def _first_bad_ray(c, got, want, ms):
    bad = np.flatnonzero(got != want)
    r = int(np.searchsorted(ms, bad[0], side="right") - 1)
    fams = [n for n, idx in c["fam"].items() if r in idx]
    return f"{len(bad)} positions differ, first {bad[0]} on ray {r} {fams} counts {c['counts'][:, r].tolist()}"


def _scratch_contract(c, rows, max_chunk):
    """what rn_field_bwd_merged's scratch_rows is sized for: a chunk and one ray of every model"""
    per_chunk = rows[:, 12:12 + R.KMAX].astype(np.int64).sum(1)
    assert per_chunk.max(initial=0) <= max_chunk + R.ray_totals(c).max(), (c["name"], int(per_chunk.max()))


# ---- (a) order -------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_order(cuda, name):
    c = R.case(name)
    perm, ms = _expected(name)
    cfg = R.CONFIGS[0]
    cap = len(_bounds(c, cfg)) + 5
    got = _plan(cuda, c, cfg, cap)
    assert np.array_equal(got["mstart"], ms), (got["mstart"], ms)
    assert np.array_equal(got["perm"], perm), _first_bad_ray(c, got["perm"], perm, ms)
    again = _plan(cuda, c, cfg, cap)
    for k in got:
        assert np.array_equal(got[k], again[k]), k


# ---- (b) prep --------------------------------------------------------------
@pytest.mark.parametrize("box", range(len(BOXES)))
@pytest.mark.parametrize("name", NAMES)
def test_prep_rows(cuda, name, box):
    c = R.case(name)
    perm, ms = _expected(name)
    mn, ext = BOXES[box]
    cfg = R.CONFIGS[0]
    cap = len(_bounds(c, cfg)) + 5
    got = _plan(cuda, c, cfg, cap, box=BOXES[box])
    assert np.array_equal(got["perm"], perm)
    o, d = R.box_rays(c, mn, ext)
    want = R.prep_rows(perm, R.ray_of_positions(ms), c["ts"], o, d, mn, ext)
    have = np.ascontiguousarray(got["prep"]).view(np.uint32)
    bad = np.flatnonzero((have != want).any(1))
    assert len(bad) == 0, (f"{len(bad)} rows differ, first {bad[:4]}: "
                           f"{have[bad[:2]].tolist()} vs {want[bad[:2]].tolist()}")
    if c["total"] >= 1000:
        # positions that leave the box are clamped to exactly 0.0 or 1.0 (and some stay inside)
        u = have[:, :3].view(np.float32)
        assert (u == 0).any() and (u == 1).any() and ((u > 0) & (u < 1)).any()
    if box == 0:
        # without prep the plan writes none: the buffer keeps its sentinel
        null = _plan(cuda, c, cfg, cap, box=BOXES[box], prep_null=True)
        assert np.isnan(null["prep"]).all() and np.array_equal(null["perm"], perm)


# ---- (c) chunk rows --------------------------------------------------------
@pytest.mark.parametrize("cfg", R.CONFIGS)
@pytest.mark.parametrize("name", NAMES)
def test_chunk_rows(cuda, name, cfg):
    c = R.case(name)
    _, ms = _expected(name)
    bounds = _bounds(c, cfg)
    n = len(bounds)
    first, rows = R.chunk_rows(ms, c["offsets"], c["seg_base"], c["seg_count"], bounds, n, c["K"])
    got = _plan(cuda, c, cfg, n + 5)
    assert got["queue"].tolist() == [0, n, 0]
    assert np.array_equal(got["first"][:n + 1], first), (got["first"][:n + 1], first)
    bad = np.flatnonzero((got["desc"][:n] != rows).any(1))
    assert len(bad) == 0, (f"{len(bad)} of {n} descriptors differ, first {bad[:4]}: "
                           f"{got['desc'][bad[0]].tolist()} vs {rows[bad[0]].tolist()}")
    # the slots past the schedule are not written
    assert np.all(got["first"][n + 1:] == SENTINEL) and np.all(got["desc"][n:] == SENTINEL)
    _scratch_contract(c, got["desc"][:n], cfg[2])


# ---- (d) a cap short of the schedule ---------------------------------------
@pytest.mark.parametrize("name,cfg", [("k2_merge", R.CONFIGS[0]), ("multi_k5", R.CONFIGS[3]),
                                      ("empties_k4", R.CONFIGS[0])])
@pytest.mark.parametrize("cap", ["n-1", "1"])
def test_short_cap_keeps_a_prefix(cuda, name, cfg, cap):
    """cap_chunks < the schedule's count: the chunks kept are the first
    cap_chunks rows of the full schedule bit for bit, the last one included,
    so no chunk outgrows the scratch rows; queue[1] == cap_chunks is the only
    sign.  (Until this test the last kept chunk ran to the last ray.)  No
    merged kernel runs on the truncated plan here."""
    c = R.case(name)
    _, ms = _expected(name)
    bounds = _bounds(c, cfg)
    n = len(bounds)
    assert n >= 4
    cap = n - 1 if cap == "n-1" else 1
    full_first, full_rows = R.chunk_rows(ms, c["offsets"], c["seg_base"], c["seg_count"], bounds, n, c["K"])
    first, rows = R.chunk_rows(ms, c["offsets"], c["seg_base"], c["seg_count"], bounds, cap, c["K"])
    assert np.array_equal(rows, full_rows[:cap]) and np.array_equal(first, full_first[:cap + 1])
    got = _plan(cuda, c, cfg, cap)
    assert got["queue"].tolist() == [0, cap, 0]
    assert np.array_equal(got["first"], first), (got["first"], first)
    assert np.array_equal(got["desc"], rows), (got["desc"][-1].tolist(), rows[-1].tolist())
    _scratch_contract(c, got["desc"], cfg[2])
    assert np.array_equal(got["perm"], _expected(name)[0])          # the order does not depend on the cap


# ---- (e) the renderer's plan on the scenes the suite already trusts --------
def _forward(cuda, sc, esf, noise=None):
    to = lambda a: torch.from_numpy(a).to(cuda)
    return ml_render_fused(sc.m, sc.g, to(sc.o), to(sc.d), to(sc.d),
                           noise=to(sc.noise if noise is None else noise), exp_step_factor=esf)


def _workspace_plan(w, B):
    torch.cuda.synchronize()
    counts, offsets, ts = (t.cpu().numpy() for t in (w.counts, w.offsets, w.ts))
    assert counts.min() >= 0 and counts.max() <= 1024, "the workspace holds no march"
    perm, ms = R.merged_order(counts, offsets, ts)
    assert np.array_equal(w.mstart[:B + 1].cpu().numpy(), ms)
    assert np.array_equal(w.perm[:len(perm)].cpu().numpy(), perm)
    return counts, offsets, ts


@pytest.mark.parametrize("B,K,scale", [(8192, 2, 0.5), (2048, 4, 16.0), (1024, 1, 0.5), (512, 8, 0.5)])
def test_scene_plan_agrees_with_restatement(cuda, B, K, scale):
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    r = get_renderer(sc.m, sc.g, B)
    _forward(cuda, sc, 1 / 256 if scale > 0.5 else 0.0)    # (grad mode on: this renderer's workspace)
    counts, _, _ = _workspace_plan(r.ws, B)
    assert counts.sum() > 10 * B


# ---- (f) the merged kernels on ties ----------------------------------------
def test_consumers_on_ties(cuda):
    """One fused step at K = 3 in which every sub-NeRF has the same occupancy
    and the same jitter: every ray's three runs of t are equal, so the merged
    order is decided by the tie rule alone.  Merged vs per-model backward
    within the bars of test_merged_backward_matches_per_model."""
    K, B, scale = 3, 256, 0.5
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    S.set_bitfields(sc.m, np.repeat(sc.bits[:1], K, 0))
    noise = np.ascontiguousarray(np.repeat(sc.noise[:1], K, 0))
    r = get_renderer(sc.m, sc.g, B)
    to = lambda a: torch.from_numpy(a).to(cuda)
    grads = []
    for merged in (True, False):
        r.merged_bwd = merged
        sc.m.zero_grad(); sc.g.zero_grad()
        res = _forward(cuda, sc, 0.0, noise)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], [to(s) for s in sc.seeds])
        grads.append([p.grad.clone() for p in (sc.m.xyz_encoder.params, sc.m.mlp_params, sc.g.params)])
        if merged:
            counts, offsets, ts = _workspace_plan(r.ws, B)
    r.merged_bwd = True
    tied = [bool(counts[0, q]) and len(set(counts[:, q])) == 1 and
            all(np.array_equal(ts[offsets[k, q]:offsets[k, q] + counts[k, q]],
                               ts[offsets[0, q]:offsets[0, q] + counts[0, q]]) for k in range(K))
            for q in range(B)]
    assert np.mean(tied) > 0.5, np.mean(tied)
    (gm, wm, tm), (gs, ws, ts_) = grads
    lv = LY.grid_levels(scale)
    gm, gs = gm.view(-1, 2), gs.view(-1, 2)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    levels = [rel(gm[int(a):int(a) + int(n)], gs[int(a):int(a) + int(n)])
              for a, n in zip(lv["offset"], lv["hsize"])]
    print(f"ties: all-ties rays {np.mean(tied):.3f}, grid per level max {max(levels):.2e}, "
          f"mlp {rel(wm, ws):.2e}, gate {rel(tm, ts_):.2e}")
    assert gs.norm() > 0 and max(levels) <= 3e-4, levels
    assert rel(wm, ws) <= 1e-5 and rel(tm, ts_) <= 1e-5
