"""GPU: camera-visibility culling of the occupancy grids and the erode decay.

The grid is fixed at 128^3, so the smallest shapes are scale 0.5 (one cascade,
2 M cells per sub-NeRF) and scale 4 (four cascades, 8.4 M), both with K = 2
and the six-camera rig of tests/visibility_ref.py.

  * rn_mark_invisible_cells against the fp32 numpy restatement: count_grid bit
    for bit, the valid mask and n_culled exactly, at both scales and at
    near = 0.06 (cells too near a camera) and 0.01 (the default); the grids and
    bitfields it leaves; idempotence;
  * rn_density_update_visible(erode=0) against rn_density_update_sampled on the
    same marked grid and seed, warm-up and sampled: grids, thresholds and
    bitfields bit-equal, tmp zero at the culled cells and equal elsewhere; on a
    grid without a negative cell everything is bit-equal;
  * erode: new = max(old * clamp(0.95^(1/count), 0.1, 0.95), tmp) against fp64
    to relative 2e-6: device powf and the fp32 reciprocal, amplified by at most
    |ln 0.1| where the clamp is inactive, give about 4 ulp; the bar is 16 ulp;
  * through the Trainer on the analytic sphere of tests/test_gpu_fit.py.
"""
import numpy as np
import pytest
import torch

import visibility_ref as V
from radnerf_amd import dist as rdist
from radnerf_amd._lib import lib
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.trainer import MAX_SAMPLES, Trainer

pytestmark = pytest.mark.gpu

K = 2
THR = 0.01 * MAX_SAMPLES / 3 ** 0.5
G3 = V.G3


def _model(cuda, scale):
    return MNGP(scale, size=K, seed=3).to(cuda)


def _grids(m):
    return [getattr(m, f"density_grid_{i}") for i in range(m.size)]


def _bits(m):
    return [getattr(m, f"density_bitfield_{i}") for i in range(m.size)]


def _fill(m, seed, negatives=True):
    """a mix of negative, zero and positive cells (a third each; the positive
    ones on both sides of the threshold), every bitfield bit set"""
    rng = np.random.default_rng(seed)
    old = []
    with torch.no_grad():
        for g, b in zip(_grids(m), _bits(m)):
            kind = rng.integers(0 if negatives else 1, 3, size=tuple(g.shape))
            v = np.where(kind == 0, -rng.uniform(0.5, 3.0, kind.shape),
                         np.where(kind == 1, 0.0, rng.uniform(0.0, 2 * THR, kind.shape)))
            v = v.astype(np.float32)
            g.copy_(torch.from_numpy(v))
            b.fill_(0xff)
            old.append(v)
    return old


def _rig(cuda, scale):
    return torch.from_numpy(V.rig_poses(scale)).to(cuda)


@pytest.mark.parametrize("near", [0.06, 0.01])
@pytest.mark.parametrize("scale", [0.5, 4.0])
def test_mark_matches_the_restatement(cuda, scale, near):
    ref = V.rig_mark(scale, near, np.float32)
    m = _model(cuda, scale)
    C = m.cascades
    assert ref["valid"].shape == (C, G3)
    old = _fill(m, 5)
    culled = m.mark_invisible_cells(V.INTRINSICS, _rig(cuda, scale), V.IMG_WH, near)
    torch.cuda.synchronize()
    count = m.count_grid.cpu().numpy()
    assert count.dtype == np.float32 and count.shape == (C, G3)
    n_bad = int((count.view(np.uint32) != ref["count"].view(np.uint32)).sum())
    print(f"scale {scale} near {near}: count_grid differs in {n_bad} cells; culled "
          f"{culled.cpu().numpy()} vs {ref['n_culled']}; too near {ref['too_near'].sum(1)}")
    assert n_bad == 0
    assert culled.dtype == torch.int32 and np.array_equal(culled.cpu().numpy(), ref["n_culled"])
    if near == 0.06:
        assert ref["too_near"].sum() > 0                 # the too-near path is exercised
    after = []
    for k in range(K):
        g = _grids(m)[k].cpu().numpy()
        b = _bits(m)[k].cpu().numpy()
        # the valid mask, read off the grid: invalid cells are -1, valid ones max(old, 0)
        assert np.array_equal(g >= 0, ref["valid"])
        want_g, want_b = V.apply_mark(old[k], np.full(C * G3 // 8, 0xff, np.uint8), ref["valid"])
        assert np.array_equal(g, want_g) and np.array_equal(b, want_b)
        after.append((g, b))
    # valid cells' bits are left alone: clear some by hand, mark again -- nothing else changes
    with torch.no_grad():
        for b in _bits(m):
            b[::3] = 0
    again = m.mark_invisible_cells(V.INTRINSICS, _rig(cuda, scale), V.IMG_WH, near)
    torch.cuda.synchronize()
    assert torch.equal(again, culled)
    assert np.array_equal(m.count_grid.cpu().numpy().view(np.uint32), count.view(np.uint32))
    for k in range(K):
        want_b = after[k][1].copy()
        want_b[::3] = 0
        assert np.array_equal(_grids(m)[k].cpu().numpy(), after[k][0])
        assert np.array_equal(_bits(m)[k].cpu().numpy(), want_b)


def _run_update(m, state, warmup, seed, visible, erode=False):
    """restore `state` (grids, bitfields), run one update through the old entry
    (count_grid hidden) or the new one; returns grids, bitfields, thr, tmp"""
    count = m.count_grid
    with torch.no_grad():
        for g, b, (g0, b0) in zip(_grids(m), _bits(m), state):
            g.copy_(g0)
            b.copy_(b0)
    if not visible:
        m.count_grid = None
    try:
        du = m.update_density_grid(THR, warmup=warmup, erode=erode, seed=seed)
    finally:
        m.count_grid = count
    torch.cuda.synchronize()
    return ([g.clone() for g in _grids(m)], [b.clone() for b in _bits(m)], du["thr"].clone(),
            du["tmp"].view(m.size, m.cascades, G3).clone())


@pytest.mark.parametrize("scale", [0.5, 4.0])
def test_update_visible_equals_update_sampled(cuda, scale):
    m = _model(cuda, scale)
    _fill(m, 6)
    m.mark_invisible_cells(V.INTRINSICS, _rig(cuda, scale), V.IMG_WH, 0.06)
    marked = [(g.clone(), b.clone()) for g, b in zip(_grids(m), _bits(m))]
    _fill(m, 7, negatives=False)
    plain = [(g.clone(), b.clone()) for g, b in zip(_grids(m), _bits(m))]
    for warmup in (True, False):
        a = _run_update(m, marked, warmup, 77, visible=False)
        b = _run_update(m, marked, warmup, 77, visible=True)
        neg = torch.stack([g < 0 for g, _ in marked])
        assert 0 < int(neg.sum()) < neg.numel()
        for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
            assert torch.equal(x, y)
        # the old entry evaluates the culled cells too (sigma > 0 there); the new one never
        listed_old = float((a[3][neg] > 0).float().mean())
        print(f"scale {scale} warmup {warmup}: culled share {float(neg.float().mean()):.3f}, "
              f"old entry evaluated {listed_old:.3f} of the culled cells, new entry "
              f"{int((b[3][neg] != 0).sum())} cells")
        assert listed_old > (0.99 if warmup else 0.2)
        assert int((b[3][neg] != 0).sum()) == 0
        assert torch.equal(a[3][~neg], b[3][~neg])
        for k in range(K):                                # culled cells stay as marked
            assert torch.equal(b[0][k][neg[k]], marked[k][0][neg[k]])
        # no negative cell: everything is bit-equal, tmp included
        a = _run_update(m, plain, warmup, 78, visible=False)
        b = _run_update(m, plain, warmup, 78, visible=True)
        for x, y in zip(a[0] + a[1] + list(a[2:]), b[0] + b[1] + list(b[2:])):
            assert torch.equal(x, y)


@pytest.mark.parametrize("scale", [0.5, 4.0])
def test_erode_decay(cuda, scale):
    m = _model(cuda, scale)
    _fill(m, 8)
    m.mark_invisible_cells(V.INTRINSICS, _rig(cuda, scale), V.IMG_WH)
    state = [(g.clone(), b.clone()) for g, b in zip(_grids(m), _bits(m))]
    new, _, _, tmp = _run_update(m, state, False, 91, visible=True, erode=True)
    count = m.count_grid.cpu().numpy()
    decay = V.erode_decay(count)
    assert len(np.unique(decay)) >= 3          # cells seen by 1, 2, ... cameras decay differently
    worst = 0.0
    for k in range(K):
        old = state[k][0].cpu().numpy()
        got = new[k].cpu().numpy().astype(np.float64)
        t = tmp[k].cpu().numpy().astype(np.float64)
        neg = old < 0
        assert neg.any() and np.array_equal(got[neg], old[neg].astype(np.float64))
        want = np.maximum(old.astype(np.float64) * decay, t)[~neg]
        err = np.abs(got[~neg] - want) / np.maximum(np.abs(want), 1e-30)
        err[want == 0] = np.abs(got[~neg])[want == 0]
        worst = max(worst, float(err.max()))
        # the decayed value, not tmp, decides a good share of the cells
        assert float((old[~neg].astype(np.float64) * decay[~neg] > t[~neg]).mean()) > 0.1
    print(f"scale {scale}: erode decay, worst relative error vs fp64 {worst:.2e} (bar 2e-6)")
    assert worst <= 2e-6
    # erode=False on the same state differs (the per-cell decay is in use)
    plain = _run_update(m, state, False, 91, visible=True, erode=False)[0]
    assert not torch.equal(plain[0], new[0])


def _sphere_inputs(cuda):
    import test_gpu_fit as F
    dirs, poses = F._cameras(F.N_TRAIN)
    u8 = (F._images(dirs, poses) * 255).round().to(torch.uint8).contiguous().to(cuda)
    W, H = F.WH
    # the pinhole of F._cameras: x = (i + 0.5 - cx) / fx spans [-half, half] over the W pixels
    half = 0.3
    fx, fy = (W - 1) / (2 * half), (H - 1) / (2 * half * H / W)
    Kmat = np.array([[fx, 0, 0.5 + half * fx], [0, fy, 0.5 + half * H / W * fy], [0, 0, 1]])
    return dirs.to(cuda), poses.to(cuda), u8, F.WH, Kmat


def _sphere_trainer(cuda, inputs, **kw):
    dirs, poses, u8, wh, _ = inputs
    m = MNGP(0.5, size=K, seed=3).to(cuda)
    g = Ray_Gate(K, seed=4).to(cuda)
    return Trainer(m, g, 4096, lr=1e-2, lambda_cv_importance=1e-2, seed=5, directions=dirs,
                   poses=poses, img_wh=wh, images=u8, **kw)


def test_trainer_culls_and_never_revives_a_culled_cell(cuda):
    inputs = _sphere_inputs(cuda)
    # two warm-up updates (steps 0, 16) and one sampled update (step 32)
    tr = _sphere_trainer(cuda, inputs, intrinsics=inputs[4], cull_invisible=True, erode=True,
                         warmup_steps=32)
    m = tr.model
    culled = [g < 0 for g in _grids(m)]
    n = int(tr.n_culled.sum())
    print(f"sphere rig: {n} of {G3} cells culled")
    assert 0 < n < G3 and all(int(c.sum()) == n for c in culled)
    shifts = torch.arange(8, device=cuda, dtype=torch.uint8)
    for step in range(33):
        terms = tr.step_sampled()
        if step % 16 == 0:
            for k in range(K):
                g = _grids(m)[k]
                bits = ((_bits(m)[k][:, None] >> shifts) & 1).bool().reshape(g.shape)
                assert bool((g[culled[k]] < 0).all()) and not bool(bits[culled[k]].any())
                assert torch.equal(g < 0, culled[k])           # and nothing else went negative
                assert bool(bits.any())                        # the rest of the grid is alive
    assert all(np.isfinite(float(v)) for v in terms.values())


def test_default_trainer_updates_through_the_old_entry(cuda):
    inputs = _sphere_inputs(cuda)
    tr = _sphere_trainer(cuda, inputs)
    assert tr.n_culled is None and tr.erode is False
    assert getattr(tr.model, "count_grid", None) is None
    terms = tr.step_sampled()                   # the warm-up update of step 0, then the step
    assert all(np.isfinite(float(v)) for v in terms.values())
    assert getattr(tr.model, "count_grid", None) is None
    # the same update by hand: rn_density_update_sampled on the same initial model, with the
    # seed dist.update_density_grid draws for (seed 5, step 0)
    m = MNGP(0.5, size=K, seed=3).to(cuda)
    seed = int(torch.randint(1 << 62, (1,), generator=rdist.step_generator(cuda, 5, 0),
                             device=cuda))
    n = K * m.cascades * G3
    tmp, occ = torch.empty(n, device=cuda), torch.empty(n, device=cuda, dtype=torch.int32)
    blk = torch.empty(2 * (n // 1024 + 1), device=cuda, dtype=torch.int32)
    part, thr = torch.empty(K * 1024, device=cuda), torch.empty(K, device=cuda)
    ptrs = torch.tensor([g.data_ptr() for g in _grids(m)] + [b.data_ptr() for b in _bits(m)],
                        dtype=torch.int64).to(cuda)
    lo, lh, lr, ls = m.xyz_encoder.level_ptrs()
    lib().density_update_sampled(
        ptrs.data_ptr(), ptrs.data_ptr() + 8 * K, K, m.cascades, 128, 0.5, THR, 0.95, seed,
        m.xyz_encoder.params_f16().data_ptr(), lo, lh, lr, ls, m._h_min.ctypes.data,
        m._h_ext.ctypes.data, m.packed_frags().data_ptr(), tmp.data_ptr(), occ.data_ptr(),
        blk.data_ptr(), part.data_ptr(), thr.data_ptr(), 1,
        torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize()
    for k in range(K):
        assert bool((_grids(tr.model)[k] >= 0).all())
        assert torch.equal(_grids(tr.model)[k], _grids(m)[k])
        assert torch.equal(_bits(tr.model)[k], _bits(m)[k])
