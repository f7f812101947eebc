"""CPU: the mathematics depth supervision's backward rests on, on the numpy
restatement (tests/depth_ref.py) -- no library, no device.

  * V = Var_w(t) + (E_w t - z)^2 for opacity-1 weights and no clip;
  * the mixture's V is linear in the gate;
  * the analytic dL/dsigma (include/radnerf.h, rn_ml_composite_depth_bw)
    against central differences in fp64, on the segment shapes the GPU test
    runs (test_gpu_distortion.SEGMENTS: 0-1024 samples, ends mid-chunk, at lane
    63, at lane 0 of the second chunk, in the first of 16 chunks, never);
  * the combined DIST + DEPTH per-sample seed gw and total wtot against the
    fp64 autograd of the summed loss.
"""
import numpy as np
import pytest
import torch

import depth_ref as DR

# test_gpu_distortion.py's K = 2 x 7 segments: (samples, termination)
SEGMENTS = [
    [(0, "never"), (1, "never"), (63, "never"), (64, 63), (65, "never"), (128, 64), (129, 63)],
    [(200, 100), (1024, 20), (1024, "never"), (129, "natural"), (200, "natural"), (128, 127),
     (1024, "natural")],
]
THR = 1e-4


def _segment(n, end, rng):
    """sigma, delta, t of one segment in fp64 (test_gpu_distortion._segments' recipe) and m,
    the number of contributing samples: the first with T <= THR is the last"""
    dl = rng.uniform(1e-3, 5e-3, n)
    ts = np.cumsum(dl) + rng.uniform(0.3, 1.0)
    tau = {"never": 2.0, "natural": 15.0}.get(end, 0.7)
    m0 = n if isinstance(end, str) else end + 1
    sig = rng.uniform(0, 2 * tau / m0, n) / dl
    sig[rng.random(n) < 0.2] = 0.0
    if not isinstance(end, str):
        sig[end] = 30.0 / dl[end]
    T = np.exp(-np.cumsum(sig * dl))
    hit = np.nonzero(T <= THR)[0]
    m = n if len(hit) == 0 else int(hit[0]) + 1
    return sig, dl, ts, m


def _cases():
    rng = np.random.default_rng(41)
    out = []
    for row in SEGMENTS:
        for n, end in row:
            if n:
                out.append((n, end) + _segment(n, end, rng))
    return out


CASES = _cases()


def _targets(ts, m):
    """before the first sample, between two samples, beyond the last contributing one"""
    j = max(0, m // 2 - 1)
    mid = 0.5 * (ts[j] + ts[min(j + 1, len(ts) - 1)])
    return [0.5 * ts[0], mid, ts[m - 1] + 0.05]


def _part_clip(t, z):
    """a clip that is active on part of the segment: halfway between the
    nearest and the farthest sample's distance from the target"""
    e = np.abs(t - z)
    return 0.5 * (e.min() + e.max()) + 1e-6


def test_termination_cases_came_out():
    want = {(64, 63): 64, (128, 64): 65, (129, 63): 64, (200, 100): 101, (1024, 20): 21,
            (128, 127): 128}
    for n, end, _, _, _, m in CASES:
        if end == "never":
            assert m == n
        elif end == "natural":
            assert 1 < m < n
        else:
            assert m == want[(n, end)]


def test_var_plus_bias_for_opacity_one():
    rng = np.random.default_rng(42)
    for n in (1, 5, 64, 200):
        w = rng.random(n)
        w /= w.sum()                                    # opacity 1
        t = np.sort(rng.uniform(0.2, 3.0, n))
        for z in (0.1, float(t[n // 2]), 4.0):
            mean = (w * t).sum()
            var = (w * (t - mean) ** 2).sum()
            V = DR.seg_var(w, t, z, np.inf)
            assert V == pytest.approx(var + (mean - z) ** 2, rel=1e-12, abs=1e-15)
    # no measurement: exactly zero, whatever the weights; a clip only lowers V
    assert DR.seg_var(w, t, 0.0, np.inf) == 0.0 and DR.seg_var(w, t, -1.0, 0.1) == 0.0
    assert DR.seg_var(w, t, 0.1, 0.5) < DR.seg_var(w, t, 0.1, np.inf)
    assert DR.seg_var(w, t, 0.1, 0.5) == pytest.approx((w * np.minimum((t - 0.1) ** 2, 0.25)).sum())


def test_fp32_order_agrees_with_fp64():
    for n, end, sig, dl, ts, m in CASES:
        w, _ = DR.weights(sig, dl, m)
        for z in _targets(ts, m):
            a, b = DR.seg_var_f32(w, ts[:m], z, np.inf), DR.seg_var(w, ts[:m], z, np.inf)
            assert abs(a - b) <= 2e-6 * b + 1e-12, (n, end, z)


def test_mixture_is_linear_in_the_gate():
    rng = np.random.default_rng(43)
    B, K = 37, 4
    V = rng.random((K, B))
    depth = rng.uniform(0.5, 2.0, (B, K))
    z = rng.uniform(0.5, 2.0, B)
    z[::3] = 0.0
    g1, g2 = rng.random((B, K)), rng.random((B, K))
    f = lambda g: DR.depth_loss(depth, g, V, z, None, 0.0, 0.7)[0]["depth_var"]
    a, b = 0.3, 1.9
    assert f(a * g1 + b * g2) == pytest.approx(a * f(g1) + b * f(g2), rel=1e-12)
    # the seeds: d_dvar = lambda / B m g, d_gate = lambda / B m V, exactly the gradient
    _, d_depth, d_gate, d_dvar = DR.depth_loss(depth, g1, V, z, None, 0.0, 0.7)
    m = (z > 0).astype(float)
    assert not d_depth.any()
    np.testing.assert_allclose(d_dvar, 0.7 / B * m[None] * g1.T, rtol=1e-14)
    np.testing.assert_allclose(d_gate, 0.7 / B * m[:, None] * V.T, rtol=1e-14)
    assert not d_dvar[:, ::3].any() and not d_gate[::3].any()


def test_depth_loss_seeds_are_the_autograd_gradient():
    rng = np.random.default_rng(44)
    B, K = 50, 3
    V, depth = rng.random((K, B)), rng.uniform(0.5, 2.0, (B, K))
    gate = rng.random((B, K))
    gate /= gate.sum(1, keepdims=True)
    z = rng.uniform(0.5, 2.0, B)
    z[1::3] = -1.0
    rw = rng.uniform(0.5, 2.0, B)
    ld, lv = 0.4, 0.9
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tg, td, tv = t(gate), t(depth), t(V)
    m = torch.tensor((z > 0).astype(float))
    rwt, zt = torch.tensor(rw), torch.tensor(z)
    # the weighted objective the seeds belong to; the terms themselves are unweighted
    per_d = m * ((tg * td).sum(1) - zt) ** 2
    per_v = m * (tg * tv.t()).sum(1)
    (ld * (rwt * per_d).sum() / B + lv * (rwt * per_v).sum() / B).backward()
    terms, d_depth, d_gate, d_dvar = DR.depth_loss(depth, gate, V, z, rw, ld, lv)
    assert terms["depth"] == pytest.approx(float((ld * per_d.sum() / B).detach()), rel=1e-12)
    assert terms["depth_var"] == pytest.approx(float((lv * per_v.sum() / B).detach()), rel=1e-12)
    np.testing.assert_allclose(d_depth, td.grad.numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(d_gate, tg.grad.numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(d_dvar, tv.grad.numpy(), rtol=1e-12, atol=1e-18)
    # fp32 arithmetic in the header's order stays within rounding of it
    _, f_depth, f_gate, f_dvar = DR.depth_loss(depth, gate, V, z, rw, ld, lv, dtype=np.float32)
    for a, b in ((f_depth, d_depth), (f_gate, d_gate), (f_dvar, d_dvar)):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


@pytest.mark.parametrize("g_dist", [0.0, 0.6])
@pytest.mark.parametrize("clip", [np.inf, "part"])
def test_dsigma_matches_central_differences(clip, g_dist):
    gv = 0.8
    for n, end, sig, dl, ts, m in CASES:
        for z in _targets(ts, m) + [0.0]:
            # a clip that is active on part of the segment
            c = np.inf if clip is np.inf else _part_clip(ts[:m], z)
            got = DR.seg_dsigma(sig, dl, ts, z, c, gv, m, g_dist)
            assert not got[m:].any()
            if z <= 0 and g_dist == 0:
                assert not got.any()
                continue
            # the contributing samples' densities move; the termination sample stays
            idx = np.unique(np.concatenate([np.arange(min(m, 8)), np.arange(max(0, m - 8), m),
                                            np.linspace(0, m - 1, 12).astype(int)]))
            ref = np.zeros(len(idx))
            for q, i in enumerate(idx):
                h = 1e-4 * max(1.0, sig[i])
                up, dn = sig.copy(), sig.copy()
                up[i] += h
                dn[i] -= h
                ref[q] = (DR.seg_loss(up, dl, ts, z, c, gv, m, g_dist)
                          - DR.seg_loss(dn, dl, ts, z, c, gv, m, g_dist)) / (2 * h)
            # central differences: truncation ~1e-8 relative at this step, and a
            # rounding floor of ~4 eps |L| / h <= 1e-10 (|L| <= 10, h >= 1e-4)
            assert np.abs(got[idx] - ref).max() <= 1e-6 * np.abs(ref).max() + 1e-10, \
                (n, end, z, clip)


def test_combined_seed_terms_match_autograd():
    """gw_s = gw_dist_s + gv phi_s is dL/dw_s of g dist(w) + gv V(w), and wtot =
    2 g dist + gv V is sum_s gw_s w_s (dist is homogeneous of degree 2, V of
    degree 1)."""
    g, gv = 0.6, 0.8
    for n, end, sig, dl, ts, m in CASES:
        w, _ = DR.weights(sig, dl, m)
        t, d = ts[:m], dl[:m]
        for z in (_targets(ts, m)[1], 0.0):
            c = _part_clip(t, z)
            gw, wtot = DR.seg_seed_terms(w, t, d, z, c, gv, g)
            wt = torch.tensor(w, requires_grad=True)
            tt, dt = torch.tensor(t - t[0]), torch.tensor(d)
            wi, wti = torch.cumsum(wt, 0), torch.cumsum(wt * tt, 0)
            dist = (2 * wt * (tt * (wi - wt) - (wti - wt * tt)) + wt * wt * dt / 3).sum()
            phi = torch.tensor(DR.phi(t, z, c))
            loss = g * dist + gv * (wt * phi).sum()
            loss.backward()
            ref = wt.grad.numpy()
            assert np.abs(gw - ref).max() <= 1e-11 * max(np.abs(ref).max(), 1e-30), (n, end, z)
            assert wtot == pytest.approx(float((ref * w).sum()), rel=1e-9, abs=1e-18)
            assert wtot == pytest.approx(2 * g * float(dist.detach()) + gv * DR.seg_var(w, t, z, c),
                                         rel=1e-12, abs=1e-18)


def test_gather_restatement():
    depths = np.array([[0, 1000, 65535, 7]], np.uint16)
    dirs = np.array([[0.5, -0.25, 1.0]] * 4, np.float32)
    idx = np.array([0, 0, 0, 0]), np.array([0, 1, 2, 3])
    t = DR.gather_depth(depths, 1e-3, 0, None, *idx)
    assert t.dtype == np.float32 and t[0] == 0
    assert t[1] == np.float32(1000) * np.float32(1e-3)
    e = DR.gather_depth(depths, 1e-3, 1, dirs, *idx)
    norm = np.sqrt(np.float32(0.25 + 0.0625 + 1.0), dtype=np.float32)
    assert e[2] == np.float32(np.float32(65535) * np.float32(1e-3)) / norm and e[0] == 0
    f = np.array([[np.nan, -2.0, 0.0, 1.5]], np.float32)
    assert DR.gather_depth(f, 2.0, 0, None, *idx).tolist() == [0.0, 0.0, 0.0, 3.0]
    # a pick outside the maps reads nothing
    assert DR.gather_depth(f, 2.0, 0, None, np.array([1, 0]), np.array([3, 4])).tolist() == [0, 0]
