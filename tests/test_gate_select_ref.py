"""CPU: the numpy restatement of the gate-sparse selection
(tests/gate_select_ref.py) has the properties include/radnerf.h promises; the
GPU tests (tests/test_gpu_sparse_render.py) hold rn_gate_select to it bit for
bit."""
import numpy as np
import pytest

import gate_select_ref as GR

KS = [2, 3, 8, 9, 16]
F = np.float32


@pytest.mark.parametrize("K", KS)
def test_every_row_keeps_one(K):
    g = GR.gate_rows(200, K, seed=K)
    for tau in (0.0, 0.5, 0.999):
        for k in (1, 2, K):
            r = GR.select_ref(g, tau, k)
            assert (r["live"].sum(1) >= 1).all() and (r["live"].sum(1) <= k).all()
            # the first maximal gate is the one always kept
            first_max = g.argmax(1)
            assert r["live"][np.arange(len(g)), first_max].all()
    # a row wholly below gate_min keeps exactly its first maximum
    low = np.full((1, K), F(1) / F(K), F)
    r = GR.select_ref(low, 0.75, None)
    assert r["live"].tolist() == [[1] + [0] * (K - 1)]


@pytest.mark.parametrize("K", KS)
def test_ties_go_to_the_lower_index(K):
    eq = np.full((1, K), F(1) / F(K), F)                      # exactly 1/K everywhere
    for k in range(1, K + 1):
        r = GR.select_ref(eq, 0.0, k)
        assert r["live"][0].tolist() == [1] * k + [0] * (K - k)
    # zeros and denormals: equal gates rank by index, a denormal outranks zero
    row = np.zeros((1, K), F)
    row[0, K - 1] = row[0, 0] = 1e-40
    assert 0 < row[0, 0] < np.finfo(F).tiny
    r = GR.select_ref(row, 0.0, 2)
    want = [0] * K
    want[0] = want[K - 1] = 1
    assert r["live"][0].tolist() == want
    assert GR.select_ref(row, 0.0, 1)["live"][0].tolist() == [1] + [0] * (K - 1)
    # gate_min exactly equal to a gate value: that pair is live
    g = GR.softmax_rows(50, K, seed=1)
    tau = float(g[7, 1])
    r = GR.select_ref(g, tau, None)
    assert r["live"][7, 1] == 1
    assert np.array_equal(r["live"].astype(bool), (g >= F(tau)) | (r["rank"] == 0))
    below = float(np.nextafter(F(tau), F(2)))                 # one ulp above: dead unless rank 0
    assert GR.select_ref(g, below, None)["live"][7, 1] == (r["rank"][7, 1] == 0)


@pytest.mark.parametrize("K", KS)
def test_topk_K_and_zero_threshold_is_dense(K):
    g = GR.gate_rows(300, K, seed=3)
    for k in (None, K):
        r = GR.select_ref(g, 0.0, k)
        assert r["live"].all()
        assert np.array_equal(r["gate_used"], g)
        assert all(np.array_equal(l, np.arange(300)) for l in r["list"])
        assert r["count"].tolist() == [300] * K


@pytest.mark.parametrize("K", KS)
def test_renormalised_rows_sum_to_one(K):
    g = GR.gate_rows(500, K, seed=5)
    for tau, k in ((0.0, 1), (0.0, 2), (0.1, None), (0.5, K), (0.999, None)):
        r = GR.select_ref(g, tau, k, renormalize=True)
        u = r["gate_used"]
        assert u.dtype == np.float32 and (u[r["live"] == 0] == 0).all()
        # each quotient is within half an ulp (of at most 1) of g / S: the
        # fp64 sum of a row is within K half-ulps of 1, K ulp with room
        s = u.astype(np.float64).sum(1)
        assert np.abs(s - 1).max() <= K * 2.0 ** -23, (tau, k, np.abs(s - 1).max())
        # and the quotient is the correctly rounded one
        i, j = np.nonzero(r["live"])
        exact = g[i, j].astype(np.float64) / r["S"][i].astype(np.float64)
        assert np.array_equal(u[i, j], exact.astype(np.float32))


@pytest.mark.parametrize("K", KS)
def test_combine_within_the_dead_mass(K):
    """|d rgb_c|, |d opacity| <= sum_dead gate (1 + 2^-20) + K 2^-23 on per-pair
    values in [0, 1]: each dropped term is (rgb + bg (1 - op)) g <= g (1 + ulp)
    for c = rgb + bg (1 - op) in [0, 1] (bg in [0, 1], rgb <= op), the two sums
    round K times each at magnitudes <= 1."""
    n = 400
    rng = np.random.default_rng(K)
    g = GR.gate_rows(n, K, seed=11)
    op = rng.random((K, n)).astype(F)
    rgb = (rng.random((K, n, 3)).astype(F) * op[:, :, None]).astype(F)       # rgb <= opacity
    depth = rng.random((K, n)).astype(F)
    for bg in (np.ones(3, F), np.zeros(3, F)):
        dense = GR.combine_ref(g, op, depth, rgb, bg)
        for tau, k in ((0.0, 1), (0.05, None), (0.3, 2), (0.999, None)):
            r = GR.select_ref(g, tau, k)
            dead = (r["live"] == 0)
            zero = lambda a: np.where(dead.T if a.ndim == 2 else dead.T[:, :, None], F(0), a)
            sparse = GR.combine_ref(r["gate_used"], zero(op), zero(depth), zero(rgb), bg)
            mass = np.where(dead, g, 0).astype(np.float64).sum(1)
            bound = mass * (1 + 2.0 ** -20) + K * 2.0 ** -23
            d_rgb = np.abs(sparse[0].astype(np.float64) - dense[0]).max(1)
            d_op = np.abs(sparse[1].astype(np.float64) - dense[1])
            assert (d_rgb <= bound).all() and (d_op <= bound).all(), (tau, k)
            # zeroed dead outputs or untouched ones: gate_used 0 kills the term either way
            keep = GR.combine_ref(r["gate_used"], op, depth, rgb, bg)
            assert all(np.array_equal(a, b) for a, b in zip(keep, sparse))
