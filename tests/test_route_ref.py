"""CPU: the routed-training restatement (tests/route_ref.py) tied to what it
restates.

  * with every pair live it reproduces ml_oracle.ml_train_step (the dense
    oracle, which it does not call): the same march, outputs and gradients;
  * select_bw_ref (rn_gate_select_bw in fp32) against fp64 autograd of mask . g
    and mask . g / sum(mask . g), per entry within (K + 3) 2^-23 (|d_i| +
    sum_live |d_j u_j|) / S -- K products, K adds, a subtraction and two
    divisions, each half an ulp of a quantity no larger than the bracket;
    dead entries exactly 0 (where gate_rows' denormal rows put the exact
    gradient beyond fp32's range, the fp32 result must be that infinity);
  * depth_mutual_ref: all-live equals NeRFLoss's depth_mutual term, dead pairs
    contribute 0.
"""
import numpy as np
import pytest
import torch

import route_ref as RR
from gate_select_ref import gate_rows, select_ref
from oracle import ml_oracle
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd.losses import NeRFLoss


def _inputs(B, K, scale, seed_gate=6):
    n_entries = int(LY.grid_levels(scale)["n_entries"])
    cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)
    grid = S.grid_params(n_entries).reshape(-1, 2)
    mlp = S.mlp_params(K, LY.FIELD_PARAMS)
    gate = S.mlp_params(1, LY.gate_params(K), seed=seed_gate)[0]
    bits = S.bitfields(K, cascades, p=0.5)
    o, d = S.rays(B, scale)
    return o, d, bits, S.noise(K, B), grid, mlp, gate, S.loss_seeds(B, K)


def test_all_live_is_the_dense_oracle():
    B, K, scale = 48, 2, 0.5
    o, d, bits, nz, grid, mlp, gate, seeds = _inputs(B, K, scale)
    ref = ml_oracle.ml_train_step(o, d, bits, nz, grid, mlp, gate, scale, seeds=seeds,
                                  input_grads=True)
    got = RR.routed_train_step(o, d, bits, nz, grid, mlp, gate, scale, np.ones((B, K), bool),
                               seeds=seeds, input_grads=True)
    assert np.array_equal(got["counts"], ref["counts"]) and got["total"] == ref["total"] > 0
    for k in range(K):
        a = int(ref["starts"][k, 0])
        n = int(ref["counts"][k].sum())
        assert np.array_equal(got["ts"][k], ref["ts"][a:a + n])
        assert np.array_equal(got["deltas"][k], ref["deltas"][a:a + n])
        assert np.array_equal(got["sigmas"][k], ref["sigmas"][k])
    assert np.array_equal(got["gate"], ref["gate"])
    assert np.array_equal(got["gate_used"], ref["gate"].astype(np.float64))
    assert np.array_equal(got["depth"], ref["depth"])
    # the combine runs in fp64 here and in fp32 there: K + 1 roundings of terms <= 1
    for k in ("rgb", "opacity"):
        assert np.abs(got[k] - ref[k]).max() <= (K + 2) * 2.0 ** -24, k
    for k in ("grid_grad", "mlp_grad", "gate_grad", "drays_o", "drays_d"):
        err = np.linalg.norm(got[k] - ref[k]) / np.linalg.norm(ref[k])
        print(k, err)
        assert err <= 1e-5, (k, err)


def test_dead_pairs_have_no_samples_and_no_gradient():
    B, K, scale = 48, 2, 0.5
    o, d, bits, nz, grid, mlp, gate, seeds = _inputs(B, K, scale)
    live = np.zeros((B, K), bool)
    live[:, 0] = True                       # sub-NeRF 1 is never used
    got = RR.routed_train_step(o, d, bits, nz, grid, mlp, gate, scale, live, seeds=seeds)
    assert got["counts"][1].sum() == 0 and got["counts"][0].sum() > 0
    assert not got["mlp_grad"][1].any() and got["mlp_grad"][0].any()
    assert not got["dgate"][:, 1].any() and got["dgate"][:, 0].any()
    assert not got["depth"][:, 1].any()


@pytest.mark.parametrize("K", [2, 3, 9, 16])
def test_select_bw_ref_vs_fp64_autograd(K):
    n = 600
    g = gate_rows(n, K, seed=K)
    rng = np.random.default_rng(100 + K)
    d = rng.standard_normal((n, K)).astype(np.float32)
    for topk, tau in ((1, 0.0), (min(2, K), 0.0), (K, 0.05), (K, 0.0)):
        sel = select_ref(g, gate_min=tau, gate_topk=topk)
        lv = sel["live"].astype(bool)
        gt = torch.tensor(g.astype(np.float64), requires_grad=True)
        mask, dt = torch.tensor(lv.astype(np.float64)), torch.tensor(d.astype(np.float64))
        # plain: d(mask . g) = mask . d, exactly
        out = RR.select_bw_ref(g, lv, d, False)
        (mask * gt * dt).sum().backward()
        assert np.array_equal(out.astype(np.float64), gt.grad.numpy())
        assert not out[~lv].any()
        # renormalised: rows with a positive live sum
        S = sel["S"].astype(np.float64)
        ok = S > 0
        gt.grad = None
        used = mask * gt
        (used[ok] / used[ok].sum(1, keepdim=True) * dt[ok]).sum().backward()
        out = RR.select_bw_ref(g, lv, d, True)
        assert not out[~lv].any() and not out[~ok].any()
        u = np.where(lv, g.astype(np.float64) / np.where(ok, S, 1.0)[:, None], 0.0)
        bound = (K + 3) * 2.0 ** -23 * (np.abs(d) + np.abs(d * u).sum(1, keepdims=True)) \
            / np.where(ok, S, 1.0)[:, None]
        ref = gt.grad.numpy()
        # the denormal rows (S = 2e-40) put the exact gradient past fp32's
        # largest number: there the fp32 result must be the infinity of that
        # sign, and the rounding bound holds everywhere else
        over = np.abs(ref) > np.finfo(np.float32).max
        rows = ok[:, None] & lv
        assert np.array_equal(out[rows & over], np.sign(ref[rows & over]) * np.float32(np.inf))
        rows &= ~over
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(out.astype(np.float64) - ref)
        assert rows.any() and np.isfinite(bound[rows]).all()
        assert (err[rows] <= bound[rows]).all(), float((err[rows] / bound[rows]).max())


def test_routed_depth_mutual():
    B, K, lam = 257, 4, 0.3
    rng = np.random.default_rng(5)
    depth = rng.random((B, K)).astype(np.float32) * 4
    gate = gate_rows(B, K, seed=2)
    # every pair live: NeRFLoss's term and its autograd seed
    dt = torch.tensor(depth, requires_grad=True)
    ref = NeRFLoss()({"rgb": torch.zeros(B, 3), "opacity": torch.ones(B), "depth": dt,
                      "gating_code": torch.tensor(gate)}, {"rgb": torch.zeros(B, 3)},
                     lambda_depth_mutual=lam)["depth_mutual"]
    ref.mean().backward()
    terms, seed = RR.depth_mutual_ref(depth, gate, np.ones((B, K), bool), lam)
    assert np.allclose(terms, ref.detach().numpy(), rtol=1e-5, atol=1e-7)
    assert np.allclose(seed, dt.grad.numpy(), rtol=1e-5, atol=1e-9)
    # routed: dead pairs add nothing, live pairs are measured against the
    # gate_used-weighted mean
    sel = select_ref(gate, gate_topk=2)
    lv = sel["live"].astype(bool)
    dep = np.where(lv, depth, np.float32(0))            # a dead pair's depth is 0
    terms, seed = RR.depth_mutual_ref(dep, sel["gate_used"], lv, lam)
    assert not terms[~lv].any() and not seed[~lv].any()
    mean = (dep.astype(np.float64) * sel["gate_used"]).sum(1, keepdims=True)
    want = np.where(lv, lam * (dep - mean) ** 2, 0.0)
    assert np.allclose(terms, want, rtol=1e-5, atol=1e-7)
    assert np.allclose(seed, np.where(lv, 2 * lam * (dep - mean) / (B * K), 0.0),
                       rtol=1e-5, atol=1e-9)
