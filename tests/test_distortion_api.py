"""CPU: the surface of the in-chain distortion loss (tests/test_gpu_distortion.py
holds the GPU side).

  * NeRFLoss reads a render's own "distortion" key: lambda * sum_i mean of
    column i, differentiable;
  * the identity the fused backward relies on: the loss is homogeneous of
    degree 2 in ws, so sum_s w_s dL/dw_s = 2 loss per ray -- the total that
    VolumeRenderer.backward takes from its scan of dL_dws * ws
    (volumerendering.cu:109-115) is 2 g loss without a pass over dL_dws;
  * the new C-ABI entries are declared in the header and bound in _lib.
"""
import os
import re

import numpy as np
import torch

import oracle
from radnerf_amd import _lib
from radnerf_amd.losses import NeRFLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _results(B, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    gate = torch.softmax(torch.randn(B, K, generator=g), 1)
    return {"rgb": torch.rand(B, 3, generator=g), "opacity": torch.rand(B, generator=g),
            "depth": torch.rand(B, K, generator=g), "gating_code": gate,
            "gating_importance": gate.sum(0)}, {"rgb": torch.rand(B, 3, generator=g)}


def test_nerf_loss_reads_distortion_key():
    B, K, lam = 50, 3, 0.02
    res, target = _results(B, K)
    dist = torch.rand(B, K, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    dist.requires_grad_(True)
    res["distortion"] = dist
    ld = NeRFLoss()(res, target, lambda_distortion=lam)
    want = lam * sum(float(dist.detach()[:, i].mean()) for i in range(K))
    assert abs(float(ld["distortion"].detach()) - want) <= 1e-12
    sum(v.mean() for v in ld.values()).backward()
    assert torch.allclose(dist.grad, torch.full_like(dist, lam / B), rtol=1e-12, atol=0)
    # render()'s (B,) form: one sub-NeRF
    one = dist.detach()[:, 0].clone().requires_grad_(True)
    res1, _ = _results(B, 1)
    res1["distortion"] = one
    ld = NeRFLoss()(res1, target, lambda_distortion=lam)
    assert abs(float(ld["distortion"].detach()) - lam * float(one.detach().mean())) <= 1e-12
    # without the weight the key is ignored; with lambda = 0 nothing is added
    assert "distortion" not in NeRFLoss()(res, target)


def _rays(n_rays=40, seed=5):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 300, n_rays)
    counts[:4] = [0, 1, 64, 65]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    N = int(counts.sum())
    ws = rng.uniform(0, 0.02, N).astype(np.float32)
    ws[rng.random(N) < 0.3] = 0.0            # as past a termination sample
    deltas = rng.uniform(1e-3, 5e-3, N).astype(np.float32)
    ts = np.concatenate([np.cumsum(rng.uniform(1e-3, 5e-3, c)) + rng.uniform(0.5, 1.0)
                         for c in counts]).astype(np.float32)
    return np.stack([np.arange(n_rays), starts, counts], 1).astype(np.int64), ws, deltas, ts


def test_weighted_gradient_sum_is_twice_the_loss():
    ra, ws, deltas, ts = _rays()
    g = np.random.default_rng(6).normal(size=len(ra)).astype(np.float32)
    loss, wi, wti = oracle.distortion_loss_fw(ws, deltas, ts, ra)
    dws = oracle.distortion_loss_bw(g, wi, wti, ws, deltas, ts, ra)
    for ray, a, n in ra:
        if n == 0:
            assert loss[ray] == 0
            continue
        w, t, d = (x[a:a + n].astype(np.float64) for x in (ws, ts, deltas))
        # the definition (losses.cu:47-142) in float64: the identity is exact
        W_in, WT_in = np.cumsum(w), np.cumsum(w * t)
        W_ex, WT_ex = W_in - w, WT_in - w * t
        L = float(np.sum(2 * (WT_in * W_ex - W_in * WT_ex) + w * w * d / 3))
        dL = 2 * (t * W_ex - WT_ex + (WT_in[-1] - WT_in) - t * (W_in[-1] - W_in)) + 2 / 3 * w * d
        assert abs(float(np.sum(w * dL)) - 2 * L) <= 1e-12 * max(abs(L), 1e-30)
        # the fp32 oracle: its scans cancel (tests/test_gpu_aux.py: 5e-5 off
        # the float64 definition at 400 samples per ray, dL/dws held to 1e-3)
        assert abs(float(loss[ray]) - L) <= 2e-4 * abs(L) + 1e-7
        s = float(np.sum(w * dws[a:a + n].astype(np.float64)))
        assert abs(s - 2 * float(g[ray]) * L) <= 1e-3 * abs(2 * float(g[ray]) * L) + 1e-7


def test_entries_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    for name in ("rn_ml_composite_dist_fw", "rn_ml_composite_dist_bw"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
    # new entries only: the plain ones keep their signatures and the ABI its version
    sig = _lib.binding_signatures()
    assert sig["rn_ml_composite_fw"] == "pppppplifpppppp"
    assert sig["rn_ml_composite_bw"] == "pppppppppppppplifppp"
    assert sig["rn_ml_composite_dist_fw"] == sig["rn_ml_composite_fw"][:-1] + "pp"
    assert _lib.ABI_VERSION == 9
