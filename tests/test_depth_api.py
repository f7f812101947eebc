"""CPU: depth supervision's public surface -- the four C entries' declarations
and argument checks, every ValueError / NotImplementedError of
sampler.TrainDepths, FusedMLRenderer, Trainer, ml_render and NeRFLoss (raised
before the library is loaded or anything is allocated: `no_library`, the
pattern of tests/test_sampler_api.py), NeRFLoss's composed terms against a
hand computation, and the state's hyper-parameters.  The GPU side is
tests/test_gpu_depth.py.
"""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import depth_ref as DR
from radnerf_amd import _lib, fused, losses, sampler
from radnerf_amd.fused import FusedMLRenderer, check_depth_args, ml_render_fused
from radnerf_amd.losses import NeRFLoss, composed_depth_var
from radnerf_amd.pinned import PinnedMLRenderer
from radnerf_amd.sampler import TrainDepths
from radnerf_amd.trainer import Trainer

from test_train_state_api import _trainer as _cpu_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "rn_ml_composite_depth_fw": "pppppplifppppppfppp",
    "rn_ml_composite_depth_bw": "pppppppppppppppfpppfpplifppp",
    "rn_gather_depth": "pillfippplpp",
    "rn_depth_loss": "pppppliffpppppp",
}
INF = float("inf")


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (sampler, _lib, fused, losses):
        monkeypatch.setattr(mod, "lib", boom)


def _fake_images(n_images, n_pix):
    ti = sampler.TrainImages.__new__(sampler.TrainImages)
    ti.images = torch.zeros(1, 1, 3, dtype=torch.uint8)
    ti.n_images, ti.n_pix, ti.dtype_code = n_images, n_pix, 0
    ti.device = ti.images.device
    return ti


# ---- the C entries ----------------------------------------------------------------
def test_entries_declared_and_bound():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    table = _lib.parse_signature_table(gs.table(hdr))
    for name, codes in ENTRIES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert _lib.binding_signatures()[name] == table[name] == codes, name
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    assert "depth.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()
    # the header states the operation order the restatement was written from
    for s in ("fminf(e * e, clip2)", "fmaf(w, phi, acc)", "sqrtf((dx dx + dy dy) + dz dz)",
              "gw_dist_s + gv * phi_s", "2 g dist_k + gv * dvar_k"):
        assert s in hdr, s


def test_entries_check_without_gpu():
    L = _lib.lib()
    gd = lambda **kw: L.gather_depth(*dict(dict(
        depths=64, dtype=0, n_images=3, n_pix=20, scale=1.0, kind=0, directions=None, img=64,
        pix=64, n=16, out=64, stream=None), **kw).values())
    with pytest.raises(RuntimeError, match=r"rn_gather_depth failed \(status 1\).*depth_dtype must be"):
        gd(dtype=2)
    with pytest.raises(RuntimeError, match="rn_gather_depth failed.*kind must be 0"):
        gd(kind=2)
    with pytest.raises(RuntimeError, match=r"rn_gather_depth failed.*must be in \[1, 2\^32\)"):
        gd(n_images=0)
    with pytest.raises(RuntimeError, match="rn_gather_depth failed.*null pointer"):
        gd(kind=1)                      # the Euclidean range needs the directions
    with pytest.raises(RuntimeError, match="rn_gather_depth failed.*null pointer"):
        gd(out=None)
    assert gd(n=0, depths=None, img=None, pix=None, out=None) == 0
    fw = lambda clip, n=16: L.ml_composite_depth_fw(None, None, None, None, None, None, n, 2, 1e-4,
                                                    None, None, None, None, None, None, clip,
                                                    None, None, None)
    for clip in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="rn_ml_composite_depth_fw failed.*clip must be positive"):
            fw(clip)
    with pytest.raises(RuntimeError, match="rn_ml_composite_depth_fw failed.*null pointer"):
        fw(INF)
    assert fw(INF, 0) == 0
    bw = lambda clip, n=16, ws=None, dk=None: L.ml_composite_depth_bw(
        *([64] * 14), 64, clip, 64, 64, None, 0.0, ws, dk, n, 2, 1e-4, None, None, None)
    with pytest.raises(RuntimeError, match="rn_ml_composite_depth_bw failed.*clip must be positive"):
        bw(0.0)
    with pytest.raises(RuntimeError, match="rn_ml_composite_depth_bw failed.*ws and dist_k go together"):
        bw(1.0, ws=64)
    assert bw(1.0, 0) == 0
    dl = lambda **kw: L.depth_loss(*dict(dict(
        depth=64, gate=64, dvar=None, target=64, rw=None, B=16, K=2, ld=1.0, lv=0.0, out=64,
        part=64, dd=64, dg=64, dv=None, stream=None), **kw).values())
    with pytest.raises(RuntimeError, match="rn_depth_loss failed.*bad sizes"):
        dl(B=0)
    with pytest.raises(RuntimeError, match="rn_depth_loss failed.*given together"):
        dl(dvar=64)
    with pytest.raises(RuntimeError, match="rn_depth_loss failed.*null pointer"):
        dl(part=None)


# ---- the Python checks ------------------------------------------------------------
def test_check_depth_args(no_library):
    z = torch.zeros(8)
    assert check_depth_args("f", 8, None) is False
    assert check_depth_args("f", 8, z) is False
    assert check_depth_args("f", 8, z, 1.0) is True and check_depth_args("f", 8, z, 0, 0.5) is True
    with pytest.raises(ValueError, match="f: lambda_depth / lambda_depth_var > 0 need depth targets"):
        check_depth_args("f", 8, None, 1.0)
    with pytest.raises(ValueError, match="lambda_depth_var > 0 need depth targets"):
        check_depth_args("f", 8, None, 0.0, 1.0)
    for bad in (torch.zeros(7), torch.zeros(8, 1), torch.zeros(8, dtype=torch.float64), [0.0] * 8):
        with pytest.raises(ValueError, match=r"depth targets must be a \(8,\) fp32 tensor"):
            check_depth_args("f", 8, bad, 1.0)
    for clip in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match=r"depth_clip must be > 0"):
            check_depth_args("f", 8, z, 1.0, depth_clip=clip)
    for name in ("lambda_depth", "lambda_depth_var"):
        with pytest.raises(ValueError, match=name + " must be >= 0"):
            check_depth_args("f", 8, z, **{name: -1.0})
    # the kernels take device pointers: targets on another device than the rays are refused
    with pytest.raises(ValueError, match="f: depth targets must be on the rays' device cuda:0, got cpu"):
        check_depth_args("f", 8, z, 1.0, device="cuda:0")
    with pytest.raises(ValueError, match="depth targets must be on the rays' device"):
        check_depth_args("f", 8, z, device=torch.device("cuda", 0))
    assert check_depth_args("f", 8, z, 1.0, device="cpu") is True
    # any stride passes the check (the callers make one contiguous copy)
    assert check_depth_args("f", 8, torch.zeros(8, 3)[:, 1], 1.0) is True
    assert check_depth_args("f", 8, torch.zeros(16)[::2], 0.0, 1.0, device=z.device) is True
    assert fused.check_depth_weights("f") is False and fused.check_depth_weights("f", 0, 2.0) is True
    with pytest.raises(ValueError, match="f: depth_clip must be > 0"):
        fused.check_depth_weights("f", 1.0, 0.0, 0.0)


def test_train_depths_checks(no_library):
    ok = torch.zeros(2, 20)
    for bad, msg in ((np.zeros((2, 20)), "must be a tensor"), (torch.zeros(2, 20, 1), r"must be \(N, H\*W\)"),
                     (torch.zeros(2, 20, dtype=torch.float64), "must be uint16 or float32"),
                     (torch.zeros(20, 2).t(), "must be contiguous")):
        with pytest.raises(ValueError, match="TrainDepths: depths " + msg):
            TrainDepths(bad)
    with pytest.raises(ValueError, match="kind must be 't' or 'euclidean'"):
        TrainDepths(ok, kind="z")
    for s in (0.0, -1.0, INF, float("nan")):
        with pytest.raises(ValueError, match="scale must be a positive finite number"):
            TrainDepths(ok, scale=s)
    with pytest.raises(ValueError, match=r"depths \(2, 20\) do not match the images' \(2, 21\)"):
        TrainDepths(ok, images=_fake_images(2, 21))
    # last of the checks: the kernel takes device pointers only
    with pytest.raises(ValueError, match="depths must be on the GPU"):
        TrainDepths(ok)
    with pytest.raises(ValueError, match="depths must be on the GPU"):
        TrainDepths(torch.zeros(2, 20, dtype=torch.int16), scale=1e-3, kind="euclidean")
    p = inspect.signature(TrainDepths.__init__).parameters
    assert [(k, p[k].default) for k in list(p)[2:4]] == [("scale", 1.0), ("kind", "t")]
    assert sampler.DEPTH_KINDS == {"t": 0, "euclidean": 1}


def _cpu_depths(n_images, n_pix):
    td = TrainDepths.__new__(TrainDepths)
    td.depths = torch.zeros(n_images, n_pix)
    td.n_images, td.n_pix, td.device = n_images, n_pix, td.depths.device
    td.dtype_code, td.scale, td.kind, td.kind_code = 1, 1.0, "t", 0
    return td


def test_trainer_argument_checks(no_library):
    p = inspect.signature(Trainer.__init__).parameters
    assert [(k, p[k].default) for k in ("depths", "lambda_depth", "lambda_depth_var",
                                        "depth_clip")] == [
        ("depths", None), ("lambda_depth", 0.0), ("lambda_depth_var", 0.0), ("depth_clip", INF)]
    for fn in (Trainer.step, Trainer.step_pixels):
        assert inspect.signature(fn).parameters["target_depth"].default is None
    d, poses = torch.rand(480, 3), torch.rand(2, 3, 4)
    kw = dict(directions=d, poses=poses)
    # raised before the model is looked at
    for clip in (0.0, -2.0):
        with pytest.raises(ValueError, match="Trainer: depth_clip must be > 0"):
            Trainer(None, None, 64, depth_clip=clip, **kw)
    with pytest.raises(ValueError, match="Trainer: lambda_depth must be >= 0"):
        Trainer(None, None, 64, lambda_depth=-1.0, **kw)
    with pytest.raises(ValueError, match="Trainer: lambda_depth_var must be >= 0"):
        Trainer(None, None, 64, lambda_depth_var=-1.0, **kw)
    with pytest.raises(ValueError, match=r"Trainer\(depths=...\) needs images"):
        Trainer(None, None, 64, depths=_cpu_depths(2, 480), **kw)
    with pytest.raises(ValueError, match=r"depths \(2, 481\) do not match the images' \(2, 480\)"):
        Trainer(None, None, 64, depths=_cpu_depths(2, 481), images=_fake_images(2, 480), **kw)
    with pytest.raises(ValueError, match=r"depths \(3, 480\) do not match"):
        Trainer(None, None, 64, depths=_cpu_depths(3, 480), images=_fake_images(2, 480), **kw)
    # the steps: a lambda > 0 without targets, or targets of another shape
    tr = Trainer.__new__(Trainer)
    tr.depth_lambdas = dict(lambda_depth=0.1, lambda_depth_var=0.0, depth_clip=INF)
    tr.images, tr.depths, tr.directions = _fake_images(2, 480), None, d
    with pytest.raises(ValueError, match="Trainer.step: lambda_depth / lambda_depth_var > 0 need"):
        tr.step(torch.zeros(64, 3), None, None, None)
    with pytest.raises(ValueError, match=r"Trainer.step: depth targets must be a \(64,\) fp32"):
        tr.step(torch.zeros(64, 3), None, None, None, target_depth=torch.zeros(63))
    with pytest.raises(ValueError, match="Trainer.step_pixels: lambda_depth"):
        tr.step_pixels(torch.zeros(64, dtype=torch.int64), None, None)
    with pytest.raises(ValueError, match=r"Trainer.step_sampled: .* need Trainer\(depths=...\)"):
        tr.step_sampled()


def test_renderer_checks(no_library):
    p = inspect.signature(FusedMLRenderer.train_step).parameters
    assert [(k, p[k].default) for k in ("target_depth", "lambda_depth", "lambda_depth_var",
                                        "depth_clip")] == [
        ("target_depth", None), ("lambda_depth", 0.0), ("lambda_depth_var", 0.0),
        ("depth_clip", INF)]
    p = inspect.signature(FusedMLRenderer.forward).parameters
    assert p["depth_target"].default is None and p["depth_clip"].default == INF
    p = inspect.signature(FusedMLRenderer.backward).parameters
    assert p["dL_ddvar"].default is None
    r = FusedMLRenderer.__new__(FusedMLRenderer)
    o = torch.zeros(16, 3)
    with pytest.raises(ValueError, match="train_step: lambda_depth / lambda_depth_var > 0 need"):
        r.train_step(o, o, o, o, None, None, lambda_depth_var=1.0)
    with pytest.raises(ValueError, match=r"train_step: depth targets must be a \(16,\) fp32"):
        r.train_step(o, o, o, o, None, None, lambda_depth=1.0, target_depth=torch.zeros(15))
    with pytest.raises(ValueError, match="train_step: depth_clip must be > 0"):
        r.train_step(o, o, o, o, None, None, lambda_depth=1.0, target_depth=torch.zeros(16),
                     depth_clip=0.0)
    # the sub-NeRF-per-GPU layout refuses both lambdas
    pr = PinnedMLRenderer.__new__(PinnedMLRenderer)
    for lam in ("lambda_depth", "lambda_depth_var"):
        with pytest.raises(NotImplementedError, match="depth supervision"):
            pr.train_step(o, o, o, o, None, None, target_depth=torch.zeros(16), **{lam: 0.1})
    with pytest.raises(NotImplementedError, match="depth supervision"):
        pr.forward(o, o, o, torch.zeros(2, 16), None, depth_target=torch.zeros(16))
    with pytest.raises(NotImplementedError, match="depth supervision"):
        pr.backward(o, o, o, None, None, None, None, None, dL_ddvar=torch.zeros(2, 16))
    # ml_render: checked before a renderer is made
    with pytest.raises(ValueError, match=r"ml_render: depth targets must be a \(16,\) fp32"):
        ml_render_fused(None, None, o, o, o, depth_target=torch.zeros(3))
    with pytest.raises(ValueError, match="ml_render: depth_clip must be > 0"):
        ml_render_fused(None, None, o, o, o, depth_target=torch.zeros(16), depth_clip=-1.0)


# ---- NeRFLoss ---------------------------------------------------------------------
def _results(B, K, rng, n_max=9):
    """an op-by-op result's keys for K sub-NeRFs: back-to-back segments of 0..n_max samples"""
    res = {"rgb": torch.rand(B, 3), "opacity": torch.rand(B),
           "depth": torch.rand(B, K, dtype=torch.float64).float() + 0.5}
    gate = torch.rand(B, K) + 0.1
    res["gating_code"] = gate / gate.sum(1, keepdim=True)
    for i in range(K):
        cnt = rng.integers(0, n_max + 1, B)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        n = int(cnt.sum())
        res[f"rays_a_{i}"] = torch.from_numpy(np.stack([np.arange(B), start, cnt], 1)).int()
        res[f"ws_{i}"] = torch.from_numpy(rng.random(n).astype(np.float32) / n_max)
        ts = np.concatenate([np.sort(rng.uniform(0.3, 2.0, c)) for c in cnt] + [[]])
        res[f"ts_{i}"] = torch.from_numpy(ts.astype(np.float32))
    return res


@pytest.mark.parametrize("clip", [INF, 0.4])
def test_nerf_loss_composed_terms(no_library, clip):
    rng = np.random.default_rng(51)
    B, K, ld, lv = 23, 3, 0.3, 0.8
    res = _results(B, K, rng)
    z = rng.uniform(0.3, 2.0, B).astype(np.float32)
    z[::3] = 0.0
    z[1] = -1.0
    tgt = {"rgb": torch.rand(B, 3), "depth": torch.from_numpy(z)}
    V = composed_depth_var(res, tgt["depth"], clip).numpy()
    # by hand, segment by segment in fp64
    want = np.zeros((B, K))
    for i in range(K):
        ws, ts = res[f"ws_{i}"].numpy(), res[f"ts_{i}"].numpy()
        for r, a, c in res[f"rays_a_{i}"].tolist():
            want[r, i] = DR.seg_var(ws[a:a + c], ts[a:a + c], z[r], clip)
    assert not want[z <= 0].any() and want[z > 0].any()
    np.testing.assert_allclose(V, want, rtol=1e-5, atol=1e-9)
    assert not V[z <= 0].any()
    ld_ = NeRFLoss()(res, tgt, lambda_depth=ld, lambda_depth_var=lv, depth_clip=clip)
    g, D = res["gating_code"].double().numpy(), res["depth"].double().numpy()
    m = z > 0
    w_d = ld * (m * ((g * D).sum(1) - z) ** 2).sum() / B
    w_v = lv * (m[:, None] * g * want).sum() / B
    assert float(ld_["depth"]) == pytest.approx(w_d, rel=1e-5)
    assert float(ld_["depth_var"]) == pytest.approx(w_v, rel=1e-5)
    # the terms the fused chain's key gives: the same numbers
    with_key = dict(res, depth_var=torch.from_numpy(want).float())
    ld2 = NeRFLoss()(with_key, tgt, lambda_depth_var=lv)
    assert set(ld2) == {"rgb", "opacity", "depth_var"}
    assert float(ld2["depth_var"]) == pytest.approx(w_v, rel=1e-5)
    # a routed result: the terms take the gate the render was combined with
    used = res["gating_code"] * (torch.rand(B, K) > 0.4)
    ld3 = NeRFLoss()(dict(with_key, gating_used=used), tgt, lambda_depth=ld, lambda_depth_var=lv)
    gu = used.double().numpy()
    assert float(ld3["depth_var"]) == pytest.approx(lv * (m[:, None] * gu * want).sum() / B, rel=1e-5)
    assert float(ld3["depth"]) == pytest.approx(
        ld * (m * ((gu * D).sum(1) - z) ** 2).sum() / B, rel=1e-5)
    # both lambdas 0: the keys of before, the target is not looked at
    assert set(NeRFLoss()(res, {"rgb": tgt["rgb"]})) == {"rgb", "opacity"}
    with pytest.raises(ValueError, match="NeRFLoss: lambda_depth / lambda_depth_var > 0 need"):
        NeRFLoss()(res, {"rgb": tgt["rgb"]}, lambda_depth=ld)
    with pytest.raises(ValueError, match=r"NeRFLoss: depth targets must be a \(23,\) fp32"):
        NeRFLoss()(res, dict(tgt, depth=tgt["depth"][:-1]), lambda_depth_var=lv)
    with pytest.raises(ValueError, match="NeRFLoss: depth_clip must be > 0"):
        NeRFLoss()(res, tgt, lambda_depth_var=lv, depth_clip=0.0)


def test_composed_terms_differentiate(no_library):
    rng = np.random.default_rng(52)
    B, K = 11, 2
    res = _results(B, K, rng)
    for i in range(K):
        res[f"ws_{i}"].requires_grad_(True)
    res["gating_code"].requires_grad_(True)
    z = torch.from_numpy(rng.uniform(0.3, 2.0, B).astype(np.float32))
    z[2] = 0.0
    out = NeRFLoss()(res, {"rgb": torch.rand(B, 3), "depth": z}, lambda_depth_var=1.0)
    out["depth_var"].backward()
    V = composed_depth_var(res, z).detach()
    m = (z > 0).float()
    assert torch.allclose(res["gating_code"].grad, m[:, None] * V / B, rtol=1e-6, atol=1e-12)
    for i in range(K):
        ws, ts = res[f"ws_{i}"], res[f"ts_{i}"]
        ray, inside = losses._ray_of(res[f"rays_a_{i}"].long(), ws.shape[0])
        assert bool(inside.all())
        want = (m * res["gating_code"].detach()[:, i])[ray] * (ts - z[ray]) ** 2 / B
        assert torch.allclose(ws.grad, want, rtol=1e-5, atol=1e-12)


# ---- the state --------------------------------------------------------------------
def test_state_hyper_parameters(no_library):
    plain = _cpu_trainer()
    sd0 = plain.state_dict()
    assert not any(k.startswith(("lambda_depth_var", "depth_clip")) for k in sd0["hyper"])
    assert "lambda_depth" not in sd0["hyper"]           # a trainer without the terms: as before
    on = dict(lambda_depth=0.1, lambda_depth_var=0.5, depth_clip=0.25)
    tr = _cpu_trainer(depth_lambdas=dict(on))
    sd = tr.state_dict()
    assert {k: sd["hyper"][k] for k in on} == on
    assert set(sd["hyper"]) == set(sd0["hyper"]) | set(on)
    # each is checked on load, in both directions
    fresh = _cpu_trainer(seed=7, filled=False)
    with pytest.raises(ValueError, match=r"lambda_depth_var: saved 0.5, this trainer 0.0"):
        fresh.load_state_dict(sd)
    assert fresh.global_step == 0
    fresh.load_state_dict(sd, override=True)
    assert fresh.global_step == 37 and "lambda_depth" not in fresh.state_dict()["hyper"]
    other = _cpu_trainer(seed=7, filled=False, depth_lambdas=dict(on, depth_clip=INF))
    with pytest.raises(ValueError, match=r"depth_clip: saved 0.25, this trainer inf"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match=r"lambda_depth: saved 0.0, this trainer 0.1"):
        other.load_state_dict(sd0)
    same = _cpu_trainer(seed=7, filled=False, depth_lambdas=dict(on))
    same.load_state_dict(sd)
    assert same.global_step == 37
