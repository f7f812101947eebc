"""GPU: depth supervision on the fused chain -- rn_gather_depth,
rn_ml_composite_depth_fw / _bw (csrc/composite.hip, the DEPTH instantiations),
rn_depth_loss, and the Python layers over them.

  1. the gather against its fp32 restatement (depth_ref.gather_depth), bit for bit;
  2. the composite kernels through lib() on test_gpu_distortion.py's segments:
     the plain outputs are the plain kernel's bits (dist_k the distortion
     kernel's), dvar_k and dsigma against fp64 on the kernel's own ws
     (composite_ref.backward with dL_dws = gv phi [+ the distortion gradient]);
  3. the loss entry against fp64 autograd;
  4. train_step against op-by-op autograd through ml_render(fused=False) +
     NeRFLoss, dense and routed (gate_topk=1): both lambdas, the expected-depth
     term alone, both with the distortion loss; a strided view of the targets;
  5. a depth step between two default steps leaves the default step as it was;
  6. Trainer(deterministic=True, depths=...) is reproducible and resumable;
  7. the sub-NeRF-per-GPU renderer refuses the lambdas.

Bars (the project's own): per-segment loss rtol 2e-4 / atol 1e-7
(test_gpu_distortion.py), dsigma <= 1e-4 max(1, |ref|max), drgb <= 1e-4
(test_gpu_parity.py), parameter gradients 1e-3 relative norm (test_gpu_ml.py),
loss terms 1e-5 max(1, |ref|) and seeds rtol 1e-4 / atol 1e-9 (test_gpu_train.py).
"""
import numpy as np
import pytest
import torch

import composite_ref as CR
import depth_ref as DR
import resume_ref as RES
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from radnerf_amd.fused import FusedMLRenderer, ml_render_fused
from radnerf_amd.losses import NeRFLoss, composed_depth_var, fused_depth_loss
from radnerf_amd.pinned import PinnedMLRenderer
from radnerf_amd.rendering import ml_render
from radnerf_amd.sampler import TrainDepths, gather_depth
from test_gpu_distortion import B1, K1, SEGMENTS, THR, _inside, _segments

pytestmark = pytest.mark.gpu
INF = float("inf")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


_rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- 1. the gather ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["t", "euclidean"])
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_gather_vs_restatement(cuda, dtype, kind):
    rng = np.random.default_rng(61)
    N, W, H, n = 3, 5, 4, 300                # 300 picks: two blocks
    P = W * H
    if dtype == "u16":
        maps = rng.integers(1, 65536, (N, P)).astype(np.uint16)
        maps[0, 3] = maps[2, 19] = maps[1, 0] = 0
        maps[1, 7] = 65535
        dev_maps = _t(maps.view(np.int16), cuda)        # int16 storage of the same words
        scale = 1e-3
    else:
        maps = rng.uniform(0.1, 9.0, (N, P)).astype(np.float32)
        maps[0, 3] = 0.0
        maps[2, 19] = np.nan
        maps[1, 0] = -1.5
        maps[1, 7] = -0.0
        maps[2, 2] = np.inf
        dev_maps = _t(maps, cuda)
        scale = 0.37
    dirs = np.stack([rng.uniform(-0.6, 0.6, P), rng.uniform(-0.6, 0.6, P), np.ones(P)], 1)
    dirs = dirs.astype(np.float32)
    img = rng.integers(0, N, n)
    pix = rng.integers(0, P, n)
    # every planted value is picked
    img[:6], pix[:6] = [0, 2, 1, 1, 2, 0], [3, 19, 0, 7, 2, 4]
    td = TrainDepths(dev_maps, scale=scale, kind=kind)
    assert (td.n_images, td.n_pix, td.dtype_code) == (N, P, 0 if dtype == "u16" else 1)
    out = torch.full((n,), -7.0, device=cuda)
    got = gather_depth(td, _t(dirs, cuda), _t(img, cuda), _t(pix, cuda), out=out)
    assert got is out
    want = DR.gather_depth(maps, scale, DR_KIND[kind], dirs, img, pix)
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    assert not g[:3].any() and (g >= 0).all() and not np.isnan(g).any()
    assert (g > 0).sum() > n // 2
    if dtype == "f32":
        assert g[3] == 0 and g[4] == np.inf     # -0.0 is no measurement; inf passes through
    if kind == "euclidean":                     # shorter than the z-depth off the axis
        z = gather_depth(TrainDepths(dev_maps, scale=scale), None, _t(img, cuda), _t(pix, cuda))
        zz = z.cpu().numpy()
        ok = np.isfinite(zz) & (zz > 0)
        assert (g[ok] <= zz[ok]).all() and (g[ok] < zz[ok]).any()


DR_KIND = {"t": 0, "euclidean": 1}


# ---- 2. the composite kernels ---------------------------------------------------------
TARGET_KINDS = ["before", "between", "beyond", "invalid", "between", "before", "beyond"]


def _ray_targets(c):
    """one target per ray, placed against the ray's second segment (never empty):
    before its first sample, between two samples, beyond its last, none"""
    z = np.zeros(B1, np.float32)
    for r, kind in enumerate(TARGET_KINDS):
        n = SEGMENTS[1][r][0]
        a = int(c["offsets"][1, r])
        ts = c["ts"][a:a + n]
        z[r] = {"before": 0.5 * ts[0], "between": 0.5 * (ts[n // 3] + ts[n // 3 + 1]),
                "beyond": ts[-1] + 0.25, "invalid": 0.0}[kind]
    return z


@pytest.fixture(scope="module")
def segs():
    sig, rgbs, deltas, ts, counts, offsets = _segments()
    rng = np.random.default_rng(62)
    gate = rng.random((B1, K1)).astype(np.float32)
    gate /= gate.sum(1, keepdims=True)
    c = dict(sig=sig, rgbs=rgbs, deltas=deltas, ts=ts, counts=counts, offsets=offsets, gate=gate,
             bg=rng.random(3).astype(np.float32),
             gRGB=rng.normal(0, 1, (B1, 3)).astype(np.float32),
             gO=rng.normal(0, 1, B1).astype(np.float32),
             gDepth=rng.normal(0, 1, (B1, K1)).astype(np.float32),
             gdist=rng.normal(0, 1, (K1, B1)).astype(np.float32),
             # the seed on dvar_k: phi is up to ~clip^2 = 0.09 and delta ~3e-3, so
             # seeds of ~20 give dsigma shares of ~1e-2, as the other seeds'
             gdvar=(20 * rng.normal(0, 1, (K1, B1))).astype(np.float32))
    c["z"] = _ray_targets(c)
    return c


@pytest.mark.parametrize("clip", [INF, 0.3])
@pytest.mark.parametrize("dist", [False, True])
def test_composite_kernels_vs_fp64(cuda, segs, dist, clip):
    """Measured on an MI355X: see DESIGN.md §4 "Depth supervision" (the test
    prints the figures)."""
    c, L = segs, lib()
    t = lambda a: _t(a, cuda)
    st = _st(cuda)
    sig, rgbs, dl, ts = t(c["sig"]), t(c["rgbs"]), t(c["deltas"]), t(c["ts"])
    cnt, off, z = t(c["counts"]), t(c["offsets"]), t(c["z"])
    gate, bg, gRGB, gO, gD = (t(c[k]) for k in ("gate", "bg", "gRGB", "gO", "gDepth"))
    gdist, gdvar = t(c["gdist"]), t(c["gdvar"])
    cap = len(c["sig"])
    inside = torch.from_numpy(_inside(c)).to(cuda)

    def forward(which):
        o = dict(used=torch.full((K1, B1), -7, device=cuda, dtype=torch.int32),
                 op=torch.full((K1, B1), -7.0, device=cuda), de=torch.full((K1, B1), -7.0, device=cuda),
                 rgb=torch.full((K1, B1, 3), -7.0, device=cuda), ws=torch.full((cap,), -7.0, device=cuda),
                 dist=torch.full((K1, B1), -7.0, device=cuda),
                 dvar=torch.full((K1, B1), -7.0, device=cuda))
        args = (sig.data_ptr(), rgbs.data_ptr(), dl.data_ptr(), ts.data_ptr(), cnt.data_ptr(),
                off.data_ptr(), B1, K1, THR, o["used"].data_ptr(), o["op"].data_ptr(),
                o["de"].data_ptr(), o["rgb"].data_ptr(), o["ws"].data_ptr())
        if which == "plain":
            L.ml_composite_fw(*args, st)
        elif which == "dist":
            L.ml_composite_dist_fw(*args, o["dist"].data_ptr(), st)
        else:
            L.ml_composite_depth_fw(*args, z.data_ptr(), clip,
                                    o["dist"].data_ptr() if dist else None, o["dvar"].data_ptr(), st)
        return o

    plain, dk, var = forward("plain"), forward("dist"), forward("depth")
    for k in ("used", "op", "de", "rgb", "ws"):
        assert torch.equal(plain[k], var[k]), k
    assert torch.equal(var["ws"][~inside], torch.full_like(var["ws"][~inside], -7.0))
    if dist:
        assert torch.equal(var["dist"], dk["dist"])
    else:
        assert torch.equal(var["dist"], torch.full_like(var["dist"], -7.0))     # not written
    # exactly zero without a measurement and on an empty segment
    dvar = var["dvar"].cpu().numpy()
    invalid = c["z"] <= 0
    assert invalid.sum() == 1 and not dvar[:, invalid].any()
    assert not dvar[c["counts"] == 0].any() and (c["counts"] == 0).sum() == 1
    assert (dvar >= 0).all() and (dvar[(c["counts"] >= 63) & ~invalid[None]] > 0).all()

    # fp64 on the kernel's own ws
    ws = var["ws"].cpu().numpy()
    used = var["used"].cpu().numpy().reshape(-1)
    starts, counts = c["offsets"].reshape(-1), c["counts"].reshape(-1)
    z_seg = np.tile(c["z"], K1)
    gv = c["gdvar"].reshape(-1)
    ref_var = np.zeros(K1 * B1)
    gw = np.zeros(cap)
    n_clipped = n_live = 0
    for j, (a, n) in enumerate(zip(starts, counts)):
        m = min(int(used[j]) + 1, int(n))
        if m <= 0:
            continue
        p = DR.phi(c["ts"][a:a + m].astype(np.float64), float(z_seg[j]), clip)
        ref_var[j] = (ws[a:a + m].astype(np.float64) * p).sum()
        gw[a:a + m] = float(gv[j]) * p
        if z_seg[j] > 0:
            n_live += m
            n_clipped += int((p >= clip * clip).sum()) if np.isfinite(clip) else 0
    if np.isfinite(clip):
        assert 0 < n_clipped < n_live       # the clip is active on part of the samples
    if dist:
        gw = gw + CR.distortion_bw(c["gdist"].reshape(-1), ws, c["deltas"], c["ts"], starts, counts)[0]
    seeds = CR.fold_seeds(c["gate"], c["bg"], c["gRGB"], c["gO"], c["gDepth"])
    ref = CR.backward(CR.alphas(c["sig"], c["deltas"]), c["rgbs"], c["deltas"], c["ts"], starts,
                      counts, used, var["op"].cpu().numpy().reshape(-1),
                      var["de"].cpu().numpy().reshape(-1), var["rgb"].cpu().numpy().reshape(-1, 3),
                      seeds["gO"], seeds["gD"], seeds["gRGB"], gw=gw, ws=ws)

    def backward(which):
        dsig = torch.full((cap,), -7.0, device=cuda)
        drgb = torch.full((cap, 3), -7.0, device=cuda)
        head = (gRGB.data_ptr(), gO.data_ptr(), gD.data_ptr())
        common = (gate.data_ptr(), bg.data_ptr(), sig.data_ptr(), rgbs.data_ptr(), dl.data_ptr(),
                  ts.data_ptr())
        tail = (cnt.data_ptr(), off.data_ptr(), var["op"].data_ptr(), var["de"].data_ptr(),
                var["rgb"].data_ptr())
        out = (B1, K1, THR, dsig.data_ptr(), drgb.data_ptr(), st)
        if which == "plain":
            L.ml_composite_bw(*head, *common, *tail, *out)
        elif which == "dist":
            L.ml_composite_dist_bw(*head, gdist.data_ptr(), 0.0, *common, var["ws"].data_ptr(),
                                   *tail, dk["dist"].data_ptr(), *out)
        else:
            seed = gdvar if which == "depth" else torch.zeros_like(gdvar)
            L.ml_composite_depth_bw(*head, *common, *tail, z.data_ptr(), clip, seed.data_ptr(),
                                    var["dvar"].data_ptr(), gdist.data_ptr() if dist else None, 0.0,
                                    var["ws"].data_ptr() if dist else None,
                                    var["dist"].data_ptr() if dist else None, *out)
        return dsig, drgb

    base = backward("dist" if dist else "plain")     # the same step without the depth seed
    got = backward("depth")
    zero = backward("depth0")
    assert torch.equal(got[1], base[1]) and torch.equal(zero[1], base[1])       # drgb untouched
    # a zero seed: the step without the term (up to the sign of a zero)
    assert torch.equal(zero[0][inside] + 0.0, base[0][inside] + 0.0)
    assert torch.equal(got[0][~inside], torch.full_like(got[0][~inside], -7.0))
    m = inside.cpu().numpy()
    scale = max(1.0, float(np.abs(ref["dsig"]).max()))
    e_sig = float(np.abs(got[0].cpu().numpy()[m] - ref["dsig"][m]).max())
    e_rgb = float(np.abs(got[1].cpu().numpy()[m] - ref["drgb"][m]).max())
    nz = ref_var > 0
    e_var = float(np.max(np.abs(dvar.reshape(-1)[nz] - ref_var[nz]) / ref_var[nz]))
    moved = float((got[0][inside] - base[0][inside]).abs().max())
    print(f"dist {dist} clip {clip}: dvar_k max rel {e_var:.2e} (max {ref_var.max():.3e}); dsigma "
          f"L_inf {e_sig:.2e} at |ref|max {np.abs(ref['dsig']).max():.3e}; drgb L_inf {e_rgb:.2e}; "
          f"the depth seed moves dsigma by {moved:.2e}")
    np.testing.assert_allclose(dvar.reshape(-1), ref_var, rtol=2e-4, atol=1e-7)
    assert e_sig <= 1e-4 * scale
    assert e_rgb <= 1e-4
    # the term stands well above the bar it is checked at, inside a supervised
    # segment: a backward that ignored the seed could not pass
    assert moved > 10 * 1e-4 * scale
    # ... and nothing moves in the segments of the ray without a measurement
    for k in range(K1):
        r = int(np.nonzero(invalid)[0][0])
        a, n = int(c["offsets"][k, r]), int(c["counts"][k, r])
        assert torch.equal(got[0][a:a + n] + 0.0, base[0][a:a + n] + 0.0)


# ---- 3. the loss entry ------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_depth_loss_vs_fp64_autograd(cuda, K, weighted):
    B, ld, lv = 300, 0.7, 1.3                # two blocks, a ragged last wave
    rng = np.random.default_rng(63 + K)
    depth = rng.uniform(0.5, 3.0, (B, K)).astype(np.float32)
    gate = rng.random((B, K)).astype(np.float32)
    gate /= gate.sum(1, keepdims=True)
    V = rng.uniform(0.0, 0.5, (K, B)).astype(np.float32)
    z = rng.uniform(0.5, 3.0, B).astype(np.float32)
    z[::3] = 0.0                            # a third of the targets invalid
    z[3] = -2.0
    rw = rng.uniform(0.25, 4.0, B).astype(np.float32) if weighted else None
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tg, td, tv = f64(gate), f64(depth), f64(V)
    m = torch.tensor((z > 0).astype(np.float64))
    zt = torch.tensor(z.astype(np.float64))
    rwt = torch.ones(B, dtype=torch.float64) if rw is None else torch.tensor(rw.astype(np.float64))
    per_d = m * ((tg * td).sum(1) - zt) ** 2
    per_v = m * (tg * tv.t()).sum(1)
    (ld * (rwt * per_d).sum() / B + lv * (rwt * per_v).sum() / B).backward()
    want = {"depth": float((ld * per_d.sum() / B).detach()),
            "depth_var": float((lv * per_v.sum() / B).detach())}

    def run(init):
        d_depth = torch.full((B, K), init, device=cuda)
        d_gate = torch.full((B, K), init, device=cuda)
        terms, d_dvar = fused_depth_loss(_t(depth, cuda), _t(gate, cuda), _t(V, cuda), _t(z, cuda),
                                         None if rw is None else _t(rw, cuda), ld, lv, d_depth, d_gate)
        return terms, d_depth, d_gate, d_dvar

    terms, d_depth, d_gate, d_dvar = run(0.0)
    assert set(terms) == {"depth", "depth_var"}
    for k in want:
        err = abs(float(terms[k]) - want[k])
        print(f"K {K} weighted {weighted}: {k} {float(terms[k]):.6e} vs fp64 {want[k]:.6e}")
        assert err <= 1e-5 * max(1.0, abs(want[k])), k
    close = lambda a, b: torch.allclose(a.cpu().double(), b, rtol=1e-4, atol=1e-9)
    assert close(d_depth, td.grad) and close(d_gate, tg.grad) and close(d_dvar, tv.grad)
    inv = torch.from_numpy(z <= 0).to(cuda)
    assert not d_depth[inv].any() and not d_gate[inv].any() and not d_dvar[:, inv].any()
    assert bool(d_depth[~inv].any()) and bool(d_dvar[:, ~inv].any())
    # two calls: the same bits, terms included
    again = run(0.0)
    assert all(torch.equal(terms[k], again[0][k]) for k in terms)
    for a, b in zip((d_depth, d_gate, d_dvar), again[1:]):
        assert torch.equal(a, b)
    # the seeds are added to what the buffers hold; dvar's is written
    t1, a_depth, a_gate, a_dvar = run(0.5)
    assert torch.equal(a_dvar, d_dvar)
    # (d_gate takes the two terms' seeds in two adds: a rounding of a value
    # near 0.5, 2^-25, per add)
    assert torch.equal(a_depth, 0.5 + d_depth)
    assert float((a_gate - (0.5 + d_gate)).abs().max()) <= 2.0 ** -23
    # the mean term alone: no dvar_k, no seed on it
    d0, g0 = torch.zeros(B, K, device=cuda), torch.zeros(B, K, device=cuda)
    t0, none = fused_depth_loss(_t(depth, cuda), _t(gate, cuda), None, _t(z, cuda), None, ld, 0.0,
                                d0, g0)
    assert none is None and set(t0) == {"depth"} and torch.equal(t0["depth"], terms["depth"])


# ---- 4. the whole step ------------------------------------------------------------------
def _depth_targets(sc, cuda, esf, seed):
    """per-ray targets around the scene's own expected depth, a third of them none"""
    to = lambda a: _t(a, cuda)
    with torch.no_grad():
        res = ml_render_fused(sc.m, sc.g, to(sc.o), to(sc.d), to(sc.d), noise=to(sc.noise),
                              exp_step_factor=esf)
        mean = (res["gating_code"] * res["depth"]).sum(1)
    gen = torch.Generator().manual_seed(seed)
    z = mean * (1 + 0.2 * torch.randn(mean.shape[0], generator=gen).to(cuda))
    z = torch.where(z > 0.02, z, torch.full_like(z, 0.5))
    z[::3] = 0.0
    return z.contiguous()


def _routed_reference(res, live, B, K):
    """the op-by-op render recombined under the fused step's selection `live`
    (held constant, as the chain differentiates it; the two gates differ by
    their MLPs' precision, so a near-tie could pick another pair): gate_used =
    gate on the live pairs and 0 elsewhere, without renormalisation; a dead
    pair contributes nothing and its depth is 0"""
    from radnerf_amd.losses import _ray_of
    gate = res["gating_code"].float()
    used = gate * live
    rgb = torch.zeros(B, 3, device=gate.device)
    op = torch.zeros(B, device=gate.device)
    for i in range(K):
        ws = res[f"ws_{i}"].float()
        ray, inside = _ray_of(res[f"rays_a_{i}"].long(), ws.shape[0])
        o_i = torch.zeros(B, device=gate.device).index_add(0, ray, ws * inside)
        rgb = rgb + res["independent_rgbs"][i].float() * used[:, i][:, None]
        op = op + o_i * used[:, i]
    return dict(res, rgb=rgb, opacity=op, depth=res["depth"].float() * live, gating_used=used)


# which terms a whole-step case trains with: both depth terms; the expected-depth
# term alone (plain composite kernels, no dvar_k in rn_depth_loss, on a routed
# step a gate seed from that term only); both with the distortion loss (the
# DIST + DEPTH composite kernels, dense chain)
CASES = [(0.5, 2, 384, False, "both"), (0.5, 2, 384, True, "both"),
         (16.0, 4, 256, False, "both"), (16.0, 4, 256, True, "both"),
         (0.5, 2, 384, False, "mean"), (16.0, 4, 256, True, "mean"),
         (0.5, 2, 384, False, "dist"), (16.0, 4, 256, False, "dist")]


@pytest.mark.parametrize("scale,K,B,routed,which", CASES)
def test_train_step_vs_opbyop_autograd(cuda, scale, K, B, routed, which):
    esf = 1 / 256 if scale > 0.5 else 0.0
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    m, g = sc.m, sc.g
    o, d, nz = (_t(a, cuda) for a in (sc.o, sc.d, sc.noise))
    tgt = torch.rand(B, 3, generator=torch.Generator().manual_seed(5)).to(cuda)
    z = _depth_targets(sc, cuda, esf, 7)
    clip = 0.5 if scale <= 0.5 else 4.0
    # (the routed loss's depth-mutual term covers the live pairs only; it has
    # its own test, tests/test_gpu_routed.py, and stays out of this one)
    lambdas = dict(lambda_opacity=1e-3, lambda_cv_importance=1e-2,
                   lambda_depth_mutual=0.0 if routed else 5e-2, lambda_depth=1.0,
                   lambda_depth_var=0.0 if which == "mean" else 1.0, depth_clip=clip)
    if which == "dist":
        # the weight at which the distortion term carries a tenth of the gradient
        # at these shapes (tests/test_gpu_distortion.py LAMBDA)
        lambdas["lambda_distortion"] = 1.0 if scale <= 0.5 else 0.1
    on = ["lambda_depth"] + ([] if which == "mean" else ["lambda_depth_var"])
    route = dict(gate_topk=1) if routed else {}
    bg = torch.ones(3, device=cuda) if esf == 0 else torch.zeros(3, device=cuda)
    # the fused step (the second backward of a workspace runs the fixed-point scatter)
    r = FusedMLRenderer(m, g, B)
    for _ in range(2):
        terms, grads = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, target_depth=z,
                                    **lambdas, **route)
    grads = [x.clone() for x in grads]
    # op-by-op: the reference's autograd structure, the terms composed in torch
    m.zero_grad(); g.zero_grad()
    res = ml_render(m, g, o, d, d, noise=nz, exp_step_factor=esf, fused=False, distortion=True)
    assert "depth_var" not in res
    if routed:
        live = r.last_forward["live"].float()
        assert float((live == 0).float().mean()) >= 0.25 and bool((live.sum(1) == 1).all())
        if which != "mean":
            assert not r.ws.dvar_k.t()[live == 0].any()       # a dead pair has no samples
        res = _routed_reference(res, live, B, K)
    ld = NeRFLoss()(res, {"rgb": tgt, "depth": z}, **lambdas)
    assert "depth" in ld and ("depth_var" in ld) == (which != "mean")
    assert ("distortion" in ld) == (which == "dist")
    sum(v.mean() for v in ld.values()).backward()
    ref = [m.xyz_encoder.params.grad.clone(), m.mlp_params.grad.clone(), g.params.grad.clone()]
    assert set(terms) == set(ld)
    for k in ld:
        want = float(ld[k].mean().detach())
        print(f"scale {scale} K {K} routed {routed} {which}: {k} {float(terms[k]):.6e} vs "
              f"{want:.6e}")
        assert abs(float(terms[k]) - want) <= 1e-5 * max(1.0, abs(want)), k
    print("  gradients rel " + ", ".join(f"{_rel(a, b):.2e}" for a, b in zip(grads, ref)))
    for a, b in zip(grads, ref):
        assert _rel(a, b) <= 1e-3
    # the terms are live: each moves the grid gradient by more than 10x the bar
    # it was compared at, so a backward without it could not have passed
    for off in on:
        _, g0 = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, target_depth=z,
                             **dict(lambdas, **{off: 0.0}), **route)
        moved = _rel(grads[0], g0[0])
        print(f"  grid gradient moves {moved:.3f} with {off} -> 0")
        assert moved > 10 * 1e-3
    terms0, _ = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, **route,
                             **{k: v for k, v in lambdas.items() if "depth" not in k or "mutual" in k})
    assert "depth" not in terms0 and "depth_var" not in terms0
    if routed or which != "both":
        return
    # a strided view of the targets (a column of an image-shaped map) is the
    # same step: one contiguous copy serves the composite and the loss
    wide = torch.stack([z, torch.full_like(z, -3.0)], 1)
    assert not wide[:, 0].is_contiguous()
    t_s, g_s = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, target_depth=wide[:, 0],
                            **lambdas)
    t_c, g_c = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, target_depth=z, **lambdas)
    # (the depth terms are ordered sums of a deterministic forward: equal bits;
    # the default step's rgb / opacity sums are fp32 atomics in arrival order)
    assert torch.equal(t_s["depth"], t_c["depth"]) and torch.equal(t_s["depth_var"], t_c["depth_var"])
    assert torch.equal(t_s["depth"], terms["depth"]) and torch.equal(t_s["depth_var"], terms["depth_var"])
    for x, y in zip(g_s, g_c):
        assert _rel(x, y) <= 1e-4
    with pytest.raises(ValueError, match="depth targets must be on the rays' device"):
        r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, target_depth=z.cpu(), **lambdas)
    # the autograd surface: results["depth_var"] with a working backward
    for _ in range(2):
        m.zero_grad(); g.zero_grad()
        rf = ml_render_fused(m, g, o, d, d, noise=nz, exp_step_factor=esf, depth_target=z,
                             depth_clip=clip)
        lf = NeRFLoss()(rf, {"rgb": tgt, "depth": z}, **lambdas)
        sum(v.mean() for v in lf.values()).backward()
    a = rf["depth_var"].detach().cpu().numpy()
    b = composed_depth_var(res, z, clip).detach().cpu().numpy()
    assert a.shape == (B, K) and a.dtype == np.float32 and not a[z.cpu().numpy() <= 0].any()
    print(f"  depth_var fused vs composed: max abs {np.abs(a - b).max():.2e} (max {b.max():.3e})")
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-7)
    for x, y in zip([m.xyz_encoder.params.grad, m.mlp_params.grad, g.params.grad], ref):
        assert _rel(x, y) <= 1e-3


# ---- 5. the default step ------------------------------------------------------------------
def test_default_step_unchanged_by_a_depth_step(cuda):
    B, K = 256, 2
    sc = S.parity_scene(K, B, device=cuda)
    m, g = sc.m, sc.g
    o, d, nz = (_t(a, cuda) for a in (sc.o, sc.d, sc.noise))
    sd = [_t(s, cuda) for s in sc.seeds]
    bg = torch.ones(3, device=cuda)
    z = _depth_targets(sc, cuda, 0.0, 8)
    r = FusedMLRenderer(m, g, B)
    r.trace = True
    r.grid_fx = False               # fp32 atomics in every step: the steps differ by the term only
    seed = torch.full((K, B), 1e-2 / B, device=cuda) * (z > 0)

    def step(depth):
        r.events = {}
        out = r.forward(o, d, d, nz, bg, depth_target=z, depth_clip=0.5) if depth \
            else r.forward(o, d, d, nz, bg)
        w = r.ws
        keep = [t.clone() for t in out[:4]] + [w.ws.clone(), w.opacity_k.clone()]
        r.backward(o, d, d, out[3], bg, *sd, None, 1e-4,
                   **({"dL_ddvar": seed.contiguous()} if depth else {}))
        keep += [w.dsigma.clone(), w.drgb.clone()]
        return keep, set(r.kernel_times_ms())

    a, ka = step(False)
    b, kb = step(True)
    c, kc = step(False)
    assert ka == kc and "composite_fw" in ka and "composite_bw" in ka
    assert "composite_depth_fw" in kb and "composite_depth_bw" in kb
    assert not any("depth" in k for k in ka)
    assert kb - ka == {"composite_depth_fw", "composite_depth_bw"}
    assert ka - kb == {"composite_fw", "composite_bw"}
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(a, c):
        assert same(x, y)
    for x, y in zip(a[:6] + a[7:], b[:6] + b[7:]):      # the depth step's plain outputs, drgb
        assert same(x, y)
    assert not same(a[6], b[6])                         # its dsigma carries the term
    # train_step: with both lambdas 0 the terms and the launches of before,
    # targets or not
    tgt = torch.rand(B, 3, generator=torch.Generator().manual_seed(5)).to(cuda)
    r.events = {}
    t0, _ = r.train_step(o, d, d, tgt, nz, bg)
    k0 = set(r.kernel_times_ms())
    r.events = {}
    t1, _ = r.train_step(o, d, d, tgt, nz, bg, target_depth=z)
    assert set(r.kernel_times_ms()) == k0 and set(t1) == set(t0) == {"rgb", "opacity"}
    # the autograd surface: no key without the targets, before or after
    for flag in (False, True, False):
        res = ml_render_fused(m, g, o, d, d, noise=nz, **({"depth_target": z} if flag else {}))
        assert ("depth_var" in res) == flag
        assert set(res) - {"depth_var"} == {"rgb", "independent_rgbs", "depth", "opacity",
                                            "gating_code", "gating_importance"}


# ---- 6. determinism and resume ------------------------------------------------------------
def _sphere_depths(cuda):
    """the analytic ray parameter of RES.dataset()'s sphere per (image, pixel):
    the directions are unit vectors, so the range is t; 0 where the ray misses"""
    dirs, poses, _ = RES.dataset(cuda)
    d = torch.einsum("pj,nij->npi", dirs, poses[:, :, :3])
    o = poses[:, None, :, 3].expand_as(d)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - RES.R_SPHERE ** 2)
    t = -b - torch.sqrt(disc.clamp_min(0))
    return torch.where((disc > 0) & (t > 0), t, torch.zeros_like(t)).contiguous()


@pytest.mark.parametrize("guided", [False, True])
def test_depth_trainer_is_reproducible_and_resumable(cuda, guided):
    K, scale, steps, cut = 2, 0.5, 20, 10
    maps = _sphere_depths(cuda)
    assert 0.1 < float((maps > 0).float().mean()) < 0.9
    # millimetres in uint16 (int16 storage of the words), as an RGB-D capture ships them
    mm = (maps * 1000).round().to(torch.int32).cpu().numpy().astype(np.uint16)
    td = TrainDepths(_t(mm.view(np.int16), cuda), scale=1e-3)
    kw = dict(img_wh=RES.WH, depths=td, lambda_depth=0.1, lambda_depth_var=0.5, depth_clip=0.5,
              guided=guided)
    a, b = RES.trainer(cuda, K, scale, False, **kw), RES.trainer(cuda, K, scale, False, **kw)
    la, lb = RES.run_steps(a, steps, []), RES.run_steps(b, cut, [])
    sd = b.state_dict()
    assert {k: sd["hyper"][k] for k in ("lambda_depth", "lambda_depth_var", "depth_clip")} == \
        {"lambda_depth": 0.1, "lambda_depth_var": 0.5, "depth_clip": 0.5}
    RES.run_steps(b, steps, lb)
    assert len(la) == len(lb) == steps and all(torch.equal(x, y) for x, y in zip(la, lb))
    end = RES.full_state(a)
    RES.assert_same_tensors(end, RES.full_state(b))         # two runs, the same bits
    c = RES.other_trainer(cuda, K, scale, False, **kw)
    c.load_state_dict(sd)
    lc = RES.run_steps(c, steps, [])
    assert all(torch.equal(x, y) for x, y in zip(la[cut:], lc))
    RES.assert_same_tensors(end, RES.full_state(c))         # saved at 10, resumed
    # the step did supervise depth: both terms are reported and positive, and the
    # targets are the maps' values at the batch's picks
    terms = a.step_sampled()
    assert float(terms["depth"]) > 0 and float(terms["depth_var"]) > 0
    bt = a.last_batch
    want = td.depths.view(-1).to(torch.int32).bitwise_and(0xffff)[
        bt["img_idxs"] * td.n_pix + bt["pix_idxs"]].float() * np.float32(1e-3)
    assert torch.equal(a._target_t, want)
    # a trainer without the terms refuses this state, and the other way round
    plain = RES.other_trainer(cuda, K, scale, False, img_wh=RES.WH, guided=guided)
    with pytest.raises(ValueError, match="lambda_depth"):
        plain.load_state_dict(sd)


# ---- 7. the sub-NeRF-per-GPU layout -------------------------------------------------------
def test_pinned_refuses_depth(cuda):
    B, K = 64, 2
    sc = S.parity_scene(K, B, device=cuda)
    o, d, nz = (_t(a, cuda) for a in (sc.o, sc.d, sc.noise))
    bg = torch.ones(3, device=cuda)
    z = torch.ones(B, device=cuda)
    r = PinnedMLRenderer(sc.m, sc.g, B)
    with pytest.raises(NotImplementedError, match="depth supervision"):
        r.forward(o, d, d, nz, bg, depth_target=z)
    for lam in ("lambda_depth", "lambda_depth_var"):
        with pytest.raises(NotImplementedError, match="depth supervision"):
            r.train_step(o, d, d, torch.zeros(B, 3, device=cuda), nz, bg, target_depth=z,
                         **{lam: 1e-2})
