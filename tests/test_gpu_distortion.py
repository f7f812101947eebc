"""GPU: the Mip-NeRF 360 distortion loss inside the fused training render
(rn_ml_composite_dist_fw / _bw, csrc/composite.hip) -- per (sub-NeRF, ray)
segment the loss of losses.cu:47-110 and its gradient of :113-142 fed through
VolumeRenderer's dL_dws terms, formed in the composite kernels' registers.

  1. kernel level, through lib(), on hand-made segments against the CPU oracle
     chain composite_train_fw -> distortion_loss_fw/_bw -> composite_train_bw;
  2. fused autograd chain vs the op-by-op chain (ml_render(fused=False,
     distortion=True): VolumeRenderer + DistortionLoss);
  3. render(distortion=True) of a single NGP;
  4. train_step(lambda_distortion) vs autograd + NeRFLoss;
  5. a distortion step between two default steps leaves the default step as
     it was; 6. the sub-NeRF-per-GPU renderer refuses the flag.

Bars (the project's own): per-ray loss rtol 2e-4 / atol 1e-7 (test_gpu_aux.py),
dsigma <= 1e-4 max(1, |ref|max) (test_gpu_parity.py), parameter gradients
1e-3 relative norm (test_gpu_ml.py), loss terms 1e-5 max(1, |ref|)
(test_gpu_train.py).
"""
import numpy as np
import pytest
import torch

import oracle
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from radnerf_amd.fused import SEG_ALIGN, FusedMLRenderer, get_renderer, ml_render_fused
from radnerf_amd.losses import DistortionLoss, NeRFLoss
from radnerf_amd.networks import NGP
from radnerf_amd.pinned import PinnedMLRenderer
from radnerf_amd.rendering import ml_render, render

pytestmark = pytest.mark.gpu

THR = 1e-4
K1, B1 = 2, 7          # 14 segments: 3.5 blocks of 4 waves
# samples per (sub-NeRF, ray) segment and where its transmittance ends:
# "never", "natural" (sigma high enough that T crosses the threshold somewhere
# inside, wherever the serial fold says) or the index of a sample so dense
# that T drops far below the threshold exactly there
SEGMENTS = [
    [(0, "never"), (1, "never"), (63, "never"), (64, 63), (65, "never"),
     (128, 64),             # lane 0 of the second chunk
     (129, 63)],            # lane 63 of the first chunk, 65 samples after it
    [(200, 100),            # mid-chunk
     (1024, 20),            # first chunk of 16: every later chunk on the `done` path
     (1024, "never"), (129, "natural"), (200, "natural"),
     (128, 127),            # lane 63 of the last chunk
     (1024, "natural")],
]


def _segments():
    """sigmas, rgbs, deltas, ts in the fused layout (sub-NeRF bases aligned to
    SEG_ALIGN, a sub-NeRF's segments back to back) + counts / offsets [K][B]."""
    rng = np.random.default_rng(21)
    counts = np.array([[n for n, _ in row] for row in SEGMENTS], np.int32)
    offsets = np.zeros_like(counts)
    base = 0
    for k in range(K1):
        base = -(-base // SEG_ALIGN) * SEG_ALIGN
        offsets[k] = base + np.concatenate([[0], np.cumsum(counts[k])[:-1]])
        base += int(counts[k].sum())
    cap = -(-base // SEG_ALIGN) * SEG_ALIGN
    sig = np.zeros(cap, np.float32)
    deltas = np.full(cap, 1e-3, np.float32)
    ts = np.zeros(cap, np.float32)
    rgbs = rng.random((cap, 3), dtype=np.float32)
    for k in range(K1):
        for r in range(B1):
            n, end = SEGMENTS[k][r]
            if n == 0:
                continue
            a = int(offsets[k, r])
            dl = rng.uniform(1e-3, 5e-3, n).astype(np.float32)
            deltas[a:a + n] = dl
            ts[a:a + n] = (np.cumsum(dl, dtype=np.float64) + rng.uniform(0.3, 1.0)).astype(np.float32)
            # optical depth sum(sigma delta): 2 (T ends at ~0.13), 15 (T crosses
            # 1e-4 = exp(-9.2) at ~0.6 n) or 0.7 before the forced sample
            tau = {"never": 2.0, "natural": 15.0}.get(end, 0.7)
            m = n if isinstance(end, str) else end + 1
            s = rng.uniform(0, 2 * tau / m, n) / dl
            s[rng.random(n) < 0.2] = 0.0
            if not isinstance(end, str):
                s[end] = 30.0 / dl[end]
            sig[a:a + n] = s
    return sig, rgbs, deltas, ts, counts, offsets


def _seg_seeds(gate, bg, gRGB, gO, gDepth):
    """the composite's per-segment seeds as k_ml_composite_bw folds them out of
    the combine's (fp32, same operation order)"""
    f = np.float32
    gr = (gate.T[:, :, None] * gRGB[None]).astype(f)                    # [K][B][3]
    bgdot = (f(bg[0]) * gRGB[:, 0] + f(bg[1]) * gRGB[:, 1]).astype(f)
    bgdot = (bgdot + f(bg[2]) * gRGB[:, 2]).astype(f)
    go = (gate.T * (gO - bgdot)[None]).astype(f)                        # [K][B]
    return gr.reshape(-1, 3), go.reshape(-1), np.ascontiguousarray(gDepth.T).reshape(-1)


@pytest.fixture(scope="module")
def kernel_case():
    """Inputs, seeds and the CPU reference of test 1, computed once."""
    sig, rgbs, deltas, ts, counts, offsets = _segments()
    rng = np.random.default_rng(22)
    n_seg = K1 * B1
    gate = rng.random((B1, K1)).astype(np.float32)
    gate /= gate.sum(1, keepdims=True)
    bg = rng.random(3).astype(np.float32)
    gRGB = rng.normal(0, 1, (B1, 3)).astype(np.float32)
    gO = rng.normal(0, 1, B1).astype(np.float32)
    gDepth = rng.normal(0, 1, (B1, K1)).astype(np.float32)
    gdist = rng.normal(0, 1, (K1, B1)).astype(np.float32)
    rows = np.stack([np.arange(n_seg), offsets.reshape(-1), counts.reshape(-1)], 1).astype(np.int64)
    used, op, de, rgb, ws = oracle.composite_train_fw(sig, rgbs, deltas, ts, rows, THR)
    loss, wi, wti = oracle.distortion_loss_fw(ws, deltas, ts, rows)
    dws = oracle.distortion_loss_bw(gdist.reshape(-1), wi, wti, ws, deltas, ts, rows)
    sr, so, sd = _seg_seeds(gate, bg, gRGB, gO, gDepth)
    dsig, drgb = oracle.composite_train_bw(so, sd, sr, dws, sig, rgbs, ws, deltas, ts, rows, op, de,
                                           rgb, THR)
    # the cases the segments were built for did come out
    want = {(0, 3): 63, (0, 5): 64, (0, 6): 63, (1, 0): 100, (1, 1): 20, (1, 5): 127}
    u = used.reshape(K1, B1)
    for (k, r), v in want.items():
        assert u[k, r] == v
    for k in range(K1):
        for r in range(B1):
            n, end = SEGMENTS[k][r]
            if end == "never":
                assert u[k, r] == n
            elif end == "natural":
                assert 0 < u[k, r] < n - 1
    return dict(sig=sig, rgbs=rgbs, deltas=deltas, ts=ts, counts=counts, offsets=offsets, gate=gate,
                bg=bg, gRGB=gRGB, gO=gO, gDepth=gDepth, gdist=gdist, rows=rows, seeds=(sr, so, sd),
                ref=dict(used=used, op=op, de=de, rgb=rgb, ws=ws, loss=loss, dsig=dsig, drgb=drgb))


def _inside(c):
    """mask of the sample slots inside a segment (the padding is never written)"""
    m = np.zeros(len(c["sig"]), bool)
    for a, n in zip(c["offsets"].reshape(-1), c["counts"].reshape(-1)):
        m[a:a + n] = True
    return m


def test_kernels_vs_oracle(cuda, kernel_case):
    """Measured on an MI355X (the test prints them): dist_k max relative error
    vs the fp32 oracle 1.96e-05 in-chain, 1.60e-05 for the explicit GPU form
    (the oracle itself is 2.0e-05 off the float64 definition on these
    segments); dsigma L_inf 1.44e-08 for both at |ref|max 6.72e-03, so the
    explicit form meets the 1e-4 max(1, |ref|max) bar and the bar stands."""
    c, L = kernel_case, lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    st = torch.cuda.current_stream(cuda).cuda_stream
    sig, rgbs, dl, ts = t(c["sig"]), t(c["rgbs"]), t(c["deltas"]), t(c["ts"])
    cnt, off = t(c["counts"]), t(c["offsets"])
    gate, bg, gRGB, gO, gD = (t(c[k]) for k in ("gate", "bg", "gRGB", "gO", "gDepth"))
    gdist = t(c["gdist"])
    cap, n_seg = len(c["sig"]), K1 * B1
    inside = torch.from_numpy(_inside(c)).to(cuda)

    def forward(dist):
        o = dict(used=torch.full((K1, B1), -7, device=cuda, dtype=torch.int32),
                 op=torch.full((K1, B1), -7.0, device=cuda), de=torch.full((K1, B1), -7.0, device=cuda),
                 rgb=torch.full((K1, B1, 3), -7.0, device=cuda), ws=torch.full((cap,), -7.0, device=cuda))
        args = (sig.data_ptr(), rgbs.data_ptr(), dl.data_ptr(), ts.data_ptr(), cnt.data_ptr(),
                off.data_ptr(), B1, K1, THR, o["used"].data_ptr(), o["op"].data_ptr(),
                o["de"].data_ptr(), o["rgb"].data_ptr(), o["ws"].data_ptr())
        if dist:
            o["dist"] = torch.full((K1, B1), -7.0, device=cuda)
            L.ml_composite_dist_fw(*args, o["dist"].data_ptr(), st)
        else:
            L.ml_composite_fw(*args, st)
        return o

    plain, var = forward(False), forward(True)
    # every plain output of the variant is the plain kernel's, bit for bit
    for k in ("used", "op", "de", "rgb", "ws"):
        assert torch.equal(plain[k], var[k]), k
    assert torch.equal(var["ws"][~inside], torch.full_like(var["ws"][~inside], -7.0))
    ref = c["ref"]
    assert np.array_equal(var["used"].cpu().numpy().reshape(-1), ref["used"])   # termination bit-exact
    dist = var["dist"].cpu().numpy().reshape(-1)

    def backward(seed):
        dsig = torch.full((cap,), -7.0, device=cuda)
        drgb = torch.full((cap, 3), -7.0, device=cuda)
        common = (gate.data_ptr(), bg.data_ptr(), sig.data_ptr(), rgbs.data_ptr(), dl.data_ptr(),
                  ts.data_ptr())
        tail = (cnt.data_ptr(), off.data_ptr(), var["op"].data_ptr(), var["de"].data_ptr(),
                var["rgb"].data_ptr())
        if seed is None:
            L.ml_composite_bw(gRGB.data_ptr(), gO.data_ptr(), gD.data_ptr(), *common, *tail, B1, K1,
                              THR, dsig.data_ptr(), drgb.data_ptr(), st)
        else:
            ptr, const = (seed.data_ptr(), 0.0) if torch.is_tensor(seed) else (None, seed)
            L.ml_composite_dist_bw(gRGB.data_ptr(), gO.data_ptr(), gD.data_ptr(), ptr, const, *common,
                                   var["ws"].data_ptr(), *tail, var["dist"].data_ptr(), B1, K1, THR,
                                   dsig.data_ptr(), drgb.data_ptr(), st)
        return dsig, drgb

    p_dsig, p_drgb = backward(None)
    v_dsig, v_drgb = backward(gdist)
    z_dsig, z_drgb = backward(torch.zeros_like(gdist))
    c_dsig, _ = backward(0.0)
    assert torch.equal(v_drgb, p_drgb) and torch.equal(z_drgb, p_drgb)      # drgb untouched
    assert torch.equal(z_dsig, p_dsig) and torch.equal(c_dsig, p_dsig)      # zero seed = plain
    # a constant seed is the same as a buffer filled with it
    k_dsig, _ = backward(0.25)
    f_dsig, _ = backward(torch.full_like(gdist, 0.25))
    assert torch.equal(k_dsig, f_dsig)

    # the explicit GPU form on the same inputs: rn_distortion_loss_fw/_bw with
    # its three sample-sized arrays, then rn_composite_train_bw with dL_dws
    rows = t(c["rows"])
    e_loss = torch.zeros(n_seg, device=cuda)
    wi, wti, dws = (torch.zeros(cap, device=cuda) for _ in range(3))
    L.distortion_loss_fw(var["ws"].data_ptr(), dl.data_ptr(), ts.data_ptr(), rows.data_ptr(), n_seg,
                         e_loss.data_ptr(), wi.data_ptr(), wti.data_ptr(), st)
    L.distortion_loss_bw(gdist.data_ptr(), wi.data_ptr(), wti.data_ptr(), var["ws"].data_ptr(),
                         dl.data_ptr(), ts.data_ptr(), rows.data_ptr(), n_seg, dws.data_ptr(), st)
    sr, so, sd = (t(a) for a in c["seeds"])
    e_dsig = torch.zeros(cap, device=cuda)
    e_drgb = torch.zeros(cap, 3, device=cuda)
    L.composite_train_bw(so.data_ptr(), sd.data_ptr(), sr.data_ptr(), dws.data_ptr(), sig.data_ptr(),
                         rgbs.data_ptr(), var["ws"].data_ptr(), dl.data_ptr(), ts.data_ptr(),
                         rows.data_ptr(), n_seg, var["op"].data_ptr(), var["de"].data_ptr(),
                         var["rgb"].data_ptr(), THR, e_dsig.data_ptr(), e_drgb.data_ptr(), st)

    m = inside.cpu().numpy()
    scale = max(1.0, float(np.abs(ref["dsig"]).max()))
    err = lambda a: float(np.abs(a.cpu().numpy()[m] - ref["dsig"][m]).max())
    rel = lambda a: float(np.max(np.abs(a - ref["loss"]) / np.maximum(np.abs(ref["loss"]), 1e-30)))
    print(f"dist_k vs oracle: in-chain max rel {rel(dist):.2e}, explicit {rel(e_loss.cpu().numpy()):.2e}; "
          f"dsigma L_inf vs oracle (|ref|max {np.abs(ref['dsig']).max():.3e}): in-chain "
          f"{err(v_dsig):.2e}, explicit {err(e_dsig):.2e}; plain part alone "
          f"{float((p_dsig[inside] - v_dsig[inside]).abs().max()):.2e} from the seeded one")
    np.testing.assert_allclose(dist, ref["loss"], rtol=2e-4, atol=1e-7)
    assert err(v_dsig) <= 1e-4 * scale
    assert np.abs(v_drgb.cpu().numpy()[m] - ref["drgb"][m]).max() <= 1e-4
    # the seed's share of dsigma stands well above the bar it is checked at
    assert float((p_dsig[inside] - v_dsig[inside]).abs().max()) > 10 * 1e-4 * scale


# lambda on distortion.mean(0).sum(): the smallest power of ten at which the
# grid gradient of the op-by-op chain moves by >= 10 % (relative norm) from the
# lambda = 0 gradient at these shapes, against seeds of 1e-3 per ray element
# (S.loss_seeds).  Measured: scale 0.5, K = 2: 0.052 at 0.1, 0.52 at 1; scale
# 16, K = 4: 0.036 at 0.01, 0.36 at 0.1.
LAMBDA = {0.5: 1.0, 16.0: 0.1}


def _loss_backward(fn, m, g, o, d, noise, seeds, cuda, esf, lam, **kw):
    m.zero_grad(); g.zero_grad()
    to = lambda a: torch.from_numpy(a).to(cuda)
    res = fn(m, g, to(o), to(d), to(d), noise=to(noise), exp_step_factor=esf, **kw)
    outs = [res["rgb"], res["opacity"], res["depth"]]
    grads = [to(s) for s in seeds]
    if lam:
        outs.append(lam * res["distortion"].mean(0).sum())
        grads.append(torch.ones((), device=cuda))
    torch.autograd.backward(outs, grads)
    return res, [m.xyz_encoder.params.grad.clone(), m.mlp_params.grad.clone(), g.params.grad.clone()]


_rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("scale,K,B", [(0.5, 2, 384), (16.0, 4, 256)])
def test_fused_vs_opbyop_autograd(cuda, scale, K, B):
    esf = 1 / 256 if scale > 0.5 else 0.0
    lam = LAMBDA[scale]
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    m, g, o, d, noise, seeds, bits = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bits
    args = (m, g, o, d, noise, seeds, cuda, esf)
    _, g0 = _loss_backward(ml_render, *args, 0.0, fused=False)
    rd, gd = _loss_backward(ml_render, *args, lam, fused=False, distortion=True)
    _, g_less = _loss_backward(ml_render, *args, lam / 10, fused=False, distortion=True)
    moved, moved_less = _rel(gd[0], g0[0]), _rel(g_less[0], g0[0])
    print(f"scale {scale} K {K}: grid gradient moves {moved:.3f} at lambda {lam:g}, "
          f"{moved_less:.3f} at {lam / 10:g}")
    assert moved >= 0.1 > moved_less        # the smallest power of ten that matters
    for i in range(K):          # the reference's per-sub-NeRF keys (losses.py:63-67)
        for key in ("ws", "deltas", "ts", "rays_a"):
            assert f"{key}_{i}" in rd
    _loss_backward(ml_render_fused, *args, lam, distortion=True)      # fp32 step (fx scales)
    rf, gf = _loss_backward(ml_render_fused, *args, lam, distortion=True)
    a, b = rf["distortion"].detach().cpu().numpy(), rd["distortion"].detach().cpu().numpy()
    assert a.shape == (B, K) and a.dtype == np.float32
    print(f"  distortion fused vs op-by-op: max rel {np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)):.2e}"
          f" (max {b.max():.3e}); gradients rel " + ", ".join(f"{_rel(x, y):.2e}" for x, y in zip(gf, gd)))
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-7)
    for x, y in zip(gf, gd):
        assert _rel(x, y) <= 1e-3
    # NeRFLoss reads the key on both chains
    for res in (rf, rd):
        ld = NeRFLoss()(res, {"rgb": torch.zeros(B, 3, device=cuda)}, lambda_distortion=lam)
        want = lam * res["distortion"].mean(0).sum()
        assert abs(float(ld["distortion"].detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))


def test_render_single_ngp(cuda):
    scale, B, lam = 0.5, 512, LAMBDA[0.5]
    m = NGP(scale, seed=3)
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(1, LY.FIELD_PARAMS)))
    S.set_bitfields(m, S.bitfields(1, m.cascades, p=0.5))
    m = m.to(cuda)
    o, d = (torch.from_numpy(a).to(cuda) for a in S.rays(B, scale))
    nz = torch.from_numpy(S.noise(1, B)[0]).to(cuda)
    seeds = [torch.from_numpy(s).to(cuda) for s in S.loss_seeds(B, 1)]
    grads = []
    for with_dist in (False, True, False, True):     # the first backward of a workspace is fp32
        m.zero_grad()
        res = render(m, o, d, noise=nz, distortion=with_dist)
        assert ("distortion" in res) == with_dist
        outs, gr = [res["rgb"], res["opacity"], res["depth"]], [seeds[0], seeds[1], seeds[2][:, 0]]
        if with_dist:
            dist = res["distortion"]
            assert dist.shape == (B,) and dist.dtype == torch.float32
            want = DistortionLoss.apply(res["ws"].detach(), res["deltas"], res["ts"],
                                        res["rays_a"].long())
            a, b = dist.detach().cpu().numpy(), want.cpu().numpy()
            print(f"render(): distortion vs DistortionLoss on its own samples: max rel "
                  f"{np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)):.2e} (max {b.max():.3e})")
            np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-7)
            assert b.max() > 0
            outs.append(lam * dist.mean())
            gr.append(torch.ones((), device=cuda))
        torch.autograd.backward(outs, gr)
        grads.append(m.xyz_encoder.params.grad.clone())
    assert torch.isfinite(grads[3]).all()
    moved = _rel(grads[3], grads[2])
    print(f"render(): grid gradient moves {moved:.3f} with lambda {lam:g}")
    assert moved >= 0.1
    # ws keeps refusing a gradient
    res = render(m, o, d, noise=nz, distortion=True)
    with pytest.raises(RuntimeError, match="does not back-propagate"):
        res["ws"].sum().backward()


@pytest.mark.parametrize("B,K,scale", [(512, 2, 0.5), (512, 4, 16.0)])
def test_train_step_matches_autograd(cuda, B, K, scale):
    esf = 1 / 256 if scale > 0.5 else 0.0
    # the distortion weight at which the term carries a tenth of the gradient
    # against per-ray seeds of ~1e-3; here the rgb term's seeds are ~1e-3 too
    # ((rgb - target) 2 / 3B with B = 512)
    lambdas = dict(lambda_opacity=1e-3, lambda_cv_importance=1e-2, lambda_depth_mutual=5e-2,
                   lambda_distortion=LAMBDA[scale])
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    m, g, o, d, noise = sc.m, sc.g, sc.o, sc.d, sc.noise
    o, d, nz = (torch.from_numpy(a).to(cuda) for a in (o, d, noise))
    tgt = torch.rand(B, 3, generator=torch.Generator().manual_seed(5)).to(cuda)
    ref = None
    for _ in range(2):          # the second backward runs the fixed-point scatter
        m.zero_grad(); g.zero_grad()
        res = ml_render_fused(m, g, o, d, d, noise=nz, exp_step_factor=esf, distortion=True)
        ld = NeRFLoss()(res, {"rgb": tgt}, **lambdas)
        assert "distortion" in ld
        sum(v.mean() for v in ld.values()).backward()
        ref = [m.xyz_encoder.params.grad.clone(), m.mlp_params.grad.clone(), g.params.grad.clone()]
    r = get_renderer(m, g, B)
    bg = torch.ones(3, device=cuda) if esf == 0 else torch.zeros(3, device=cuda)
    terms, grads = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, **lambdas)
    assert set(terms) == set(ld)
    for k in ld:
        want = float(ld[k].mean().detach())
        assert abs(float(terms[k]) - want) <= 1e-5 * max(1.0, abs(want)), k
    print(f"train_step: distortion term {float(terms['distortion']):.4e}; gradients rel "
          + ", ".join(f"{_rel(a, b):.2e}" for a, b in zip(grads, ref)))
    for a, b in zip(grads, ref):
        assert _rel(a, b) <= 1e-3
    # the term is live: without it the grid gradient is another one
    lambdas["lambda_distortion"] = 0.0
    terms0, grads0 = r.train_step(o, d, d, tgt, nz, bg, exp_step_factor=esf, **lambdas)
    assert "distortion" not in terms0
    moved = _rel(grads[0], grads0[0])
    print(f"  grid gradient moves {moved:.3f} with lambda {LAMBDA[scale]:g} -> 0")
    assert moved >= 0.1


def test_default_step_unchanged_by_a_distortion_step(cuda):
    B, K = 256, 2
    sc = S.parity_scene(K, B, device=cuda)
    m, g, o, d, noise, seeds = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds
    o, d, nz = (torch.from_numpy(a).to(cuda) for a in (o, d, noise))
    sd = [torch.from_numpy(s).to(cuda) for s in seeds]
    bg = torch.ones(3, device=cuda)
    r = FusedMLRenderer(m, g, B)
    r.trace = True
    r.grid_fx = False               # fp32 atomics in every step: the steps differ by the flag only

    def step(dist):
        r.events = {}
        out = r.forward(o, d, d, nz, bg, distortion=True) if dist else r.forward(o, d, d, nz, bg)
        w = r.ws
        keep = [t.clone() for t in out[:4]] + [w.ws.clone(), w.opacity_k.clone()]
        r.backward(o, d, d, out[3], bg, *sd, None, 1e-4,
                   **({"dL_ddist": 1e-2 / B} if dist else {}))
        keep += [w.dsigma.clone(), w.drgb.clone()]
        return keep, set(r.kernel_times_ms())

    a, ka = step(False)
    b, kb = step(True)
    c, kc = step(False)
    assert ka == kc and "composite_fw" in ka and "composite_bw" in ka
    assert "composite_dist_fw" in kb and "composite_dist_bw" in kb
    assert not any("dist" in k for k in ka)
    # bit patterns: the padding between the sub-NeRFs' samples is never written
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(a, c):
        assert same(x, y)
    for x, y in zip(a[:6] + a[7:], b[:6] + b[7:]):    # the distortion step's plain outputs, drgb
        assert same(x, y)
    assert not same(a[6], b[6])         # and its backward's dsigma carries the term
    # the autograd surface: no key without the flag, before or after
    for flag in (False, True, False):
        res = ml_render_fused(m, g, o, d, d, noise=nz, **({"distortion": True} if flag else {}))
        assert ("distortion" in res) == flag
        assert set(res) - {"distortion"} == {"rgb", "independent_rgbs", "depth", "opacity",
                                             "gating_code", "gating_importance"}


def test_pinned_refuses_distortion(cuda):
    B, K = 64, 2
    sc = S.parity_scene(K, B, device=cuda)
    m, g, o, d, noise, seeds = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds
    o, d, nz = (torch.from_numpy(a).to(cuda) for a in (o, d, noise))
    bg = torch.ones(3, device=cuda)
    r = PinnedMLRenderer(m, g, B)
    with pytest.raises(NotImplementedError, match="distortion"):
        r.forward(o, d, d, nz, bg, distortion=True)
    with pytest.raises(NotImplementedError, match="distortion"):
        r.train_step(o, d, d, torch.zeros(B, 3, device=cuda), nz, bg, lambda_distortion=1e-2)
