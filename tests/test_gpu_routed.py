"""GPU: routed training -- the step that marches and differentiates only the
(ray, sub-NeRF) pairs the gate keeps (DESIGN.md §4 "Routed training").

  * rn_gate_select_bw against its numpy fp32 restatement (route_ref), bit for
    bit, plain and renormalised, in place and out of place;
  * rn_ml_march_count_list: a listed pair gets rn_ml_march_count's bits in any
    list order, an unlisted pair count 0 and an untouched staging slot;
  * with every pair live the routed launches reproduce the dense step bit for
    bit (deterministic mode);
  * a routed step against the restated oracle (route_ref.routed_train_step)
    with the GPU's own selection;
  * a uniform gate under top-1: sub-NeRFs 1..K-1 get no ray, no sample and an
    exactly zero gradient, and the step finishes;
  * the default arguments issue none of the routed launches;
  * Trainer: routed runs are reproducible and resumable, validate(**routing).
"""
import numpy as np
import pytest
import torch

import resume_ref as RES
import route_ref as RR
from gate_select_ref import gate_rows, select_ref
from parity import GATE_TOL, check_grads, rel
from radnerf_amd import _lib
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd.fused import (MAX_SAMPLES, NEAR_DISTANCE, FusedMLRenderer, get_renderer,
                               ml_render_fused)

pytestmark = pytest.mark.gpu
GUARD = 64
GATE_SEED = 9       # the gate whose selections meet the conditions _conditions() asserts


class Guarded:
    """n elements between two runs of GUARD guard elements"""

    def __init__(self, n, dtype, fill, dev):
        self.guard = {torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.float32: -1234.5}[dtype]
        self.all = torch.full((n + 2 * GUARD,), self.guard, dtype=dtype, device=dev)
        self.t = self.all[GUARD:GUARD + n]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.all[:GUARD] == self.guard).all()) and \
            bool((self.all[-GUARD:] == self.guard).all())


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- rn_gate_select_bw ------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 9, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_gate_select_bw_vs_restatement(cuda, n, K):
    L = _lib.lib()
    g_np = gate_rows(n, K, seed=10 * K + n)
    d_np = np.random.default_rng(n + K).standard_normal((n, K)).astype(np.float32)
    gate = _t(g_np, cuda)
    for tau, k in ((0.0, 1), (0.0, min(2, K)), (0.2, None), (0.0, None)):
        sel = select_ref(g_np, tau, k)
        live = Guarded(n * K, torch.uint8, 0, cuda)
        live.t.copy_(_t(sel["live"].reshape(-1), cuda))
        for renorm in (False, True):
            want = RR.select_bw_ref(g_np, sel["live"], d_np, renorm)
            for in_place in (False, True):
                d = Guarded(n * K, torch.float32, 0.0, cuda)
                d.t.copy_(_t(d_np.reshape(-1), cuda))
                out = d if in_place else Guarded(n * K, torch.float32, 7.5, cuda)
                L.gate_select_bw(gate.data_ptr(), live.t.data_ptr(), d.t.data_ptr(), n, K,
                                 int(renorm), out.t.data_ptr(), _st(cuda))
                got = out.t.cpu().numpy().reshape(n, K)
                tag = (n, K, tau, k, renorm, in_place)
                assert np.array_equal(got, want, equal_nan=True), tag
                assert not got[sel["live"] == 0].any(), tag
                assert out.intact() and d.intact() and live.intact(), tag
                if not in_place:
                    assert np.array_equal(d.t.cpu().numpy().reshape(n, K), d_np), tag


# ---- rn_ml_march_count_list -------------------------------------------------------
def _march_args(cuda, B, K, scale):
    cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)
    esf = 1 / 256 if scale > 0.5 else 0.0
    o, d = S.rays(B, scale)
    bits = S.bitfields(K, cascades, p=0.5)
    keep = [_t(a, cuda) for a in (o, d, np.zeros(3, np.float32), np.full(3, scale, np.float32),
                                  S.noise(K, B), bits)]
    args = (keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
            NEAR_DISTANCE, keep[4].data_ptr(), keep[5].data_ptr(), bits.shape[1], K, cascades,
            float(scale), esf, 128, MAX_SAMPLES, B)
    return args, keep


STAGE_GUARD = -4321.0


def _list_march(cuda, L, args, B, K, lists):
    """rn_ml_march_count_list on `lists` (K arrays of ray indices) with a dirty
    counts buffer; returns (counts (K, B), stage_ts, stage_dt (K*B, MAX))."""
    cnt = Guarded(K * B, torch.int32, 123456, cuda)             # dirty on entry
    ts = Guarded(K * B * MAX_SAMPLES, torch.float32, STAGE_GUARD, cuda)
    dt = Guarded(K * B * MAX_SAMPLES, torch.float32, STAGE_GUARD, cuda)
    lst = Guarded(K * B, torch.int32, -99, cuda)
    count = Guarded(K, torch.int32, 0, cuda)
    for k, rays in enumerate(lists):
        assert len(rays) <= B
        lst.t[k * B:k * B + len(rays)].copy_(_t(np.array(rays, np.int32), cuda))   # (a copy)
    count.t.copy_(_t(np.array([len(r) for r in lists], np.int32), cuda))
    L.ml_march_count_list(*args, cnt.t.data_ptr(), ts.t.data_ptr(), dt.t.data_ptr(),
                          lst.t.data_ptr(), count.t.data_ptr(), _st(cuda))
    torch.cuda.synchronize()
    assert all(b.intact() for b in (cnt, ts, dt, lst, count))
    return (cnt.t.cpu().numpy().reshape(K, B), ts.t.view(K * B, MAX_SAMPLES),
            dt.t.view(K * B, MAX_SAMPLES))


def _check_listed(tag, B, K, lists, got, dense):
    cnt, ts, dt = got
    dcnt, dts, ddt = dense
    listed = np.zeros((K, B), bool)
    for k, rays in enumerate(lists):
        rays = np.asarray(rays, np.int64)
        listed[k, rays[(rays >= 0) & (rays < B)]] = True
    assert np.array_equal(cnt, np.where(listed, dcnt, 0)), tag
    flat = torch.from_numpy(listed.reshape(-1)).to(ts.device)
    used = torch.arange(MAX_SAMPLES, device=ts.device)[None, :] < \
        torch.from_numpy(cnt.reshape(-1).astype(np.int64)).to(ts.device)[:, None]
    for name, a, b in (("ts", ts, dts), ("dt", dt, ddt)):
        ai, bi = a.view(torch.int32), b.view(torch.int32)
        # live pairs: the dense kernel's bits in the slots it wrote
        assert torch.equal(ai[used], bi[used]), (tag, name)
        # everything else (dead pairs' slots, slots past a count) keeps the guard
        assert bool((a[~used] == STAGE_GUARD).all()), (tag, name)
    assert not used[~flat].any()


@pytest.mark.parametrize("scale", [0.5, 16.0])
@pytest.mark.parametrize("K", [2, 3, 9])
@pytest.mark.parametrize("B", [1, 5, 64, 259])
def test_list_march_is_the_dense_march_on_listed_pairs(cuda, B, K, scale):
    L = _lib.lib()
    args, keep = _march_args(cuda, B, K, scale)
    dcnt = torch.full((K * B,), -1, dtype=torch.int32, device=cuda)
    dts = torch.full((K * B, MAX_SAMPLES), STAGE_GUARD, device=cuda)
    ddt = torch.full((K * B, MAX_SAMPLES), STAGE_GUARD, device=cuda)
    L.ml_march_count(*args, dcnt.data_ptr(), dts.data_ptr(), ddt.data_ptr(), _st(cuda))
    dense = (dcnt.cpu().numpy().reshape(K, B), dts, ddt)
    assert B < 64 or dense[0].sum() > 0
    g = gate_rows(B, K, seed=3 * B + K)
    rng = np.random.default_rng(B + K)
    for name, sel in (("top1", select_ref(g, gate_topk=1)),
                      ("top2", select_ref(g, gate_topk=min(2, K))),
                      ("tau", select_ref(g, gate_min=float(np.median(g))))):
        for order in ("ascending", "reversed", "shuffled"):
            lists = [{"ascending": l, "reversed": l[::-1],
                      "shuffled": rng.permutation(l)}[order] for l in sel["list"]]
            _check_listed((name, order), B, K, lists,
                          _list_march(cuda, L, args, B, K, lists), dense)
    every = np.arange(B, dtype=np.int32)
    hand = {"one list empty": [every if k != 1 else every[:0] for k in range(K)],
            "all rays to one": [every if k == K - 1 else every[:0] for k in range(K)],
            "nothing listed": [every[:0]] * K,
            # entries outside [0, B) are skipped, the rest of the list is marched
            "out of range": [np.concatenate([[-1, B, 2 ** 30], every[k % 2::2], [-(2 ** 31)]])
                             .astype(np.int32)[:B] for k in range(K)]}
    for name, lists in hand.items():
        _check_listed(name, B, K, lists, _list_march(cuda, L, args, B, K, lists), dense)


# ---- the chain ----------------------------------------------------------------------
def _setup(cuda, B, K, scale, uniform_gate=False):
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    with torch.no_grad():                               # this file's gate on the shared scene
        sc.g.params.copy_(torch.from_numpy(S.mlp_params(1, LY.gate_params(K), seed=GATE_SEED)[0]))
        if uniform_gate:
            sc.g.params[LY.gate_params(0):].zero_()     # the last layer: every logit 0
    return sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bits


def _bg(scale, cuda):
    return torch.ones(3, device=cuda) if scale <= 0.5 else torch.zeros(3, device=cuda)


@pytest.mark.parametrize("scale", [0.5, 16.0])
@pytest.mark.parametrize("K", [2, 4])
def test_all_live_routed_step_is_the_dense_step(cuda, K, scale):
    B = 384
    esf = 1 / 256 if scale > 0.5 else 0.0
    m, g, o, d, noise, seeds, _ = _setup(cuda, B, K, scale)
    o, d, nz = _t(o, cuda), _t(d, cuda), _t(noise, cuda)
    sd = [_t(s, cuda) for s in seeds]
    bg = _bg(scale, cuda)
    r = FusedMLRenderer(m, g, B, deterministic=True)
    r.input_grad = True
    w = r.ws

    def step(**route):
        out = r.forward(o, d, d, nz, bg, exp_step_factor=esf, distortion=True, **route)
        grads = r.backward(o, d, d, out[3], bg, *sd, dL_ddist=0.01)
        torch.cuda.synchronize()
        # the samples: each sub-NeRF's segment (the alignment gaps between them
        # are never written)
        n = torch.cat([torch.arange(b, b + c, device=cuda)
                       for b, c in zip(w.seg_base.tolist(), w.seg_count.tolist())])
        snap = dict(counts=w.counts, offsets=w.offsets, seg=w.seg, ts=w.ts[n], deltas=w.deltas[n],
                    ray_of=w.ray_of[n], rgb=out[0], opacity=out[1], depth=out[2], gate=out[3],
                    importance=out[4], dist=w.dist_k, grid=grads[0], mlp=grads[1], gate_grad=grads[2],
                    dgate=w.dgate, drays_o=w.drays_o, drays_d=w.drays_d, gate_dx=w.gate_dx)
        return {k: v.clone() for k, v in snap.items()}

    dense = step()
    assert r._routed is None and int(dense["counts"].sum()) > 0
    r._route_always = True
    routed = step(gate_topk=K, gate_min=0.0)
    assert r._routed == (K, 0.0, False)
    rt = w.route_buffers()
    assert bool(rt["live"].all()) and torch.equal(rt["gate_used"], dense["gate"])
    assert rt["count"].tolist() == [B] * K
    for k in dense:
        assert torch.equal(dense[k], routed[k]), k


def _conditions(live, K, B):
    """what a routed-vs-reference case needs to mean anything: every sub-NeRF
    owns at least 1/16 of the rays, at least a quarter of the pairs are dead"""
    assert (live.sum(0) >= B / 16).all(), live.sum(0)
    assert (live == 0).mean() >= 0.25


CASES = {"K2 top1": (2, 0.5, dict(gate_topk=1), False),
         "K4 top2 renorm": (4, 0.5, dict(gate_topk=2, renormalize=True), False),
         "K8 s16 median": (8, 16.0, "median", False),
         "K2 top1 dist+input": (2, 0.5, dict(gate_topk=1), True)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_routed_step_vs_reference(cuda, case):
    K, scale, route, extra = CASES[case]
    B = 384
    esf = 1 / 256 if scale > 0.5 else 0.0
    m, g, o, d, noise, seeds, bits = _setup(cuda, B, K, scale)
    to = lambda a: _t(a, cuda)
    if route == "median":
        with torch.no_grad():
            gate0 = ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise),
                                    exp_step_factor=esf)["gating_code"]
        route = dict(gate_min=float(np.median(gate0.cpu().numpy())))
    ot, dt = to(o).requires_grad_(extra), to(d).requires_grad_(extra)
    res = ml_render_fused(m, g, ot, dt, dt, noise=to(noise), exp_step_factor=esf,
                          distortion=extra, **route)
    w = get_renderer(m, g, B).ws
    outs, gs = [res["rgb"], res["opacity"], res["depth"]], [to(s) for s in seeds]
    g_dist = None
    if extra:
        # a seed of the other seeds' size: on the reference it moves the grid
        # gradient by ~2x its norm and the MLP's by ~0.4x, so neither share hides
        g_dist = (np.random.default_rng(5).normal(0, 1, (B, K)) * 4 / B).astype(np.float32)
        outs.append(res["distortion"])
        gs.append(to(g_dist))
    torch.autograd.backward(outs, gs)
    torch.cuda.synchronize()
    # the selection, restated on the GPU's own gate (its f16 MLP and the
    # oracle's fp32 one differ by ~1e-3: a near-tie could flip otherwise)
    gate = res["gating_code"].detach().cpu().numpy()
    sel = select_ref(gate, route.get("gate_min", 0.0), route.get("gate_topk"),
                     route.get("renormalize", False))
    live = sel["live"]
    _conditions(live, K, B)
    assert res["gating_live"].dtype == torch.bool
    assert np.array_equal(res["gating_live"].cpu().numpy(), live.astype(bool))
    assert np.array_equal(res["gating_used"].cpu().numpy(), sel["gate_used"])
    assert torch.equal(res["gating_importance"], res["gating_code"].sum(0))
    assert w.route_buffers()["count"].tolist() == sel["count"].tolist()
    ref = RR.routed_train_step(o, d, bits, noise,
                               m.xyz_encoder.params.detach().cpu().view(-1, 2),
                               m.mlp_params.detach().cpu(), g.params.detach().cpu(), scale,
                               live, renormalize=route.get("renormalize", False),
                               seeds=seeds, input_grads=extra, dist_seed=g_dist)
    # the march: counts and t / dt bit-exact for live pairs, nothing for dead ones
    cnt, off = w.counts.cpu().numpy(), w.offsets.cpu().numpy()
    assert np.array_equal(cnt, ref["counts"]) and not cnt[live.T == 0].any()
    assert cnt[live.T != 0].sum() > 0
    ts, dl = w.ts.cpu().numpy(), w.deltas.cpu().numpy()
    for k in range(K):
        n = int(cnt[k].sum())
        a = int(off[k, 0])
        assert np.array_equal(off[k] - a, ref["starts"][k])
        assert np.array_equal(ts[a:a + n].view(np.uint32), ref["ts"][k].view(np.uint32))
        assert np.array_equal(dl[a:a + n].view(np.uint32), ref["deltas"][k].view(np.uint32))
    err = {k: float(np.abs(res[k].detach().cpu().numpy() - ref[k]).max())
           for k in ("rgb", "opacity", "depth")}
    print(f"{case}: {int(cnt.sum())} samples, {float((live == 0).mean()):.2f} of the pairs dead; "
          f"Linf {err}")
    assert max(err.values()) <= 1e-4, err
    # a dead pair: depth 0, its own colour the background, dL/dgate exactly 0
    dead = torch.from_numpy(live == 0).to(cuda)
    assert not res["depth"].detach()[dead].any()
    for i in range(K):
        assert torch.equal(res["independent_rgbs"][i].detach()[dead[:, i]],
                           _bg(scale, cuda).expand(int(dead[:, i].sum()), 3))
    assert not w.dgate[dead].any() and bool(w.dgate[~dead].any())
    dg = w.dgate.cpu().numpy()
    e_dg = rel(dg, ref["dgate"])
    print(f"{case}: dgate rel {e_dg:.2e}")
    assert e_dg <= GATE_TOL                 # parity's bar for the gate's gradient
    check_grads(scale, m.xyz_encoder.params.grad.cpu().view(-1, 2).numpy(), ref["grid_grad"],
                m.mlp_params.grad.cpu().numpy(), ref["mlp_grad"],
                g.params.grad.cpu().numpy(), ref["gate_grad"], case)
    if extra:
        # the segment losses: the reference's, and -- the samples and sigmas of a
        # live pair being the dense chain's -- the dense chain's bit for bit; 0
        # for a dead pair
        dist = w.dist_k.clone()
        e_dist = np.abs(dist.t().cpu().numpy() - ref["distortion"]).max() \
            / np.abs(ref["distortion"]).max()
        eo = rel(ot.grad.cpu().numpy(), ref["drays_o"])
        ed = rel(dt.grad.cpu().numpy(), ref["drays_d"])
        print(f"{case}: distortion rel {e_dist:.2e}, drays_o rel {eo:.2e}, drays_d rel {ed:.2e}")
        assert e_dist <= 1e-4           # a per-ray output like rgb / opacity / depth: their bar
        assert eo <= 3e-3 and ed <= 3e-3        # test_input_grads_vs_oracle's
        with torch.no_grad():
            ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise), exp_step_factor=esf,
                            distortion=True)
        dense = get_renderer(m, g, B, grad=False).ws.dist_k
        lk = torch.from_numpy(live.T != 0).to(cuda)
        assert torch.equal(dist[lk], dense[lk]) and not dist[~lk].any()
        assert bool(dist[lk].any())


@pytest.mark.parametrize("K,scale,det", [(2, 0.5, False), (4, 16.0, False), (4, 0.5, True)])
def test_uniform_gate_routes_every_ray_to_the_first(cuda, K, scale, det):
    """The gate's last layer zeroed: every gate is exactly 1 / K, top-1 keeps
    index 0.  The plan, the merged forward and backward run with K - 1 empty
    sub-NeRFs.  (The deterministic case also renormalises: gate_used is 1.)"""
    B = 384
    esf = 1 / 256 if scale > 0.5 else 0.0
    m, g, o, d, noise, _, _ = _setup(cuda, B, K, scale, uniform_gate=True)
    o, d, nz = _t(o, cuda), _t(d, cuda), _t(noise, cuda)
    target = torch.rand(B, 3, device=cuda)
    r = FusedMLRenderer(m, g, B, deterministic=det)
    terms, (gg, mg, ag) = r.train_step(o, d, d, target, nz, _bg(scale, cuda), exp_step_factor=esf,
                                       lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3,
                                       gate_topk=1, renormalize=det)
    torch.cuda.synchronize()
    lf = r.last_forward
    assert torch.equal(lf["gate"], torch.full((B, K), 1.0 / K, device=cuda))
    assert lf["route_count"].tolist() == [B] + [0] * (K - 1)
    assert lf["route_count"].dtype == torch.int32 and lf["route_count"].is_cuda
    assert bool(lf["live"][:, 0].all()) and not lf["live"][:, 1:].any()
    assert torch.equal(lf["gate_used"][:, 0], torch.full((B,), 1.0 if det else 1.0 / K,
                                                         device=cuda))
    assert not lf["gate_used"][:, 1:].any()
    cnt = r.ws.counts
    assert int(cnt[0].sum()) > 0 and not cnt[1:].any()
    assert r.ws.seg_count.tolist()[1:] == [0] * (K - 1)
    assert not mg[1:].any() and bool(mg[0].any())
    for t in (gg, mg, ag, *terms.values()):
        assert bool(torch.isfinite(t).all())
    assert bool(gg.any())
    if det:     # one live pair per ray with weight 1: its depth is the row's mean
        assert float(terms["depth_mutual"]) == 0.0


def test_default_arguments_issue_no_routed_launch(cuda, monkeypatch):
    B, K, scale = 384, 2, 0.5
    m, g, o, d, noise, _, _ = _setup(cuda, B, K, scale)
    o, d, nz = _t(o, cuda), _t(d, cuda), _t(noise, cuda)
    target = torch.rand(B, 3, device=cuda)
    L = _lib.lib()

    def boom(*a, **k):
        raise AssertionError("a routed launch on the default path")
    for name in ("gate_select", "ml_march_count_list", "gate_select_bw", "nerf_loss_routed",
                 "nerf_loss_routed_det"):
        monkeypatch.setattr(L, name, boom)
    for kw in ({}, dict(gate_topk=None, gate_min=0.0, renormalize=False), dict(gate_topk=K)):
        r = FusedMLRenderer(m, g, B)
        terms, grads = r.train_step(o, d, d, target, nz, _bg(scale, cuda),
                                    lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3, **kw)
        torch.cuda.synchronize()
        assert sorted(terms) == ["cv_importance", "depth_mutual", "opacity", "rgb"]
        assert sorted(r.last_forward) == ["depth", "gate", "importance", "opacity", "rgb"]
        assert len(grads) == 3 and all(bool(torch.isfinite(x).all()) for x in grads)
    res = ml_render_fused(m, g, o, d, d, noise=nz)
    assert sorted(res) == ["depth", "gating_code", "gating_importance", "independent_rgbs",
                           "opacity", "rgb"]
    # and a routed step does go through them
    with pytest.raises(AssertionError, match="routed launch"):
        FusedMLRenderer(m, g, B).train_step(o, d, d, target, nz, _bg(scale, cuda), gate_topk=1)


# ---- rn_nerf_loss_routed / rn_nerf_loss_routed_det -------------------------------------
LAMBDAS = dict(lambda_opacity=1e-3, lambda_cv_importance=1e-2, lambda_depth_mutual=0.3)


@pytest.mark.parametrize("det,B", [(False, 200), (False, 1000), (True, 1000)])
@pytest.mark.parametrize("K", [2, 4, 9])
def test_routed_loss_vs_dense_entry_and_restatement(cuda, det, B, K):
    """The routed loss entries against the dense ones (every pair live: the same
    bits) and against route_ref.depth_mutual_ref under a selection."""
    from radnerf_amd.losses import fused_nerf_loss
    rng = np.random.default_rng(7 * B + K)
    g_np = gate_rows(B, K, seed=B + K)
    rgb, target = (_t(rng.random((B, 3), dtype=np.float32), cuda) for _ in range(2))
    opacity = _t(rng.random(B, dtype=np.float32), cuda)
    depth_np = (rng.random((B, K), dtype=np.float32) * 4).astype(np.float32)
    gate = _t(g_np, cuda)
    imp = gate.sum(0)
    loss = lambda dep, gt, live: fused_nerf_loss(rgb, target, opacity, dep, gt, imp,
                                                 deterministic=det, live=live, **LAMBDAS)
    # (a) every pair live, gate_used = gate: the dense entry's seeds bit for bit,
    # and its terms too where the sum has one order (one block, or the ordered form)
    dense_t, dense_s = loss(_t(depth_np, cuda), gate, None)
    all_t, all_s = loss(_t(depth_np, cuda), gate,
                        torch.ones(B, K, dtype=torch.uint8, device=cuda))
    assert sorted(all_t) == sorted(dense_t) == ["cv_importance", "depth_mutual", "opacity", "rgb"]
    for x, y in zip(all_s, dense_s):
        assert torch.equal(x, y)
    for k in dense_t:
        if det or B <= 256:
            assert torch.equal(all_t[k], dense_t[k]), k
        else:       # one fp32 atomic per block, in arrival order
            assert abs(float(all_t[k]) - float(dense_t[k])) <= 1e-6 * abs(float(dense_t[k])), k
    # (b) a selection: dead pairs have depth 0 and weight 0
    for sel in (select_ref(g_np, gate_topk=1), select_ref(g_np, gate_topk=max(1, K // 2)),
                select_ref(g_np, gate_min=float(np.median(g_np)))):
        lv = sel["live"].astype(bool)
        assert (~lv).any()
        dep = np.where(lv, depth_np, np.float32(0))
        terms, (d_rgb, d_op, d_depth, d_gate) = loss(_t(dep, cuda), _t(sel["gate_used"], cuda),
                                                     _t(sel["live"], cuda))
        want_t, want_seed = RR.depth_mutual_ref(dep, sel["gate_used"], lv, LAMBDAS["lambda_depth_mutual"])
        got = d_depth.cpu().numpy()
        assert np.array_equal(got, want_seed)
        assert not got[~lv].any() and got[lv].any()
        # the term: B K non-negative fp32 numbers summed in fp32 in some order,
        # |error| <= (n - 1) 2^-24 sum|terms|, and one division
        total = want_t.astype(np.float64).sum()
        n = B * K
        assert abs(float(terms["depth_mutual"]) * n - total) <= n * 2.0 ** -24 * total
        assert total > 0
        # routing touches the depth-mutual part alone
        for x, y in ((d_rgb, dense_s[0]), (d_op, dense_s[1]), (d_gate, dense_s[3])):
            assert torch.equal(x, y)
        if det or B <= 256:
            for k in ("rgb", "opacity", "cv_importance"):
                assert torch.equal(terms[k], dense_t[k]), k


# ---- Trainer --------------------------------------------------------------------------
ROUTE = dict(gate_topk=1, route_from_step=3)


def test_routed_trainer_is_reproducible_and_resumable(cuda):
    K, scale, steps, cut = 2, 0.5, 12, 6
    a = RES.trainer(cuda, K, scale, False, img_wh=RES.WH, **ROUTE)
    b = RES.trainer(cuda, K, scale, False, img_wh=RES.WH, **ROUTE)
    assert a.routing == {"gate_topk": 1, "gate_min": 0.0, "renormalize": False}
    RES.run_steps(a, 2)
    assert "live" not in a.renderer.last_forward            # dense before route_from_step
    RES.run_steps(a, steps)
    lf = a.renderer.last_forward
    assert int(lf["route_count"].sum()) == RES.N_RAYS and int(lf["live"].sum()) == RES.N_RAYS
    RES.run_steps(b, cut)
    sd = b.state_dict()
    assert sd["hyper"]["gate_topk"] == 1 and sd["hyper"]["route_from_step"] == 3
    RES.run_steps(b, steps)
    end = RES.full_state(a)
    RES.assert_same_tensors(end, RES.full_state(b))         # two runs, the same bits
    c = RES.other_trainer(cuda, K, scale, False, img_wh=RES.WH, **ROUTE)
    c.load_state_dict(sd)
    RES.run_steps(c, steps)
    RES.assert_same_tensors(end, RES.full_state(c))         # saved at 6, resumed
    dirs, poses, u8 = RES.dataset(cuda)
    images = (u8[:2].float() / 255).contiguous()
    routed = a.validate(poses[:2], images, **a.routing)
    dense = a.validate(poses[:2], images)
    for v in (routed, dense):
        assert bool(torch.isfinite(v["psnr"])) and float(v["psnr"]) > 0
    print(f"12 steps, top-1 from step 3: psnr routed {float(routed['psnr']):.2f}, "
          f"dense {float(dense['psnr']):.2f}")
