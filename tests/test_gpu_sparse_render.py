"""GPU: the gate-sparse test-time render.

  (a) rn_gate_select against its numpy restatement (tests/gate_select_ref.py),
      bit for bit: live, gate_used, count, the lists (ascending, tails
      untouched), zeros in the dead output slots only, guard words intact;
  (b) rn_render_test_list against rn_render_test on hand-made lists: a listed
      pair has the dense kernel's bits, in any list order; nothing else is
      written (a sub-NeRF with count 0 included);
  (c) ImageEvaluator.render_image(gate_min / gate_topk / renormalize) on the
      24 x 20 image of tests/test_gpu_evaluate.py: equal to rn_ml_combine_test
      on the dense per-pair outputs with the restatement's gate_used, within
      the dead gate mass of the dense image, independent of the chunk; the
      dense-equivalent arguments return the dense dict;
  (d) Trainer.validate with the keywords.
"""
import numpy as np
import pytest
import torch

import gate_select_ref as GR
from radnerf_amd import _lib, metrics, sparse_gate
from radnerf_amd.evaluate import ImageEvaluator
from radnerf_amd.trainer import Trainer
from test_gpu_evaluate import CHUNK, WH, _setup

pytestmark = pytest.mark.gpu

GUARD = 16


class Guarded:
    """A device buffer of n elements between two runs of GUARD guard elements."""

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


# ---- (a) rn_gate_select ---------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 8, 9, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_gate_select_vs_restatement(cuda, n, K):
    L = _lib.lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    g_np = GR.gate_rows(n, K, seed=100 * K + n)
    gate = _t(g_np, cuda)
    inside = g_np[(g_np > 0) & (g_np < 1)]
    present = float(np.sort(inside)[len(inside) // 2]) if len(inside) else 0.25
    SENT = 7.5
    for tau in (0.0, present, 0.5, 0.999):
        for k in (None, 1, 2, K):
            for renorm in (False, True):
                ref = GR.select_ref(g_np, tau, k, renorm)
                tag = (n, K, tau, k, renorm)
                live = Guarded(n * K, torch.uint8, 0xAB, cuda)
                used = Guarded(n * K, torch.float32, -3.0, cuda)
                lst = Guarded(K * n, torch.int32, -1, cuda)
                cnt = Guarded(K, torch.int32, -5, cuda)
                op, de = (Guarded(K * n, torch.float32, SENT, cuda) for _ in range(2))
                rgb = Guarded(K * n * 3, torch.float32, SENT, cuda)
                ns = Guarded(K * n, torch.int32, 77, cuda)
                work = Guarded(_lib.GATE_SELECT_WORK_BYTES, torch.uint8, 0xFF, cuda)
                L.gate_select(gate.data_ptr(), n, K, tau, K if k is None else k, int(renorm),
                              live.t.data_ptr(), used.t.data_ptr(), lst.t.data_ptr(),
                              cnt.t.data_ptr(), op.t.data_ptr(), de.t.data_ptr(),
                              rgb.t.data_ptr(), ns.t.data_ptr(), work.t.data_ptr(), st)
                for b in (live, used, lst, cnt, op, de, rgb, ns, work):
                    assert b.intact(), tag
                assert torch.equal(live.t.view(n, K).cpu(), torch.from_numpy(ref["live"])), tag
                # bit for bit: the int32 view also tells -0 from 0
                assert torch.equal(used.t.view(n, K).cpu().view(torch.int32),
                                   torch.from_numpy(ref["gate_used"]).view(torch.int32)), tag
                assert torch.equal(cnt.t.cpu(), torch.from_numpy(ref["count"])), tag
                lists = lst.t.view(K, n).cpu().numpy()
                for i in range(K):
                    c = int(ref["count"][i])
                    assert np.array_equal(lists[i, :c], ref["list"][i]), (tag, i)
                    assert (np.diff(lists[i, :c]) > 0).all(), (tag, i)
                    assert (lists[i, c:] == -1).all(), (tag, i)
                # the per-pair outputs ([K][n]): dead -> 0, live untouched
                dead = torch.from_numpy(ref["live"].T == 0)
                want_f = torch.where(dead, 0.0, SENT)
                assert torch.equal(op.t.view(K, n).cpu(), want_f), tag
                assert torch.equal(de.t.view(K, n).cpu(), want_f), tag
                assert torch.equal(rgb.t.view(K, n, 3).cpu(),
                                   want_f[:, :, None].expand(K, n, 3)), tag
                assert torch.equal(ns.t.view(K, n).cpu(),
                                   torch.where(dead, 0, 77).to(torch.int32)), tag


def test_select_module_and_large_chunk(cuda):
    """sparse_gate.select (no per-pair outputs) on more rays than 1024 blocks of
    256 cover in one step each: a block then owns several steps."""
    n, K = 256 * 1024 + 300, 3
    g_np = GR.softmax_rows(n, K, seed=4)
    ref = GR.select_ref(g_np, 0.2, 2, True)
    sel = sparse_gate.select(_t(g_np, cuda), gate_min=0.2, gate_topk=2, renormalize=True)
    assert set(sel) == {"live", "gate_used", "list", "count"}
    assert torch.equal(sel["live"].cpu(), torch.from_numpy(ref["live"]))
    assert torch.equal(sel["gate_used"].cpu().view(torch.int32),
                       torch.from_numpy(ref["gate_used"]).view(torch.int32))
    assert torch.equal(sel["count"].cpu(), torch.from_numpy(ref["count"]))
    for i in range(K):
        c = int(ref["count"][i])
        assert np.array_equal(sel["list"][i, :c].cpu().numpy(), ref["list"][i]), i
    # into the caller's buffers: the same, and the same objects
    again = sparse_gate.select(_t(g_np, cuda), 0.2, 2, True, out=dict(sel))
    assert all(again[k] is sel[k] for k in sel)
    assert torch.equal(again["count"].cpu(), torch.from_numpy(ref["count"]))
    with pytest.raises(ValueError, match=r"out\['list'\]"):
        sparse_gate.select(_t(g_np, cuda), out={**sel, "list": sel["list"][:, :-1]})


# ---- (b) rn_render_test_list ------------------------------------------------------
def _render_args(ev, n, T_threshold=1e-4, max_samples=1024):
    """ImageEvaluator.render_image's rn_render_test arguments up to the outputs,
    on the rays its last chunk left in its buffers"""
    m = ev.model
    bits, nb = ev._bitfields()
    lo, lh, lr, ls = m.xyz_encoder.level_ptrs()
    keep = (m.xyz_encoder.params_f16(), m.packed_frags(), bits)
    return (ev.rays_o.data_ptr(), ev.rays_d.data_ptr(), ev.hits_t.data_ptr(), n, m.size,
            bits.data_ptr(), nb, m.cascades, float(m.scale), ev.esf, m.grid_size, max_samples,
            keep[0].data_ptr(), lo, lh, lr, ls, m._h_min.ctypes.data, m._h_ext.ctypes.data,
            keep[1].data_ptr(), T_threshold), keep


@pytest.mark.parametrize("scale", [0.5, 16.0])
@pytest.mark.parametrize("K", [2, 3, 9])
def test_render_list_vs_dense(cuda, K, scale):
    L = _lib.lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    m, g, dirs, poses = _setup(cuda, K, "ray", scale)
    n = dirs.shape[0]
    assert n == 480
    ev = ImageEvaluator(m, g, dirs, WH, chunk=n)
    ev.render_image(poses[1])                 # fills rays_o / rays_d / hits_t of the one chunk
    args, keep = _render_args(ev, n)
    blocks = max(1, min((n + 3) // 4, 512 // K))
    SENT = -9.25

    def buffers():
        return (Guarded(K * n, torch.float32, SENT, cuda), Guarded(K * n, torch.float32, SENT, cuda),
                Guarded(K * n * 3, torch.float32, SENT, cuda), Guarded(K * n, torch.int32, -9, cuda))

    dense = buffers()
    L.render_test(*args, *(b.t.data_ptr() for b in dense), blocks, st)
    d_op, d_de, d_rgb, d_ns = (b.t.clone() for b in dense)
    assert int(d_ns.sum()) > 0 and bool((d_ns >= 0).all()) and bool((d_op != SENT).all())
    # the evaluator's own dense launch wrote the same per-pair values
    assert torch.equal(d_op, ev.op_k) and torch.equal(d_ns, ev.n_smp)
    # a hand-made selection: about half the pairs, sub-NeRF 1 none at all
    rng = np.random.default_rng(17 * K)
    live = rng.random((K, n)) < 0.5
    live[1] = False
    live[0, :5] = True
    live_t = torch.from_numpy(live).to(cuda)
    count = torch.from_numpy(live.sum(1).astype(np.int32)).to(cuda)
    results = []
    for order in ("ascending", "reversed", "shuffled"):
        lst = Guarded(K * n, torch.int32, -1, cuda)
        for i in range(K):
            rays = np.nonzero(live[i])[0].astype(np.int32)
            rays = {"ascending": rays, "reversed": rays[::-1],
                    "shuffled": rng.permutation(rays)}[order]
            lst.t.view(K, n)[i, :len(rays)] = _t(rays, cuda)
        out = buffers()
        L.render_test_list(*args, *(b.t.data_ptr() for b in out), lst.t.data_ptr(),
                           count.data_ptr(), blocks, st)
        op, de, rgb, ns = (b.t for b in out)
        assert all(b.intact() for b in out) and lst.intact(), order
        # listed pairs: the dense kernel's bits; the rest (all of sub-NeRF 1): not written
        assert torch.equal(op.view(K, n), torch.where(live_t, d_op.view(K, n), SENT)), order
        assert torch.equal(de.view(K, n), torch.where(live_t, d_de.view(K, n), SENT)), order
        assert torch.equal(rgb.view(K, n, 3), torch.where(live_t[:, :, None], d_rgb.view(K, n, 3),
                                                          SENT)), order
        assert torch.equal(ns.view(K, n), torch.where(live_t, d_ns.view(K, n), -9)), order
        assert bool((op.view(K, n)[1] == SENT).all()) and bool((ns.view(K, n)[1] == -9).all())
        results.append(torch.cat([op, de, rgb]))
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    # every pair listed: the dense outputs whole
    full = Guarded(K * n, torch.int32, -1, cuda)
    full.t.view(K, n)[:] = torch.arange(n, dtype=torch.int32, device=cuda)
    out = buffers()
    L.render_test_list(*args, *(b.t.data_ptr() for b in out), full.t.data_ptr(),
                       torch.full((K,), n, dtype=torch.int32, device=cuda).data_ptr(), blocks, st)
    for got, want in zip(out, (d_op, d_de, d_rgb, d_ns)):
        assert torch.equal(got.t, want) and got.intact()
    del keep


# ---- (c) ImageEvaluator -------------------------------------------------------------
def _sparse_case(cuda, K, scale, kw_of):
    """dense render (one chunk of 480, so its per-pair buffers hold the whole
    image), then kw_of(gate) -> the sparse keywords; the restatement and the
    expected image from rn_ml_combine_test on the dense per-pair outputs"""
    L = _lib.lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    m, g, dirs, poses = _setup(cuda, K, "ray", scale)
    N = dirs.shape[0]
    pose = poses[1]
    ev1 = ImageEvaluator(m, g, dirs, WH, chunk=N)
    dense = {k: v.clone() for k, v in ev1.render_image(pose).items()}
    pairs = {"op": ev1.op_k.clone(), "de": ev1.depth_k.clone(), "rgb": ev1.rgb_k.clone(),
             "ns": ev1.n_smp.clone()}
    gate = dense["gating_code"]
    kw = kw_of(gate)
    ref = GR.select_ref(gate.cpu().numpy(), kw.get("gate_min", 0.0), kw.get("gate_topk"),
                        kw.get("renormalize", False))
    used = _t(ref["gate_used"], cuda)
    f32 = dict(device=cuda, dtype=torch.float32)
    want = {"rgb": torch.empty(N, 3, **f32), "opacity": torch.empty(N, **f32),
            "depth": torch.empty(N, **f32)}
    L.ml_combine_test(used.data_ptr(), pairs["op"].data_ptr(), pairs["de"].data_ptr(),
                      pairs["rgb"].data_ptr(), ev1.bg.data_ptr(), N, K, 0, want["rgb"].data_ptr(),
                      want["opacity"].data_ptr(), want["depth"].data_ptr(), None, st)
    live = _t(ref["live"], cuda)
    want["depth_k"] = torch.where(live != 0, dense["depth_k"], 0.0)
    want["total_samples"] = (pairs["ns"].view(K, N).t() * live).sum()
    return m, g, dirs, pose, dense, ref, used, live, want, kw


CASES = [
    # (K, scale, keywords from the image's gate, dead share bounds)
    ("median", 2, 0.5, lambda gate: {"gate_min": float(gate.flatten().median())}, (0.25, 0.75)),
    ("median-renorm", 2, 0.5, lambda gate: {"gate_min": float(gate.flatten().median()),
                                           "renormalize": True}, (0.25, 0.75)),
    ("top1", 3, 16.0, lambda gate: {"gate_topk": 1}, (0.66, 0.67)),
    ("top1-renorm", 3, 16.0, lambda gate: {"gate_topk": 1, "renormalize": True}, (0.66, 0.67)),
]


@pytest.mark.parametrize("name,K,scale,kw_of,dead_share", CASES, ids=[c[0] for c in CASES])
def test_render_image_sparse(cuda, name, K, scale, kw_of, dead_share):
    m, g, dirs, pose, dense, ref, used, live, want, kw = _sparse_case(cuda, K, scale, kw_of)
    N = dirs.shape[0]
    share = 1.0 - float(ref["live"].mean())
    print(f"sparse render_image {name}: K {K} scale {scale} {kw}, dead share {share:.3f}")
    assert dead_share[0] <= share <= dead_share[1]
    ev = ImageEvaluator(m, g, dirs, WH, chunk=CHUNK)
    assert N == 3 * CHUNK + 96 and ev.sparse is None
    res = {k: v.clone() for k, v in ev.render_image(pose, **kw).items()}
    assert set(res) == set(dense) | {"gating_live", "gating_used", "pairs"}
    assert res["gating_live"].dtype == torch.uint8 and res["gating_live"].shape == (N, K)
    assert res["pairs"].dtype == torch.int64 and res["pairs"].device.type == "cuda"
    assert torch.equal(res["gating_live"], live)
    assert torch.equal(res["gating_used"].view(torch.int32), used.view(torch.int32))
    assert int(res["pairs"]) == int(live.sum()) == int(ref["count"].sum())
    # the full softmax stays, so the gate pictures do not change
    assert torch.equal(res["gating_code"], dense["gating_code"])
    for k in ("rgb", "opacity", "depth", "depth_k"):
        assert torch.equal(res[k], want[k]), k
    assert int(res["total_samples"]) == int(want["total_samples"]) < int(dense["total_samples"])
    # the workspaces are made once
    bufs = {k: v.data_ptr() for k, v in ev.sparse.items()}
    ev.render_image(pose, **kw)
    assert bufs == {k: v.data_ptr() for k, v in ev.sparse.items()}
    # within the dead gate mass of the dense image (not renormalised)
    if not kw.get("renormalize"):
        mass = torch.where(live == 0, dense["gating_code"], 0.0).double().sum(1)
        bound = mass * (1 + 2.0 ** -20) + K * 2.0 ** -23
        d_rgb = (res["rgb"].double() - dense["rgb"].double()).abs().amax(1)
        d_op = (res["opacity"].double() - dense["opacity"].double()).abs()
        print(f"  max |d rgb| {float(d_rgb.max()):.3e}, |d opacity| {float(d_op.max()):.3e}, "
              f"largest dead mass {float(mass.max()):.3e}")
        assert bool((d_rgb <= bound).all()) and bool((d_op <= bound).all())
        assert float(d_rgb.max()) > 0            # something was dropped
    # independent of the chunk: one chunk of 480 against four, bitwise
    one = ImageEvaluator(m, g, dirs, WH, chunk=N).render_image(pose, **kw)
    for k, v in res.items():
        assert torch.equal(v, one[k]), k


def test_dense_arguments_run_the_dense_launches(cuda, monkeypatch):
    K = 3
    m, g, dirs, poses = _setup(cuda, K, "ray", 0.5)
    ev = ImageEvaluator(m, g, dirs, WH, chunk=CHUNK)
    dense = {k: v.clone() for k, v in ev.render_image(poses[0]).items()}

    def boom(*a, **k):
        raise AssertionError("a dense-equivalent render reached the selection")
    L = _lib.lib()
    monkeypatch.setattr(L, "gate_select", boom)
    monkeypatch.setattr(L, "render_test_list", boom)
    monkeypatch.setattr(sparse_gate, "select", boom)
    for kw in ({"gate_min": 0.0}, {"gate_topk": K}, {"gate_min": 0, "gate_topk": None},
               {"gate_topk": K, "renormalize": True}):
        res = ev.render_image(poses[0], **kw)
        assert set(res) == set(dense), kw
        for k, v in dense.items():
            assert torch.equal(res[k], v), (kw, k)
    assert ev.sparse is None
    # a single NGP (no gate): dense whatever the keywords
    m1, _, dirs1, poses1 = _setup(cuda, 1, None, 0.5)
    ev1 = ImageEvaluator(m1, None, dirs1, WH, chunk=CHUNK)
    d1 = {k: v.clone() for k, v in ev1.render_image(poses1[0]).items()}
    r1 = ev1.render_image(poses1[0], gate_min=0.5, gate_topk=1, renormalize=True)
    assert set(r1) == set(d1) and all(torch.equal(r1[k], d1[k]) for k in d1)


# ---- (d) Trainer.validate -----------------------------------------------------------
def test_trainer_validate_sparse(cuda):
    m, g, dirs, poses = _setup(cuda, 2, "ray", 0.5)
    tr = Trainer(m, g, 256, directions=dirs, poses=poses, img_wh=WH)
    gt = torch.rand(2, dirs.shape[0], 3, generator=torch.Generator().manual_seed(4)).to(cuda)
    state = lambda: [t.detach().clone() for t in
                     [m.xyz_encoder.params, m.mlp_params, g.params]
                     + [getattr(m, f"density_{k}_{i}") for k in ("grid", "bitfield")
                        for i in range(2)]]
    before, step = state(), tr.global_step
    kw = dict(gate_topk=1, renormalize=True)
    val = tr.validate(poses, gt, **kw)
    assert tr.global_step == step
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    ev = ImageEvaluator(m, g, dirs, WH, exp_step_factor=tr.esf)
    for i in range(2):
        res = ev.render_image(poses[i], **kw)
        assert int(res["pairs"]) == dirs.shape[0]            # one sub-NeRF per ray
        assert torch.equal(metrics.psnr(res["rgb"], gt[i]), val["per_image"][i]["psnr"])
        assert torch.equal(ev.evaluate(poses[i], gt[i], **kw)["ssim"], val["per_image"][i]["ssim"])
    # and it is not the dense validation
    dense = tr.validate(poses, gt)
    assert not torch.equal(dense["psnr"], val["psnr"])
