"""GPU: the 9..16 sub-NeRF range.

The product accepts up to 16 sub-NeRFs, and above 8 the code runs differently:
the gate's logit rows 8..15 live in accumulator registers 4..7 (gate.hip), the
renderer falls back to the per-model field kernels (fused.py: merged_bwd,
merged_fwd and level_fwd are off, fwd_blocks = 2048 // K, bwd_blocks = 256 //
K, no plan), and rn_scan_segments switches kernels at 3 and 17 segments.  Every
test here compares a kernel with a plain restatement of the same operation
(numpy int64, torch fp32 / fp64 autograd, the CPU oracle) at K on both sides
of 8, with K <= 8 rows as controls of the same body and bars.
"""
import numpy as np
import pytest
import torch

from oracle import field_oracle as fo
from oracle import ml_oracle
from oracle.ml_oracle import _split_gate
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from radnerf_amd.fused import get_renderer, ml_render_fused
from radnerf_amd.networks import Ray_Gate
from radnerf_amd.rendering import ml_render as _ml_render
from parity import GATE_TOL, check_grads, rel

pytestmark = pytest.mark.gpu

GUARD = -7.0


def _st(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


# --------------------------------------------------------------------- 1. scan
def _scan_ref(counts, align):
    """march.hip's header comment in int64: exclusive scan inside each
    segment, segment k at align_up(seg_base[k-1] + seg_count[k-1]), meta =
    (aligned end, unaligned total)."""
    counts = counts.astype(np.int64)
    offsets = np.zeros_like(counts)
    seg_base, seg_count = [], []
    base = 0
    for k in range(counts.shape[0]):
        offsets[k] = base + np.cumsum(counts[k]) - counts[k]
        seg_base.append(base)
        seg_count.append(int(counts[k].sum()))
        base = -(-(base + seg_count[-1]) // align) * align
    return offsets, np.array(seg_base), np.array(seg_count), np.array([base, counts.sum()])


def _scan_counts(n_seg, n_per, seed):
    """uniform in [0, 300], a tenth of them zero, one segment all zero (with
    one segment only: kept, and the all-zero segment is a case of its own)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 301, (n_seg, n_per))
    c[rng.random((n_seg, n_per)) < 0.1] = 0
    if n_seg > 1:
        c[n_seg // 2] = 0
    return c.astype(np.int32)


@pytest.mark.parametrize("n_seg", [1, 2, 3, 8, 9, 15, 16, 17])
def test_scan_segments_exact(cuda, n_seg):
    """rn_scan_segments on both of its kernels (one block per segment for 3..16
    segments, the single block for 1, 2 and >= 17) and both sides of each
    switch: offsets, seg_base, seg_count and meta equal the int64 restatement,
    and nothing is written past any output.  n_per covers one element, a
    partial wave, exactly one 4096-element pass, one more, and a ragged second
    pass; (9, 4097, 256), (16, 5000, 32) and (17, 4097, 32) are among them."""
    st = _st(cuda)
    cases = [(n_per, align) for n_per in (1, 63, 4096, 4097, 5000) for align in (1, 32, 256)]
    for n_per, align in cases:
        counts = _scan_counts(n_seg, n_per, 1000 * n_seg + n_per)
        variants = [counts]
        if n_seg == 1 and n_per == 4097:
            variants.append(np.zeros_like(counts))
        for cnt in variants:
            want = _scan_ref(cnt, align)
            assert want[3][0] < 2 ** 31
            c = torch.from_numpy(cnt).to(cuda)
            i32 = dict(device=cuda, dtype=torch.int32)
            off = torch.full((n_seg * n_per + 64,), -7, **i32)
            sb, sc = torch.full((n_seg + 8,), -7, **i32), torch.full((n_seg + 8,), -7, **i32)
            meta = torch.full((2 + 8,), -7, **i32)
            lib().scan_segments(c.data_ptr(), n_seg, n_per, align, off.data_ptr(), sb.data_ptr(),
                                sc.data_ptr(), meta.data_ptr(), st)
            tag = (n_seg, n_per, align)
            got = [t.cpu().numpy().astype(np.int64) for t in (off, sb, sc, meta)]
            assert np.array_equal(got[0][:n_seg * n_per].reshape(n_seg, n_per), want[0]), tag
            assert np.array_equal(got[1][:n_seg], want[1]), tag
            assert np.array_equal(got[2][:n_seg], want[2]), tag
            assert np.array_equal(got[3][:2], want[3]), tag
            for g, n in zip(got, (n_seg * n_per, n_seg, n_seg, 2)):
                assert np.all(g[n:] == -7), tag
            assert np.array_equal(c.cpu().numpy(), cnt), tag


# --------------------------------------------------------------------- 2. gate
GATE_OFFS = {"w0": (0, 384), "w1": (384, 4480), "w2": (4480, 8576), "w3": (8576, 12672)}
GATE_INPUT_TOL = 1.5e-3     # test_gpu_field.py test_gate_input_grad's bar


def _gate(cuda, K, gate_type="ray"):
    g = Ray_Gate(K, type=gate_type, seed=2)
    with torch.no_grad():
        g.params.copy_(torch.from_numpy(S.mlp_params(1, LY.gate_params(K), seed=6, scale=0.3)[0]))
    return g.to(cuda)


def _gate_direct(cuda, g, in0, in1, dg, want_dx):
    """rn_gate_fwd / rn_gate_bwd through the library on (n, 3) + (n, 3)
    inputs of row stride 3, every output with a guard row after the last ray
    (NaN) / guard elements after the last parameter: returns gate, importance,
    dw, dx (or None) on the host and asserts the guards untouched."""
    K, n = g.out_dim, in0.shape[0]
    st = _st(cuda)
    nan = float("nan")
    frags = g.packed_frags()
    gate = torch.full((n + 1, K), nan, device=cuda)
    imp = torch.zeros(K + 16, device=cuda)
    imp[K:] = GUARD
    nb = max(1, min(256, (n + 127) // 128))
    lib().gate_fwd(in0.data_ptr(), in1.data_ptr(), 3, n, K, frags.data_ptr(), gate.data_ptr(),
                   imp.data_ptr(), nb, st)
    assert bool(torch.isnan(gate[n]).all()), "gate: the row after the last ray was written"
    assert not bool(torch.isnan(gate[:n]).any())
    assert bool((imp[K:] == GUARD).all()), "importance: a row >= K was written"
    n_params = LY.gate_params(K)
    assert n_params == 12672 + 64 * K == g.params.numel()
    dgate = torch.full((n + 1, K), nan, device=cuda)
    dgate[:n] = dg
    dw = torch.zeros(n_params + 64 * (17 - K), device=cuda)
    dw[n_params:] = GUARD
    dx = None
    dfr = None
    if want_dx:
        dx = torch.full((n + 1, 6), nan, device=cuda)
        dfr = g.packed_dinput_frags()
    lib().gate_bwd(in0.data_ptr(), in1.data_ptr(), 3, n, K, frags.data_ptr(), dgate.data_ptr(),
                   dw.data_ptr(), n_params, None if dfr is None else dfr.data_ptr(),
                   None if dx is None else dx.data_ptr(), max(1, min(128, (n + 127) // 128)), st)
    assert bool((dw[n_params:] == GUARD).all()), "dw: a W4 row >= K was written"
    assert bool(torch.isfinite(dw[:n_params]).all()), "dw: the NaN guard row of dgate was read"
    if dx is not None:
        assert bool(torch.isnan(dx[n]).all()) and bool(torch.isfinite(dx[:n]).all())
        dx = dx[:n].cpu().numpy()
    return gate[:n].cpu(), imp[:K].cpu(), dw[:n_params].cpu().numpy(), dx


def _gate_layer_errors(K, got, ref):
    """relative L2 per layer w0..w3, and per output row of w4 (offsets as in
    ml_oracle._split_gate): {name: error}; an all-zero reference (K = 1: the
    softmax over one logit has no gradient) must be matched exactly"""
    parts = dict(GATE_OFFS)
    for r in range(K):
        parts[f"w4[{r}]"] = (12672 + 64 * r, 12672 + 64 * (r + 1))
    errs = {}
    for name, (a, b) in parts.items():
        if np.abs(ref[a:b]).max() == 0:
            assert np.abs(got[a:b]).max() == 0, name
            errs[name] = 0.0
        else:
            errs[name] = rel(got[a:b], ref[a:b])
    return errs


def _gate_case(cuda, K, n, gate_type="ray", want_dx=False):
    g = _gate(cuda, K, gate_type)
    o, d = S.rays(n)
    second = S.rays(n, seed=77)[1] if gate_type == "image" else d
    x = np.concatenate([o, second], 1)
    dg = np.random.default_rng(100 * K + n).normal(0, 1, (n, K)).astype(np.float32)
    in0, in1 = torch.from_numpy(o).to(cuda), torch.from_numpy(second).to(cuda)
    gate, imp, dw, dx = _gate_direct(cuda, g, in0, in1, torch.from_numpy(dg).to(cuda), want_dx)
    gp = g.params.detach().cpu().clone().requires_grad_(True)
    xo = torch.from_numpy(x).requires_grad_(True)
    ogate = fo.gate_forward(xo, _split_gate(gp, K))
    ogate.backward(torch.from_numpy(dg))
    out = {"gate": float((gate - ogate.detach()).abs().max()),
           "rowsum": float((gate.double().sum(1) - 1).abs().max()),
           "imp": float((imp.double() - gate.double().sum(0)).abs().max()),
           "layers": _gate_layer_errors(K, dw, gp.grad.numpy()),
           "dx": None if dx is None else rel(dx, xo.grad.numpy())}
    lay = out["layers"]
    w4 = [v for k_, v in lay.items() if k_.startswith("w4")]
    print(f"gate K={K} n={n} {gate_type}: L_inf {out['gate']:.2e} rowsum {out['rowsum']:.2e} "
          f"imp {out['imp']:.2e} | " + " ".join(f"{k_} {lay[k_]:.2e}" for k_ in GATE_OFFS)
          + f" w4 rows max {max(w4):.2e} (row {int(np.argmax(w4))})"
          + ("" if dx is None else f" | dx {out['dx']:.2e}"))
    return out


def _gate_check(K, n, out):
    # test_gate_forward_backward's bar; measured <= 1.8e-7, row sums <= 1.6e-7
    assert out["gate"] <= 1e-5, (K, n, out["gate"])
    assert out["rowsum"] <= 1e-5, (K, n, out["rowsum"])
    # the kernel's importance is the fp32 sum (per-wave tree, then atomics) of
    # the gate it stored: against the fp64 column sum of that gate
    assert out["imp"] <= 1e-6 * n, (K, n, out["imp"])             # measured <= 5.9e-8 n
    # measured, K = 8 / 9 / 12 / 16: w0..w3 <= 6.1e-4 / 6.9e-4 / 5.6e-4 / 5.4e-4,
    # worst W4 row 1.17e-3 / 1.33e-3 / 1.19e-3 / 1.37e-3: every layer and row is
    # inside parity.GATE_TOL on both sides of 8, so no bar of its own is needed
    bad = {k_: v for k_, v in out["layers"].items() if v > GATE_TOL}
    assert not bad, (K, n, bad)
    if out["dx"] is not None:
        assert out["dx"] <= GATE_INPUT_TOL, (K, n, out["dx"])     # measured <= 6.7e-4


# 8: the control (rows 0..7 only: accumulator registers 0..3, the range the
# suite covered before); 9, 12, 16 use registers 4..7
@pytest.mark.parametrize("K", [1, 3, 8, 9, 12, 16])
def test_gate_rows_per_layer(cuda, K):
    """rn_gate_fwd / rn_gate_bwd against fo.gate_forward with autograd, at one
    ray, one ray short of a tile, a tile, one more, and three tiles + 4: gate
    and row sums (1e-5), the returned importance, the parameter gradient per
    layer w0..w3 and per W4 row (parity.GATE_TOL each: a wrong row >= 8 moves
    64 of 13000+ parameters, which a whole-tensor norm need not notice), the
    input gradient at K = 9 and 16, and guards after the last ray / parameter.
    Measured on MI355X: see DESIGN.md §2 (gate, per layer)."""
    for n in (1, 31, 32, 33, 100):
        _gate_check(K, n, _gate_case(cuda, K, n, want_dx=K in (9, 16)))


def test_gate_image_type_split_inputs(cuda):
    """gate type "image" at K = 9: the gate reads cat(rays_o, imgs_d) from two
    separate (n, 3) tensors (in0 / in1), forward, parameter and input
    gradients."""
    _gate_check(9, 100, _gate_case(cuda, 9, 100, gate_type="image", want_dx=True))


def test_gate_module_many_rows(cuda):
    """Ray_Gate.forward (the (n, 6) tensor as in0 / in1 at stride 6, several
    blocks) at K = 16 with the existing whole-tensor bars of
    test_gate_forward_backward, plus the per-layer ones."""
    K, n = 16, 3000
    g = _gate(cuda, K)
    o, d = S.rays(n)
    x = np.concatenate([o, d], 1)
    gate, imp, _ = g(torch.from_numpy(x).to(cuda))
    gp = g.params.detach().cpu().clone().requires_grad_(True)
    ogate = fo.gate_forward(torch.from_numpy(x), _split_gate(gp, K))
    assert float((gate.detach().cpu() - ogate.detach()).abs().max()) <= 1e-5
    dg = np.random.default_rng(1).normal(0, 1, (n, K)).astype(np.float32)
    gate.backward(torch.from_numpy(dg).to(cuda))
    ogate.backward(torch.from_numpy(dg))
    a, b = g.params.grad.cpu().numpy(), gp.grad.numpy()
    lay = _gate_layer_errors(K, a, b)
    print(f"gate module K={K} n={n}: whole {rel(a, b):.2e} per layer max {max(lay.values()):.2e}")
    assert rel(a, b) <= 1.5e-3
    assert max(lay.values()) <= GATE_TOL, lay


# ------------------------------------------------------------------ 3. combine
@pytest.mark.parametrize("B", [1, 63, 257])
@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_ml_combine_fw_bw_vs_fp64(cuda, K, B):
    """rn_ml_combine_fw / rn_ml_combine_bw against the reference's loop
    (per sub-NeRF rgb_i + bg (1 - opacity_i), gate-weighted sums; depth passed
    through per sub-NeRF) in torch fp64 with autograd.  Inputs in [0, 1] (rgb_k
    <= opacity_k as a composite gives them), seeds in [-1, 1]: every output is
    a sum of at most 16 (forward) / 4 (backward) products below 1 in magnitude,
    so 2e-6 (test_ml_combine_test_vs_torch's bar) covers fp32 rounding."""
    gen = torch.Generator().manual_seed(100 * K + B)
    gate = torch.softmax(torch.randn(B, K, generator=gen), 1)
    op_k = torch.rand(K, B, generator=gen)
    depth_k = torch.rand(K, B, generator=gen)
    rgb_k = torch.rand(K, B, 3, generator=gen) * op_k[:, :, None]
    d_rgb = torch.rand(B, 3, generator=gen) * 2 - 1
    d_op = torch.rand(B, generator=gen) * 2 - 1
    st = _st(cuda)
    c = lambda t: t.to(cuda).contiguous()
    for bg in (torch.ones(3), torch.tensor([0.0, 0.25, 1.0])):
        gd = gate.double().requires_grad_(True)
        rgb = torch.zeros(B, 3, dtype=torch.float64)
        op = torch.zeros(B, dtype=torch.float64)
        for i in range(K):
            r = rgb_k[i].double() + bg.double() * (1 - op_k[i].double())[:, None]
            rgb = rgb + r * gd[:, i][:, None]
            op = op + op_k[i].double() * gd[:, i]
        torch.autograd.backward([rgb, op], [d_rgb.double(), d_op.double()])
        bufs = [torch.full(s, GUARD, device=cuda) for s in ((B + 3, 3), (B + 3,), (B + 3, K))]
        g_, o_, d_, r_, b_ = c(gate), c(op_k), c(depth_k), c(rgb_k), c(bg)
        lib().ml_combine_fw(g_.data_ptr(), o_.data_ptr(), d_.data_ptr(), r_.data_ptr(),
                            b_.data_ptr(), B, K, *[t.data_ptr() for t in bufs], st)
        want = (rgb.detach(), op.detach(), depth_k.t().double())
        for name, got, ref in zip(("rgb", "opacity", "depth"), bufs, want):
            err = float((got[:B].cpu().double() - ref).abs().max())
            assert err <= 2e-6, (name, err)
            assert bool((got[B:] == GUARD).all()), name
        assert torch.equal(bufs[2][:B].cpu(), depth_k.t())         # a copy
        dgate = torch.full((B + 3, K), GUARD, device=cuda)
        gr, go = c(d_rgb), c(d_op)
        lib().ml_combine_bw(gr.data_ptr(), go.data_ptr(), o_.data_ptr(), r_.data_ptr(),
                            b_.data_ptr(), B, K, dgate.data_ptr(), st)
        err = float((dgate[:B].cpu().double() - gd.grad).abs().max())
        assert err <= 2e-6, ("dgate", err)
        assert bool((dgate[B:] == GUARD).all())


# -------------------------------------------------------------------- 4. chain
def _dropin(*a, **kw):
    return _ml_render(*a, fused=False, **kw)


def _run(fn, m, g, o, d, noise, seeds, cuda, esf):
    m.zero_grad(); g.zero_grad()
    to = lambda a: torch.from_numpy(a).to(cuda)
    res = fn(m, g, to(o), to(d), to(d), noise=to(noise), exp_step_factor=esf)
    torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], [to(s) for s in seeds])
    return res, [m.xyz_encoder.params.grad.clone(), m.mlp_params.grad.clone(),
                 g.params.grad.clone()]


FIELD_ENTRIES = ("field_fwd", "field_bwd", "field_fwd_merged", "field_fwd_levels",
                 "field_bwd_merged", "bwd_plan")


def _count_field_launches(monkeypatch):
    """wraps the library's field entry points with counters: which kernels a
    step really ran"""
    L, n = lib(), {k: 0 for k in FIELD_ENTRIES}
    for name in FIELD_ENTRIES:
        def wrap(*a, _f=getattr(L, name), _n=name):
            n[_n] += 1
            return _f(*a)
        monkeypatch.setattr(L, name, wrap)
    return n


# (scale, K, B): 72 rays = two full gate tiles and a ragged one.  K = 8: the
# control, the merged chain at the same batch and bars
@pytest.mark.parametrize("scale,K,B", [(0.5, 8, 72), (16.0, 8, 72), (0.5, 9, 72), (16.0, 16, 72)])
def test_chain_defaults_vs_dropin_vs_oracle(cuda, monkeypatch, scale, K, B):
    """test_gpu_ml.py::test_fused_vs_dropin_vs_oracle with the defaults a model
    of this size gets (nothing set by hand) and without its fixed-point checks
    (the per-model backward scatters with fp32 atomics only): above 8 sub-NeRFs
    merged_bwd / merged_fwd / level_fwd are off and rn_field_fwd / rn_field_bwd
    run once per step with no plan; fused vs drop-in chain (outputs 1e-5,
    gradients 1e-3), march bit-exact and outputs within 1e-4 of the oracle,
    gradients per grid level / MLP layer / gate within parity.check_grads'
    bars.  Measured: DESIGN.md §2."""
    esf = 1 / 256 if scale > 0.5 else 0.0
    sc = S.parity_scene(K, B, scale=scale, device=cuda)
    m, g, o, d, noise, seeds, bits = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bits
    r = get_renderer(m, g, B)
    if K > 8:
        assert (r.merged_bwd, r.merged_fwd, r.level_fwd) == (False, False, False)
        assert (r.fwd_blocks, r.bwd_blocks) == (2048 // K, 256 // K)
        assert r.scatter_mode == "fp32-atomics"
    else:
        assert r.merged_bwd and r.merged_fwd and r.level_fwd
    launches = _count_field_launches(monkeypatch)
    rf, gf = _run(ml_render_fused, m, g, o, d, noise, seeds, cuda, esf)
    if K > 8:
        assert launches == dict.fromkeys(FIELD_ENTRIES, 0) | {"field_fwd": 1, "field_bwd": 1}
    else:
        assert launches["field_fwd"] == launches["field_bwd"] == 0
        assert launches["field_fwd_levels"] == launches["field_bwd_merged"] == 1
    monkeypatch.undo()
    rd, gd = _run(_dropin, m, g, o, d, noise, seeds, cuda, esf)
    for k in ("rgb", "opacity", "depth", "gating_code"):
        assert torch.allclose(rf[k], rd[k], atol=1e-5, rtol=0), k
    for a, b in zip(gf, gd):
        e = (a - b).norm() / b.norm().clamp_min(1e-30)
        assert e <= 1e-3, e
    ores = ml_oracle.ml_train_step(o, d, bits, noise,
                                   m.xyz_encoder.params.detach().cpu().view(-1, 2),
                                   m.mlp_params.detach().cpu(), g.params.detach().cpu(), scale,
                                   seeds=seeds)
    w = r.ws
    cnt = w.counts.cpu().numpy()
    assert np.array_equal(cnt, ores["counts"])
    # the scan's bases: every later sub-NeRF's samples sit where the oracle's do
    off = w.offsets.cpu().numpy()
    ts, dl = w.ts.cpu().numpy(), w.deltas.cpu().numpy()
    for k in range(K):
        for ray in range(B):
            a, c, n = off[k, ray], ores["starts"][k, ray], cnt[k, ray]
            assert np.array_equal(ts[a:a + n].view(np.uint32), ores["ts"][c:c + n].view(np.uint32))
            assert np.array_equal(dl[a:a + n].view(np.uint32),
                                  ores["deltas"][c:c + n].view(np.uint32))
    errs = {k: float(np.abs(rf[k].detach().cpu().numpy() - ores[k]).max())
            for k in ("rgb", "opacity", "depth")}
    e_gate = float(np.abs(rf["gating_code"].detach().cpu().numpy() - ores["gate"]).max())
    print(f"chain scale {scale} K {K} B {B}: {int(cnt.sum())} samples; {errs} gate {e_gate:.2e}")
    assert all(v <= 1e-4 for v in errs.values()), errs
    assert e_gate <= 1e-5
    check_grads(scale, gf[0].cpu().view(-1, 2).numpy(), ores["grid_grad"], gf[1].cpu().numpy(),
                ores["mlp_grad"], gf[2].cpu().numpy(), ores["gate_grad"], f"chain s{scale} K{K}")
    # printed, not asserted: at scale 16 the softmax saturates and a sub-NeRF
    # whose gate stays below 1e-7 on every ray has a dz under the f16 normal
    # range of the wave's gradient scale -- W4 row 3 measures 4.4e-3 at K = 8
    # and 3.1e-2 at K = 16, every other row <= 2.0e-3;
    # test_gate_rows_per_layer holds every row on an unsaturated gate
    lay = _gate_layer_errors(K, gf[2].cpu().numpy(), np.asarray(ores["gate_grad"]).reshape(-1))
    print(f"chain s{scale} K{K}: gate per layer {['%s %.1e' % kv for kv in lay.items()]}")


# --------------------------------------------------------------- 5. validation
def _camera(W, H, scale, half=0.6):
    """as tests/test_gpu_evaluate.py::_camera: a pinhole's unit pixel
    directions and a pose on the ring of radius 3 * scale looking at the origin"""
    y, x = torch.meshgrid(torch.linspace(-half * H / W, half * H / W, H),
                          torch.linspace(-half, half, W), indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    pos = 3 * scale * torch.tensor([np.cos(1.5), np.sin(1.5), 0.3 * np.sin(4.5)],
                                   dtype=torch.float32)
    fwd = -pos / pos.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
    right = right / right.norm()
    up = torch.linalg.cross(right, fwd)
    return dirs, torch.cat([torch.stack([right, up, fwd], 1), pos[:, None]], 1).contiguous()


def test_image_evaluator_nine_models(cuda):
    """ImageEvaluator.render_image at K = 9 on a 16 x 12 image in chunks of 80
    rays (two full, one of 32): against rendering.ml_render(test_time=True) on
    the same rays (the same render kernel: 2e-6, test_gpu_evaluate.py's bar)
    and against the CPU oracle's test-time loop (1e-4, test_gpu_render.py's
    bar for the same comparison)."""
    from radnerf_amd.evaluate import ImageEvaluator
    from radnerf_amd.rays import batch_rays
    K, scale, (W, H) = 9, 0.5, (16, 12)
    sc = S.parity_scene(K, 8, scale=scale, p=0.3, device=cuda)
    m, g, bits = sc.m, sc.g, sc.bits
    dirs, pose = _camera(W, H, scale)
    dirs, pose = dirs.to(cuda), pose.to(cuda)
    N = W * H
    ev = ImageEvaluator(m, g, dirs, (W, H), chunk=80)
    res = {k: v.clone() for k, v in ev.render_image(pose).items()}
    zero = torch.zeros(N, dtype=torch.int64, device=cuda)
    o, d, i_d = batch_rays(dirs, pose[None].contiguous(), zero, torch.arange(N, device=cuda))
    with torch.no_grad():
        ref = _ml_render(m, g, o, d, i_d, test_time=True, exp_step_factor=0.0)
    errs = {"rgb": float((res["rgb"] - ref["rgb"]).abs().max()),
            "opacity": float((res["opacity"] - ref["opacity"]).abs().max()),
            "depth_k": float((res["depth_k"] - ref["depth"]).abs().max()),
            "gate": float((res["gating_code"] - ref["gating_code"]).abs().max())}
    assert res["depth_k"].shape == (N, K) and res["gating_code"].shape == (N, K)
    assert all(v <= 2e-6 for v in errs.values()), errs
    assert int(res["total_samples"]) == int(ref["total_samples"]) > 0
    orc = ml_oracle.ml_render_test(o.cpu().numpy(), d.cpu().numpy(), bits,
                                   m.xyz_encoder.params.detach().cpu().view(-1, 2),
                                   m.mlp_params.detach().cpu(), g.params.detach().cpu(), scale)
    oerrs = {"rgb": float(np.abs(res["rgb"].cpu().numpy() - orc["rgb"]).max()),
             "opacity": float(np.abs(res["opacity"].cpu().numpy() - orc["opacity"]).max()),
             "depth_k": float(np.abs(res["depth_k"].cpu().numpy() - orc["depth"]).max()),
             "gate": float(np.abs(res["gating_code"].cpu().numpy() - orc["gate"]).max())}
    print(f"ImageEvaluator K=9 {W}x{H}: vs ml_render {errs}; vs oracle {oerrs}; opacity mean "
          f"{float(orc['opacity'].mean()):.3f}, samples {int(res['total_samples'])}")
    assert all(oerrs[k] <= 1e-4 for k in ("rgb", "opacity", "depth_k")), oerrs
    assert oerrs["gate"] <= 1e-5
    assert 0.02 < float(orc["opacity"].mean()) < 0.999          # hits and background


# -------------------------------------------------------------------- 6. hooks
@pytest.mark.parametrize("K,per_model_by_hand", [(9, False), (2, True)])
def test_per_model_backward_calls_hooks(cuda, K, per_model_by_hand):
    """The per-model backward (the default above 8 sub-NeRFs, or merged_bwd
    switched off) calls after_field_bwd and then after_grid_levels(0), once
    each per backward: a data-parallel caller launches its all-reduces from
    them (bench.py, tests/dp_worker.py), so a branch that skips them silently
    trains without the all-reduce.  Empty hooks change nothing: the gradients
    equal the no-hook run's bitwise whenever the no-hook backward reproduces
    itself bitwise (its grid scatter is fp32 atomics, whose order the hardware
    does not promise), and to the float-atomic order bar of test_gpu_ml.py
    (1e-5 relative) otherwise."""
    B = 72
    sc = S.parity_scene(K, B, device=cuda)
    m, g, o, d, noise, seeds = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds
    r = get_renderer(m, g, B)
    if per_model_by_hand:
        r.merged_bwd = False
    assert not r.merged_bwd
    _, ref = _run(ml_render_fused, m, g, o, d, noise, seeds, cuda, 0.0)
    _, ref2 = _run(ml_render_fused, m, g, o, d, noise, seeds, cuda, 0.0)
    calls = []
    r.after_field_bwd = lambda: calls.append(("field_bwd",))
    r.after_grid_levels = lambda level: calls.append(("grid_levels", level))
    _, hooked = _run(ml_render_fused, m, g, o, d, noise, seeds, cuda, 0.0)
    assert calls == [("field_bwd",), ("grid_levels", 0)], calls
    _run(ml_render_fused, m, g, o, d, noise, seeds, cuda, 0.0)
    assert calls == [("field_bwd",), ("grid_levels", 0)] * 2, calls
    r.after_field_bwd = r.after_grid_levels = None
    reproducible = all(torch.equal(a, b) for a, b in zip(ref, ref2))
    print(f"hooks K={K}: no-hook backward bitwise reproducible: {reproducible}")
    for a, b in zip(hooked, ref):
        assert float(b.abs().max()) > 0
        if reproducible:
            assert torch.equal(a, b)
        else:
            assert float((a - b).norm() / b.norm()) <= 1e-5
