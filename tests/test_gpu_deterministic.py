"""GPU: the deterministic training mode (FusedMLRenderer(deterministic=True),
Trainer(deterministic=True); DESIGN.md §4 "Deterministic training").

On one GPU in one process the same parameters, inputs and seed must give the
same bits whatever the order blocks and waves run in.  The four fp32 sums of
a step that went in arrival order (MLP dW, gate dW, gate importance, loss
terms) are ordered sums in this mode and the grid gradient is the exact
integer form, so every comparison of two runs here is torch.equal.

Shapes (B, K, scale), chosen so the schedule matters: (1024, 2, 0.5),
(512, 4, 16), (256, 8, 16), (256, 1, 0.5); each with the renderer's default
chunking and with 8 persistent blocks and chunks of 64 merged positions (max,
tail and head alike).  64 is a quarter of one block iteration (8 waves x 32
samples) and the smallest chunk tests/test_gpu_ml.py runs; a ray's samples of
all K sub-NeRFs are more than that, so nearly every chunk is one whole ray or
empty, and a smaller bound only adds empty chunks.  The plan then has far more
than 4 chunks per block (asserted from queue[1]), so every block takes several
chunks and every model is met by several blocks.

  1. two separately built renderers, three train_steps each, a large matmul on
     another stream during two of them: all six results bit-equal;
  2. mlp_grad / gate_grad equal the float32 loop over the per-block slots bit
     for bit; rn_reduce_partials and rn_colsum_ordered on their own;
  3. the same gradients as the default mode to 1e-5 (the bar of
     test_gpu_ml.py::test_int_grad_matches_fp32), bit-equal forward outputs;
  4. two trainers, 40 sampled steps (three grid updates, warm-up and after),
     with and without pose refinement: every parameter, Adam moment, density
     grid, bitfield and loss term bit-equal; fit() lands on the same bits;
  5. with the flag off nothing is allocated and scatter_mode is what it was;
  6. ml_render(..., deterministic=True) runs the autograd path on a cached
     deterministic renderer of its own.

Case 2 also runs the smallest shape on 512 persistent blocks, more than its
plan has chunks: the blocks past the plan leave their slots zero.  The slots
hold NaN before the step, so what the test reads is what the step wrote.
"""
import math

import numpy as np
import pytest
import torch

from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from radnerf_amd.fused import FusedMLRenderer
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.sampler import cosine_lr
from radnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 2, 0.5), (512, 4, 16.0), (256, 8, 16.0), (256, 1, 0.5)]
CHUNKINGS = ["default", "small"]
SMALL_BLOCKS, SMALL_CHUNK = 8, 64
IDLE_BLOCKS = 512       # more persistent blocks than the smallest shape's plan has chunks
LAMBDAS = dict(lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3, lambda_distortion=1e-3)

_SCENES = {}


def _scene(cuda, B, K, scale):
    """model, gate and one batch of synthetic.parity_scene (occupancy p = 0.5);
    built once per shape and never written to"""
    key = (B, K, scale)
    if key not in _SCENES:
        ps = S.parity_scene(K, B, scale=scale, device=cuda)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        gen = torch.Generator().manual_seed(11)
        _SCENES[key] = dict(m=ps.m, g=ps.g, o=to(ps.o), d=to(ps.d), noise=to(ps.noise),
                            target=torch.rand(B, 3, generator=gen).to(cuda),
                            bg=torch.ones(3, device=cuda),
                            esf=1 / 256 if scale > 0.5 else 0.0)
    return _SCENES[key]


def _renderer(sc, B, chunking, deterministic):
    r = FusedMLRenderer(sc["m"], sc["g"], B, deterministic=deterministic)
    if chunking == "small":
        r.merged_blocks = SMALL_BLOCKS
        r.max_chunk = r.min_chunk = r.head_chunk = SMALL_CHUNK
    elif chunking == "idle":
        r.merged_blocks = IDLE_BLOCKS
    return r


def _step(r, sc, input_grad=False):
    """one train_step into zeroed gradient buffers; everything it produced, cloned"""
    m, g = sc["m"], sc["g"]
    gg = torch.zeros_like(m.xyz_encoder.params)
    mg = torch.zeros_like(m.mlp_params)
    ag = torch.zeros_like(g.params)
    out = r.train_step(sc["o"], sc["d"], sc["d"], sc["target"], sc["noise"], sc["bg"],
                       exp_step_factor=sc["esf"], grid_grad=gg, mlp_grad=mg, gate_grad=ag,
                       input_grad=input_grad, **LAMBDAS)
    res = {"grid_grad": gg, "mlp_grad": mg, "gate_grad": ag}
    for k, v in out[0].items():
        res["term_" + k] = v.clone()
    for k in ("rgb", "opacity", "depth"):
        res[k] = r.last_forward[k].clone()
    if input_grad:
        w = r.ws
        res.update(drays_o=w.drays_o.clone(), drays_d=w.drays_d.clone(),
                   gate_dx=w.gate_dx.clone())
    return res


def _assert_small_plan(r):
    n_chunks = int(r.ws.queue[1])
    assert n_chunks >= 4 * SMALL_BLOCKS, n_chunks
    return n_chunks


class _Busy:
    """a large matmul queue on another stream, so the step's blocks share the
    CUs with it and arrive in another order"""

    def __init__(self, cuda):
        self.stream = torch.cuda.Stream(cuda)
        self.a = torch.randn(4096, 4096, device=cuda)
        torch.cuda.synchronize()

    def start(self, n=12):
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                self.a @ self.a


@pytest.mark.parametrize("input_grad", [False, True])
@pytest.mark.parametrize("chunking", CHUNKINGS)
@pytest.mark.parametrize("B,K,scale", SHAPES)
def test_repeatable_step(cuda, B, K, scale, chunking, input_grad):
    sc = _scene(cuda, B, K, scale)
    busy = _Busy(cuda)
    results = []
    for which in range(2):
        r = _renderer(sc, B, chunking, True)
        for i in range(3):
            if which == 1 and i >= 1:
                busy.start()
            results.append(_step(r, sc, input_grad))
        if chunking == "small":
            _assert_small_plan(r)
        torch.cuda.synchronize()
    want = {"grid_grad", "mlp_grad", "gate_grad", "term_rgb", "term_opacity", "term_distortion",
            "rgb", "opacity", "depth"}
    if K > 1:
        want |= {"term_cv_importance", "term_depth_mutual"}
    if input_grad:
        want |= {"drays_o", "drays_d", "gate_dx"}
    assert set(results[0]) == want
    for k in sorted(want):
        for i, other in enumerate(results[1:], 1):
            assert torch.equal(results[0][k], other[k]), (k, i)
    assert float(results[0]["grid_grad"].abs().max()) > 0
    assert float(results[0]["mlp_grad"].abs().max()) > 0


def _loop_sum(part, acc=None):
    """the order contract, restated: float32 adds in ascending slot order"""
    part = np.asarray(part, dtype=np.float32)
    acc = np.zeros(part.shape[1], np.float32) if acc is None else acc.astype(np.float32)
    for s in range(part.shape[0]):
        acc = acc + part[s]
    return acc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("B,K,scale,chunking",
                         [s + (c,) for s in SHAPES for c in CHUNKINGS] + [(256, 1, 0.5, "idle")])
def test_order_contract_of_the_step(cuda, B, K, scale, chunking):
    sc = _scene(cuda, B, K, scale)
    r = _renderer(sc, B, chunking, True)
    # the slots as the step finds them hold NaN: what it leaves is its own
    r.ws.dw_part = torch.full((r.merged_blocks, K * LY.FIELD_PARAMS), float("nan"), device=cuda)
    if K > 1:
        r.ws.gate_part = torch.full((max(1, min(128, (B + 127) // 128)), sc["g"].params.numel()),
                                    float("nan"), device=cuda)
        gate_part_before = r.ws.gate_part
    dw_part_before = r.ws.dw_part
    res = _step(r, sc)
    torch.cuda.synchronize()
    w = r.ws
    n_chunks = int(w.queue[1])
    blocks = r.merged_blocks
    assert w.dw_part is dw_part_before and (K == 1 or w.gate_part is gate_part_before)
    assert w.dw_part.shape == (blocks, K * LY.FIELD_PARAMS)
    part = w.dw_part.cpu().numpy()
    assert np.array_equal(_bits(_loop_sum(part)), _bits(res["mlp_grad"].cpu().numpy().ravel()))
    # chunk c goes to block c mod blocks: a block past the plan took none
    idle = list(range(min(n_chunks, blocks), blocks))
    for b in idle:
        assert not part[b].any(), b
    assert (len(idle) > 0) == (chunking == "idle")
    busy_slots = int((np.abs(part).max(1) > 0).sum())
    print(f"B {B} K {K} s {scale} {chunking}: {n_chunks} chunks on {blocks} blocks, "
          f"{busy_slots} slots written, {len(idle)} idle")
    assert busy_slots >= 2                      # several blocks' partials are summed
    if chunking == "small":
        _assert_small_plan(r)
        # every model is met by several blocks
        per_model = np.abs(part.reshape(blocks, K, -1)).max(2) > 0
        assert (per_model.sum(0) >= 2).all(), per_model.sum(0)
    if K > 1:
        gp = w.gate_part.cpu().numpy()
        assert gp.shape[1] == sc["g"].params.numel() and gp.shape[0] >= 2
        assert np.array_equal(_bits(_loop_sum(gp)), _bits(res["gate_grad"].cpu().numpy()))
        assert float(np.abs(gp).max()) > 0
    else:
        assert float(res["gate_grad"].abs().max()) == 0


def test_reduce_partials_is_the_loop(cuda):
    L = lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    gen = torch.Generator().manual_seed(5)
    for n_slots in (1, 2, 7, 300):
        for n in (1, 63, 64, 65, 9472 * 2):
            # magnitudes spread over ~2^20, so the order of the adds shows
            part = (torch.randn(n_slots, n, generator=gen) *
                    torch.exp2(torch.randint(-10, 10, (n_slots, n), generator=gen).float()))
            for incoming in (False, True):
                out0 = torch.randn(n, generator=gen) if incoming else torch.zeros(n)
                out = out0.to(cuda)
                L.reduce_partials(part.to(cuda).data_ptr(), n_slots, n, out.data_ptr(), st)
                want = _loop_sum(part.numpy(), out0.numpy())
                assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (n_slots, n, incoming)
    # not a tree: a case where pairwise summation rounds differently
    part = torch.tensor([[1.0], [2.0 ** -24], [2.0 ** -24], [2.0 ** -24]])
    out = torch.zeros(1, device=cuda)
    L.reduce_partials(part.to(cuda).data_ptr(), 4, 1, out.data_ptr(), st)
    assert float(out) == 1.0 == float(_loop_sum(part.numpy())[0])
    # n == 0 is accepted and touches nothing
    L.reduce_partials(part.to(cuda).data_ptr(), 4, 0, out.data_ptr(), st)
    assert float(out) == 1.0


def test_colsum_ordered(cuda):
    L = lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    gen = torch.Generator().manual_seed(6)
    for rows in (1, 31, 32, 33, 8192):
        for cols in (1, 5, 16):
            x = torch.randn(rows, cols, generator=gen)
            xd = x.to(cuda)
            outs = []
            for _ in range(3):
                out = torch.full((cols,), float("nan"), device=cuda)
                L.colsum_ordered(xd.data_ptr(), rows, cols, out.data_ptr(), st)
                outs.append(out.cpu())
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
            ref = x.double().sum(0)
            bound = rows * 2.0 ** -24 * x.double().abs().sum(0)
            err = (outs[0].double() - ref).abs()
            assert bool((err <= bound).all()), (rows, cols, float((err / bound).max()))
    # a softmax output: every column sum is what gate.sum(0) gives, to rounding
    g = torch.softmax(torch.randn(777, 4, generator=gen), 1).to(cuda)
    out = torch.empty(4, device=cuda)
    L.colsum_ordered(g.data_ptr(), 777, 4, out.data_ptr(), st)
    assert torch.allclose(out, g.sum(0), rtol=1e-5)


@pytest.mark.parametrize("chunking", CHUNKINGS)
@pytest.mark.parametrize("B,K,scale", SHAPES)
def test_same_gradients_as_the_default_mode(cuda, B, K, scale, chunking):
    """The default renderer's first backward of a workspace scatters in fp32
    (no fixed-point scale yet), the comparison test_int_grad_matches_fp32
    makes; both renderers cut the same chunks."""
    sc = _scene(cuda, B, K, scale)
    det = _step(_renderer(sc, B, chunking, True), sc)
    ref = _step(_renderer(sc, B, chunking, False), sc)
    for k in ("rgb", "opacity", "depth"):
        assert torch.equal(det[k], ref[k]), k
    for k in ("grid_grad", "mlp_grad", "gate_grad"):
        a, b = det[k].double(), ref[k].double()
        if float(b.norm()) == 0:
            assert float(a.norm()) == 0, k
            continue
        rel = float((a - b).norm() / b.norm())
        print(f"B {B} K {K} s {scale} {chunking}: {k} rel {rel:.2e}")
        assert rel <= 1e-5, (k, rel)
    terms = [k for k in det if k.startswith("term_")]
    assert len(terms) == (5 if K > 1 else 3)
    for k in terms:
        a, b = float(det[k]), float(ref[k])
        # tests/test_gpu_train.py's bar for fused_nerf_loss against fp64
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (k, a, b)


# ---------------------------------------------------------------- training
WH, N_IMG, R_SPHERE = (32, 32), 4, 0.25


def _dataset(cuda):
    """4 images of 32 x 32 of tools/train_demo.py's analytic sphere (radius
    0.25, coloured 0.5 + 0.5 normal, white background), cameras on a ring"""
    W, H = WH
    half = 0.3
    y, x = torch.meshgrid(torch.linspace(-half, half, H), torch.linspace(-half, half, W),
                          indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    ang = torch.arange(N_IMG) * (2 * math.pi / N_IMG) + 0.3
    pos = 1.5 * torch.stack([torch.cos(ang), torch.sin(ang), 0.3 * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2).contiguous()
    d = torch.einsum("pj,nij->npi", dirs, poses[:, :, :3])
    o = poses[:, None, :, 3].expand_as(d)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - R_SPHERE ** 2)
    t = -b - torch.sqrt(disc.clamp_min(0))
    hit = (disc > 0) & (t > 0)
    nrm = o + t[..., None] * d
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    img = torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.ones_like(nrm))
    assert 0.02 < float(hit.float().mean()) < 0.9
    u8 = (img * 255).round().to(torch.uint8).contiguous()
    return dirs.to(cuda), poses.to(cuda), u8.to(cuda)


STEPS, EPOCHS, PER_EPOCH, LR = 40, 2, 20, 1e-2


def _trainer(cuda, data, K, scale, ext):
    dirs, poses, u8 = data
    m = MNGP(scale, size=K, seed=3).to(cuda)
    g = Ray_Gate(K, seed=4).to(cuda)
    return Trainer(m, g, 512, lr=LR, deterministic=True, seed=3, update_interval=16,
                   warmup_steps=16, images=u8, directions=dirs, poses=poses, optimize_ext=ext,
                   **LAMBDAS)


def _state(tr):
    m, g = tr.model, tr.gate
    st = {"grid": m.xyz_encoder.params, "mlp": m.mlp_params, "gate": g.params}
    params = dict(st)
    if tr.optimize_ext:
        params.update(dR=tr.dR, dT=tr.dT)
        st.update(dR=tr.dR, dT=tr.dT)
    for name, p in params.items():
        for mom in ("exp_avg", "exp_avg_sq"):
            st[f"{name}.{mom}"] = tr.opt.state[p][mom]
    for i in range(m.size):
        for what in ("density_grid", "density_bitfield"):
            st[f"{what}_{i}"] = getattr(m, f"{what}_{i}")
    return {k: v.detach().clone() for k, v in st.items()}


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("K,scale", [(2, 0.5), (4, 16.0)])
def test_repeatable_training(cuda, K, scale, ext):
    data = _dataset(cuda)
    busy = _Busy(cuda)
    runs = []
    for which in range(2):
        tr = _trainer(cuda, data, K, scale, ext)
        assert tr.renderer.deterministic and tr.renderer.scatter_mode == "int-grad"
        losses = []
        for step in range(STEPS):
            if step % PER_EPOCH == 0:       # fit's schedule, by hand
                tr.opt.param_groups[0]["lr"] = cosine_lr(LR, step // PER_EPOCH, EPOCHS)
            if which == 1 and step % 7 == 3:
                busy.start(4)
            terms = tr.step_sampled()
            losses.append(torch.stack([terms[k] for k in sorted(terms)]).clone())
        assert tr.global_step == STEPS
        runs.append((_state(tr), torch.stack(losses), sorted(terms)))
        torch.cuda.synchronize()
    (s0, l0, names), (s1, l1, _) = runs
    assert "rgb" in names and "distortion" in names and "cv_importance" in names
    assert bool(torch.isfinite(l0).all())
    assert torch.equal(l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    # the parameters moved, and the pose corrections with them
    fresh = MNGP(scale, size=K, seed=3)
    assert not torch.equal(s0["mlp"].cpu(), fresh.mlp_params.detach())
    if ext:
        assert float(s0["dR"].abs().max()) > 0 and float(s0["dT"].abs().max()) > 0
    # fit: the same 40 steps under its own epoch loop
    tr = _trainer(cuda, data, K, scale, ext)
    log = tr.fit(num_epochs=EPOCHS, steps_per_epoch=PER_EPOCH)
    assert tr.global_step == STEPS and [e["lr"] for e in log] == [
        cosine_lr(LR, e, EPOCHS) for e in range(EPOCHS)]
    s2 = _state(tr)
    for k in s0:
        assert torch.equal(s0[k], s2[k]), k


@pytest.mark.parametrize("B,K,scale,mode", [(1024, 2, 0.5, "fixed-point"),
                                            (512, 4, 16.0, "binned"),
                                            (256, 8, 16.0, "binned"),
                                            (256, 1, 0.5, "fp32-atomics")])
def test_default_untouched(cuda, B, K, scale, mode):
    sc = _scene(cuda, B, K, scale)
    r = _renderer(sc, B, "default", False)
    assert r.deterministic is False and r.scatter_mode == mode
    _step(r, sc)
    torch.cuda.synchronize()
    assert getattr(r.ws, "dw_part", None) is None and getattr(r.ws, "gate_part", None) is None
    assert getattr(r.ws, "_igrad", None) is None


def test_ml_render_takes_the_flag(cuda):
    """ml_render(..., fused=True, deterministic=True): the autograd path on a
    cached deterministic renderer of its own; gradients repeat bit for bit."""
    from radnerf_amd.fused import get_renderer
    from radnerf_amd.rendering import ml_render
    B, K, scale = 1024, 2, 0.5
    sc = _scene(cuda, B, K, scale)
    m, g = sc["m"], sc["g"]
    seeds = [torch.from_numpy(s).to(cuda) for s in S.loss_seeds(B, K)]
    grads = []
    for _ in range(2):
        m.zero_grad(); g.zero_grad()
        res = ml_render(m, g, sc["o"], sc["d"], sc["d"], noise=sc["noise"], deterministic=True)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], seeds)
        grads.append([p.grad.clone() for p in (m.xyz_encoder.params, m.mlp_params, g.params)])
    m.zero_grad(); g.zero_grad()
    r = get_renderer(m, g, B, deterministic=True)
    assert r.deterministic and r.scatter_mode == "int-grad" and r.ws.dw_part is not None
    assert get_renderer(m, g, B) is not r and not get_renderer(m, g, B).deterministic
    for a, b in zip(*grads):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
