"""GPU: error-guided sampling (csrc/guided.hip, sampler.GuidedSampler,
FusedMLRenderer.train_step(ray_weight=, guided=), Trainer(guided=True))
against its numpy restatement (tests/guided_ref.py).

Geometry of the sampling cases: 3 images of 37 x 21 with tile 16 (3 x 2 cells
per image, edge cells 5 wide and 5 tall), 1000 rays (three blocks and a tail
of 232).  Everything integer or a single rounded operation is compared bit for
bit.  Scan sizes: 1, 255, 256, 257 and 65,537 cells, and 1,049,604 cells (1026
scan blocks of 1024 cells: the one block that scans the block sums then takes
two sums per thread).
"""
import numpy as np
import pytest
import torch

import guided_ref as GR
import sampler_ref as SR
from march_ref import Guarded
from radnerf_amd import sampler
from radnerf_amd._lib import GUIDED_WORK_BYTES
from radnerf_amd.rays import batch_rays, pose_rays
from radnerf_amd.sampler import GUIDED_KEYS, GuidedSampler, TrainImages, sample_batch
from radnerf_amd.trainer import Trainer
from test_gpu_deterministic import LAMBDAS, WH, _dataset, _renderer, _scene, _state

pytestmark = pytest.mark.gpu

N_IMG, W, H, TILE, N, K, SEED = 3, 37, 21, 16, 1000, 2, 11
N_PIX = W * H
HOT = 7


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def scene(cuda):
    gen = torch.Generator().manual_seed(5)
    dirs = torch.randn(N_PIX, 3, generator=gen)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    poses = torch.randn(N_IMG, 3, 4, generator=gen).contiguous()
    u8 = torch.randint(0, 256, (N_IMG, N_PIX, 3), generator=gen, dtype=torch.uint8)
    f32 = torch.rand(N_IMG, N_PIX, 3, generator=gen)
    dR = 0.05 * torch.randn(N_IMG, 3, generator=gen)
    dT = 0.05 * torch.randn(N_IMG, 3, generator=gen)
    rng = np.random.default_rng(3)
    emap = rng.uniform(0.001, 0.2, 18).astype(np.float32)
    emap[HOT] = 3.0
    dirs = dirs.to(cuda)
    return {"dirs": dirs, "poses": poses.to(cuda), "uint8": u8.to(cuda), "fp32": f32.to(cuda),
            "dR": dR.to(cuda), "dT": dT.to(cuda), "mean_dir": dirs.mean(0).contiguous(),
            "emap": emap, "geo": GR.Geometry(N_IMG, W, H, TILE)}


def _sampler(cuda, images, wh, emap, tile=TILE, frac=0.5):
    gs = GuidedSampler(TrainImages(images), wh, tile=tile, uniform_frac=frac)
    assert float(gs.emap.min()) == 1.0 == float(gs.emap.max()) and not bool(gs.acc_cnt.any())
    gs.emap.copy_(torch.from_numpy(emap))
    gs.update_weights()
    return gs


# ---------------------------------------------------------------- sampling
@pytest.mark.parametrize("pose", [False, True])
@pytest.mark.parametrize("dtype", ["uint8", "fp32"])
@pytest.mark.parametrize("frac", [0.0, 0.5, 1.0])
def test_batch_matches_restatement(cuda, scene, frac, dtype, pose):
    geo, images = scene["geo"], scene[dtype]
    gs = _sampler(cuda, images, (W, H), scene["emap"], frac=frac)
    w, cdf = GR.weights(scene["emap"], geo)
    assert np.array_equal(_u32(gs.w), w) and np.array_equal(_u64(gs.cdf), cdf)
    step, rank = 5, 2
    kw = dict(rank=rank)
    if pose:
        kw.update(dR=scene["dR"], dT=scene["dT"], mean_dir=scene["mean_dir"])
    b = gs.sample(scene["dirs"], scene["poses"], N, K, SEED, step, **kw)
    assert set(b) == set(GUIDED_KEYS)
    img, pix, cell, wgt = GR.sample(SEED, step, rank, N, geo, w, cdf, frac)
    assert b["img_idxs"].dtype == torch.int64 and b["cell_idx"].dtype == torch.int32
    assert np.array_equal(b["img_idxs"].cpu().numpy(), img)
    assert np.array_equal(b["pix_idxs"].cpu().numpy(), pix)
    assert np.array_equal(b["cell_idx"].cpu().numpy(), cell)
    assert np.array_equal(b["ray_weight"].cpu().numpy().view(np.uint32), wgt.view(np.uint32))
    if 0 < frac < 1:
        i0, p0 = SR.picks(SEED, step, rank, N, N_IMG, N_PIX)
        moved = int(((img != i0) | (pix != p0)).sum())
        assert 0.3 * N < moved < 0.7 * N            # both branches ran
        assert float(b["ray_weight"].min()) < 1 < float(b["ray_weight"].max()) <= 1 / frac
    # target, rays, jitter and background: rn_sample_batch's on these picks
    ii, pp = b["img_idxs"], b["pix_idxs"]
    if dtype == "uint8":
        want = (images.cpu()[ii.cpu(), pp.cpu()].float() / 255).to(cuda)
    else:
        want = images[ii, pp]
    assert _same_bits(b["target"], want)
    if pose:
        o, d, i_d = pose_rays(scene["dirs"], scene["poses"], scene["dR"], scene["dT"], ii, pp,
                              mean_dir=scene["mean_dir"])
        assert _same_bits(b["imgs_d"], i_d)
    else:
        o, d, _ = batch_rays(scene["dirs"], scene["poses"], ii, pp)
        assert b["imgs_d"] is None
    assert _same_bits(b["rays_o"], o) and _same_bits(b["rays_d"], d)
    u = sample_batch(gs.images, scene["dirs"], scene["poses"], N, K, SEED, step, **kw)
    assert _same_bits(b["noise"], u["noise"]) and _same_bits(b["bg"], u["bg"])
    assert np.array_equal(b["noise"].cpu().numpy(), SR.noise(SEED, step, rank, K, N))
    if frac == 1.0:
        for k in sampler.KEYS:
            assert (b[k] is None and u[k] is None) or _same_bits(b[k].float(), u[k].float()), k
        assert torch.equal(b["img_idxs"], u["img_idxs"]) and torch.equal(b["pix_idxs"],
                                                                          u["pix_idxs"])
        assert bool((b["ray_weight"] == 1).all())
    # the buffers are reused
    again = gs.sample(scene["dirs"], scene["poses"], N, K, SEED, step + 1, out=b, **kw)
    assert again is b and not np.array_equal(b["pix_idxs"].cpu().numpy(), pix)


@pytest.mark.parametrize("n_img,wh,tile", [(300, (16, 16), 16), (1, (256, 256), 1),
                                           (20480, (2, 2), 2), (20481, (2, 2), 2)])
def test_two_level_search(cuda, n_img, wh, tile):
    """one cell per image (the search is all first level) and 65,536 cells in
    one image (all second level), against the plain bisection; 20,480 images
    fill the 160 KiB of LDS the image totals are staged in, one more and the
    first level reads them from memory"""
    geo = GR.Geometry(n_img, wh[0], wh[1], tile)
    rng = np.random.default_rng(n_img)
    emap = rng.uniform(0.0, 0.3, geo.n_cells).astype(np.float32)
    emap[rng.integers(0, geo.n_cells, 5)] = 2.0
    gen = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (n_img, geo.n_pix, 3), generator=gen, dtype=torch.uint8).to(cuda)
    dirs = torch.randn(geo.n_pix, 3, generator=gen).to(cuda)
    poses = torch.randn(n_img, 3, 4, generator=gen).to(cuda)
    gs = _sampler(cuda, images, wh, emap, tile=tile, frac=0.0)
    w, cdf = GR.weights(emap, geo)
    assert np.array_equal(_u32(gs.w), w) and np.array_equal(_u64(gs.cdf), cdf)
    b = gs.sample(dirs, poses, N, K, SEED, 9)
    img, pix, cell, wgt = GR.sample(SEED, 9, 0, N, geo, w, cdf, 0.0)
    assert np.array_equal(b["img_idxs"].cpu().numpy(), img)
    assert np.array_equal(b["pix_idxs"].cpu().numpy(), pix)
    assert np.array_equal(b["cell_idx"].cpu().numpy(), cell)
    assert np.array_equal(b["ray_weight"].cpu().numpy().view(np.uint32), wgt.view(np.uint32))
    assert len(set(cell.tolist())) > 100
    assert _same_bits(b["target"], (images.cpu()[img, pix].float() / 255).to(cuda))


# ---------------------------------------------------------------- weights and scan
@pytest.mark.parametrize("n_img,wh,tile", [
    (1, (5, 5), 16), (255, (16, 9), 16), (256, (7, 16), 16), (257, (16, 16), 16),
    (65537, (3, 2), 4), (174934, (37, 21), 16), (5, (300, 300), 256)])
def test_weights_and_scan(cuda, n_img, wh, tile):
    geo = GR.Geometry(n_img, wh[0], wh[1], tile)
    n = geo.n_cells
    rng = np.random.default_rng(n)
    emap = rng.uniform(0.0, 0.3, n).astype(np.float32)
    # the clamps (0 and NaN -> 1, 300 -> 2^24) and rounding ties (to even)
    special = np.array([0.0, 300.0, np.nan, 2.5 / 65536, 3.5 / 65536, 0.5 / 65536, 1.5 / 65536,
                        256.0, 255.99999], np.float32)
    at = rng.permutation(n)[:len(special)]
    emap[at] = special[:len(at)]
    if tile == 256:
        emap[:] = 300.0                     # every mass 2^24 * 65536 = 2^40
        emap[-1] = 0.1
    w = Guarded(n, torch.int32, cuda)
    cdf = Guarded(n, torch.int64, cuda)
    work = torch.empty(GUIDED_WORK_BYTES // 8, dtype=torch.int64, device=cuda)
    e = torch.from_numpy(emap).to(cuda)
    sampler.guided_weights(e, n_img, wh, tile, w.buf[:n], cdf.buf[:n], work)
    w_ref, cdf_ref = GR.weights(emap, geo)
    assert np.array_equal(w.check("w").view(np.uint32), w_ref)
    assert np.array_equal(cdf.check("cdf").view(np.uint64), cdf_ref)
    assert np.array_equal(cdf_ref, np.cumsum(w_ref.astype(np.uint64) * geo.n_px().astype(np.uint64),
                                             dtype=np.uint64))
    if n >= len(special) and tile != 256:
        got = dict(zip(special[:7].tolist(), w_ref[at[:7]].tolist()))
        assert [int(w_ref[i]) for i in at[:2]] == [1, 1 << 24] and int(w_ref[at[2]]) == 1
        assert [int(w_ref[i]) for i in at[3:7]] == [2, 4, 1, 2], got
    if tile == 256:
        assert int(cdf_ref[0]) == 1 << 40 and int(cdf_ref[-1]) > 1 << 32
    assert _same_bits(e, torch.from_numpy(emap).to(cuda))       # the map is read only


# ---------------------------------------------------------------- epilogue and refresh
def _epilogue_case(one_cell):
    rng = np.random.default_rng(17 + one_cell)
    n = 5000
    rgb = rng.random((n, 3), dtype=np.float32)
    tgt = rng.random((n, 3), dtype=np.float32)
    rgb[11, 1], rgb[70, 0], rgb[71, 2], rgb[4000] = np.nan, np.inf, -np.inf, 1e3
    rgb[4999] = tgt[4999]                                       # e = 0 counts
    cell = (np.full(n, HOT) if one_cell else rng.integers(0, 18, n)).astype(np.int32)
    wgt = rng.uniform(0.3, 2.0, n).astype(np.float32)
    seeds = [rng.standard_normal((n, 3)).astype(np.float32),
             rng.standard_normal(n).astype(np.float32),
             rng.standard_normal((n, K)).astype(np.float32)]
    return rgb, tgt, cell, wgt, seeds


@pytest.mark.parametrize("one_cell", [True, False])
def test_epilogue_and_refresh(cuda, one_cell):
    rgb, tgt, cell, wgt, seeds = _epilogue_case(one_cell)
    n, n_cells = len(cell), 18
    dev = lambda a: torch.from_numpy(a).to(cuda)
    acc_sum, acc_cnt = Guarded(n_cells, torch.int64, cuda), Guarded(n_cells, torch.int32, cuda)
    prior_sum = np.arange(n_cells, dtype=np.uint64) * np.uint64(3)
    prior_cnt = (np.arange(n_cells) % 3).astype(np.uint32)
    prior_sum[prior_cnt == 0] = 0
    acc_sum.buf[:n_cells] = dev(prior_sum.view(np.int64))
    acc_cnt.buf[:n_cells] = dev(prior_cnt.view(np.int32))
    bufs = [Guarded(s.shape, torch.float32, cuda) for s in seeds]
    for g, s in zip(bufs, seeds):
        g.buf[:g.n] = dev(s).reshape(-1)
    d_gate = torch.randn(n, K, device=cuda)
    d_gate0 = d_gate.clone()
    views = [g.buf[:g.n].view(g.shape) for g in bufs]
    sampler.guided_epilogue(dev(rgb), dev(tgt), dev(cell), dev(wgt), K, acc_sum.buf[:n_cells],
                            acc_cnt.buf[:n_cells], *views)
    ref_sum, ref_cnt = prior_sum.copy(), prior_cnt.copy()
    want = GR.epilogue(rgb, tgt, cell, wgt, ref_sum, ref_cnt, seeds)
    got_sum, got_cnt = acc_sum.check("acc_sum").view(np.uint64), acc_cnt.check("acc_cnt").view(np.uint32)
    assert np.array_equal(got_sum, ref_sum) and np.array_equal(got_cnt, ref_cnt)
    assert int(ref_cnt.sum() - prior_cnt.sum()) == n - 3
    for g, x, name in zip(bufs, want, ("dL_drgb", "dL_dopacity", "dL_ddepth")):
        assert np.array_equal(g.check(name).view(np.uint32), x.view(np.uint32)), name
    assert torch.equal(d_gate, d_gate0)
    # without accumulators: the seeds are weighted, nothing else is read
    again = [dev(s) for s in seeds]
    sampler.guided_epilogue(None, None, None, dev(wgt), K, None, None, *again)
    for a, x in zip(again, want):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), x.view(np.uint32))
    # ---- refresh, from these accumulators
    rng = np.random.default_rng(2)
    emap = rng.uniform(0.0, 1.0, n_cells).astype(np.float32)
    e = Guarded(n_cells, torch.float32, cuda)
    e.buf[:n_cells] = dev(emap)
    seen = ref_cnt > 0
    assert seen.any() and (one_cell is False or (~seen).any())
    sampler.guided_refresh(e.buf[:n_cells], acc_sum.buf[:n_cells], acc_cnt.buf[:n_cells], 0.3)
    new = GR.refresh(emap, ref_sum, ref_cnt, 0.3)
    got = e.check("emap")
    assert np.array_equal(got.view(np.uint32), new.view(np.uint32))
    assert np.array_equal(got[~seen].view(np.uint32), emap[~seen].view(np.uint32))
    assert not (got[seen] == emap[seen]).all()
    assert not acc_sum.check("acc_sum").any() and not acc_cnt.check("acc_cnt").any()
    sampler.guided_refresh(e.buf[:n_cells], acc_sum.buf[:n_cells], acc_cnt.buf[:n_cells], 0.3)
    assert np.array_equal(e.check("emap").view(np.uint32), new.view(np.uint32))
    assert not acc_sum.check("acc_sum").any() and not acc_cnt.check("acc_cnt").any()


# ---------------------------------------------------------------- the chain
CHAIN = (512, 4, 16.0)


def _chain_step(cuda, lambdas, weight=None, guided=None):
    """one deterministic train_step of a fresh renderer into zeroed buffers"""
    B, K_, scale = CHAIN
    sc = _scene(cuda, B, K_, scale)
    r = _renderer(sc, B, "default", True)
    m, g = sc["m"], sc["g"]
    res = {"grid_grad": torch.zeros_like(m.xyz_encoder.params),
           "mlp_grad": torch.zeros_like(m.mlp_params), "gate_grad": torch.zeros_like(g.params)}
    kw = {} if weight is None else dict(
        ray_weight=torch.full((B,), float(weight), device=cuda), guided=guided)
    terms, _ = r.train_step(sc["o"], sc["d"], sc["d"], sc["target"], sc["noise"], sc["bg"],
                            exp_step_factor=sc["esf"], grid_grad=res["grid_grad"],
                            mlp_grad=res["mlp_grad"], gate_grad=res["gate_grad"], **lambdas, **kw)
    for k, v in terms.items():
        res["term_" + k] = v.clone()
    torch.cuda.synchronize()
    return res


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_unit_weights_change_nothing(cuda):
    ref = _chain_step(cuda, LAMBDAS)
    one = _chain_step(cuda, LAMBDAS, weight=1.0)
    assert set(ref) == set(one) and "term_distortion" in ref and "term_cv_importance" in ref
    for k in ref:
        assert torch.equal(ref[k], one[k]), k
    assert float(ref["grid_grad"].abs().max()) > 0


def test_half_weights_halve_the_gradients(cuda):
    """every seed but the cv^2 term's is weighted: with that term off the
    gradients are half the unweighted ones, to the 1e-5 of
    test_gpu_deterministic.py::test_same_gradients_as_the_default_mode; the
    terms stay the unweighted means"""
    lam = dict(LAMBDAS, lambda_cv_importance=0.0)
    ref = _chain_step(cuda, lam)
    half = _chain_step(cuda, lam, weight=0.5)
    for k in ("grid_grad", "mlp_grad", "gate_grad"):
        rel = _rel(2 * half[k], ref[k])
        print(f"{k}: rel {rel:.2e}")
        assert rel <= 1e-5, (k, rel)
    for k in ref:
        if k.startswith("term_"):
            assert torch.equal(ref[k], half[k]), k
    # the distortion share alone: lambda 1.0, so that it is of the size of the rest
    base = dict(lam, lambda_distortion=0.0)
    big = dict(lam, lambda_distortion=1.0)
    r0, r1 = _chain_step(cuda, base), _chain_step(cuda, big)
    h0, h1 = _chain_step(cuda, base, weight=0.5), _chain_step(cuda, big, weight=0.5)
    for k in ("grid_grad", "mlp_grad"):
        share, share_h = r1[k].double() - r0[k].double(), h1[k].double() - h0[k].double()
        rel = float((2 * share_h - share).norm() / share.norm())
        print(f"distortion share of {k}: rel {rel:.2e}, share / whole "
              f"{float(share.norm() / r1[k].double().norm()):.2f}")
        assert float(share.norm()) > 0.1 * float(r1[k].double().norm())
        assert rel <= 1e-5, (k, rel)


def test_seeds_handed_to_the_backward(cuda):
    """what train_step passes on: the seeds on rgb, opacity and depth are the
    loss's times the weights bit for bit, the distortion seed is the [K][B]
    tensor lambda w / B, and dL_dgate (the cv^2 term, a batch statistic) is
    the loss's own"""
    B, K_, scale = CHAIN
    sc = _scene(cuda, B, K_, scale)
    lam = dict(LAMBDAS, lambda_cv_importance=1.0)
    gen = torch.Generator().manual_seed(8)
    w = (0.25 + 1.5 * torch.rand(B, generator=gen)).to(cuda)
    seen = []
    for weight in (None, w):
        r = _renderer(sc, B, "default", True)
        inner = r.backward

        def spy(*a, _inner=inner):
            seen.append([None if not torch.is_tensor(t) else t.clone() for t in a[5:9]] + [a[13]])
            return _inner(*a)
        r.backward = spy
        kw = {} if weight is None else dict(ray_weight=weight)
        r.train_step(sc["o"], sc["d"], sc["d"], sc["target"], sc["noise"], sc["bg"],
                     exp_step_factor=sc["esf"], **lam, **kw)
    (rgb0, op0, dep0, gate0, dist0), (rgb1, op1, dep1, gate1, dist1) = seen
    assert _same_bits(rgb1, rgb0 * w[:, None]) and _same_bits(op1, op0 * w)
    assert _same_bits(dep1, dep0 * w[:, None])
    assert torch.equal(gate1, gate0) and float(gate0.abs().max()) > 0
    assert isinstance(dist0, float) and dist0 == LAMBDAS["lambda_distortion"] / B
    assert dist1.shape == (K_, B) and dist1.is_contiguous()
    assert _same_bits(dist1, (w * dist0).expand(K_, B))


def test_train_step_records_the_errors(cuda):
    B, K_, scale = CHAIN
    sc = _scene(cuda, B, K_, scale)
    images = torch.zeros(1, 64 * 64, 3, dtype=torch.uint8, device=cuda)
    gs = GuidedSampler(TrainImages(images), (64, 64))
    cells = (torch.arange(B, device=cuda) % 16).int()
    r = _renderer(sc, B, "default", True)
    w = torch.ones(B, device=cuda)
    r.train_step(sc["o"], sc["d"], sc["d"], sc["target"], sc["noise"], sc["bg"],
                 exp_step_factor=sc["esf"], ray_weight=w, guided=(gs, cells), **LAMBDAS)
    rgb = r.last_forward["rgb"].cpu().numpy()
    s, c = np.zeros(16, np.uint64), np.zeros(16, np.uint32)
    GR.epilogue(rgb, sc["target"].cpu().numpy(), cells.cpu().numpy(), w.cpu().numpy(), s, c, [])
    assert np.array_equal(_u64(gs.acc_sum), s) and np.array_equal(_u32(gs.acc_cnt), c)
    assert int(c.sum()) == B
    with pytest.raises(ValueError, match="needs ray_weight"):
        r.train_step(sc["o"], sc["d"], sc["d"], sc["target"], sc["noise"], sc["bg"],
                     guided=(gs, cells))


# ---------------------------------------------------------------- the trainer
STEPS, CUT, EVERY = 24, 13, 8


def _trainer(cuda, data, guided=True):
    from radnerf_amd.networks import MNGP, Ray_Gate
    dirs, poses, u8 = data
    m = MNGP(0.5, size=2, seed=3).to(cuda)
    g = Ray_Gate(2, seed=4).to(cuda)
    kw = dict(guided=True, guided_refresh_every=EVERY) if guided else {}
    return Trainer(m, g, 512, lr=1e-2, deterministic=True, seed=3, update_interval=16,
                   warmup_steps=16, images=u8, directions=dirs, poses=poses, img_wh=WH,
                   **LAMBDAS, **kw)


def _full_state(tr):
    st = _state(tr)
    st.update(emap=tr.guided.emap.clone(), acc_sum=tr.guided.acc_sum.clone(),
              acc_cnt=tr.guided.acc_cnt.clone(), w=tr.guided.w.clone(), cdf=tr.guided.cdf.clone())
    return st


def _run(tr, steps):
    out = []
    for _ in range(steps):
        terms = tr.step_sampled()
        out.append(torch.stack([terms[k] for k in sorted(terms)]).clone())
    return torch.stack(out)


def test_guided_training_repeats_and_resumes(cuda, tmp_path):
    data = _dataset(cuda)
    a = _trainer(cuda, data)
    assert a.guided.n_cells == 4 * 2 * 2 and a.guided.tile == 16
    la = _run(a, EVERY)
    # nothing refreshed yet: the map is flat, every weight 1, the errors recorded
    assert bool((a.guided.emap == 1).all()) and bool((a.last_batch["ray_weight"] == 1).all())
    assert int(a.guided.acc_cnt.sum()) == EVERY * 512
    la = torch.cat([la, _run(a, 1)])
    assert not bool((a.guided.emap == 1).any()) and int(a.guided.acc_cnt.sum()) == 512
    assert bool((a.last_batch["ray_weight"] != 1).any())
    assert float(a.last_batch["ray_weight"].max()) <= 2.0       # 1 / uniform_frac
    la = torch.cat([la, _run(a, STEPS - EVERY - 1)])
    sa = _full_state(a)
    assert a.global_step == STEPS and bool(torch.isfinite(la).all())
    # a second run, saved between two refreshes
    b = _trainer(cuda, data)
    lb = _run(b, CUT)
    assert int(b.guided.acc_cnt.sum()) == (CUT - EVERY) * 512
    path = str(tmp_path / "guided.pt")
    assert b.save_state(path).wait() == path
    sd = b.state_dict()
    lb = torch.cat([lb, _run(b, STEPS - CUT)])
    sb = _full_state(b)
    assert torch.equal(la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # resumed in a fresh trainer, from the file and from the dict
    for load in (lambda t: t.load_state(path), lambda t: t.load_state_dict(sd)):
        c = _trainer(cuda, data)
        load(c)
        assert c.global_step == CUT and int(c.guided.acc_cnt.sum()) == (CUT - EVERY) * 512
        lc = _run(c, STEPS - CUT)
        sc = _full_state(c)
        assert torch.equal(lc, la[CUT:])
        for k in sa:
            assert torch.equal(sa[k], sc[k]), k
    # the two kinds of state do not mix
    plain = _trainer(cuda, data, guided=False)
    with pytest.raises(ValueError, match="guided: saved True"):
        plain.load_state_dict(sd)
    assert plain.global_step == 0
    with pytest.raises(ValueError, match="guided"):
        _trainer(cuda, data).load_state_dict(plain.state_dict())
    # the unguided trainer draws what it drew before the option existed
    plain.step_sampled()
    i0, p0 = SR.picks(3, 0, 0, 512, 4, WH[0] * WH[1])
    assert np.array_equal(plain.last_batch["img_idxs"].cpu().numpy(), i0)
    assert np.array_equal(plain.last_batch["pix_idxs"].cpu().numpy(), p0)
    assert set(plain.last_batch) == set(sampler.KEYS)
