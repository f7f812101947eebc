"""GPU: the remaining §8 rows end to end.

  a11  single-NeRF `render()` with `NGP` (rendering.py:12-46, C1/C2): forward
       and backward vs the CPU oracle (ml_oracle with K = 1, where the gate's
       softmax over one model is exactly 1);
  a10  test-time rendering (ml_rendering.py:81-155): with exp_step_factor 0 the
       progressive-compaction loop must reproduce the training render with zero
       jitter (same samples, same early termination);
  §8f  density-grid maintenance (networks.py:375-409): the bitfield written by
       update_density_grid equals packbits(density_grid > min(mean, thr)) of
       the oracle on the updated grid, and the grid holds the field's σ at the
       jittered cell positions.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import field_oracle as fo
from oracle import ml_oracle
from oracle.ml_oracle import _split_field
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd.networks import MNGP, NGP
from radnerf_amd.rendering import ml_render, render
from parity import check_grads

pytestmark = pytest.mark.gpu


def _du_hash(seed, seg, i, st):
    """field_aux.hip du_hash (splitmix64 finaliser), numpy uint64"""
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
             + ((np.uint64(seg) << np.uint64(32)) | i.astype(np.uint64))
             + np.uint64(st) * np.uint64(0xD1B54A32D192ED03))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def _du_unit(h):
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _init(m, p=0.5):
    """a single NGP with the tables and occupancy of synthetic.parity_scene"""
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(1, LY.FIELD_PARAMS)))
    bits = S.bitfields(1, m.cascades, p=p)
    S.set_bitfields(m, bits)
    return bits


@pytest.mark.parametrize("fused", [True, False])
def test_ngp_render_train_vs_oracle(cuda, fused):
    """a11: render() training render of a single NGP, fused K = 1 chain (the
    default) and the op-by-op chain, vs the oracle: counts bit-exact, outputs
    <= 1e-4, per-level / per-layer gradient bars; the per-sample keys
    (rays_a, ts, deltas, ws, rm_samples, vr_samples) vs the oracle too."""
    scale, B = 0.5, 512
    m = NGP(scale, seed=3)
    bits = _init(m)
    m = m.to(cuda)
    o, d = S.rays(B, scale)
    nz = S.noise(1, B)
    d_rgb, d_op, d_depth = S.loss_seeds(B, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    res = render(m, t(o), t(d), noise=t(nz[0]), fused=fused)
    torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]],
                            [t(d_rgb), t(d_op), t(d_depth[:, 0])])
    for k in ("rays_a", "ws", "deltas", "ts", "rm_samples", "vr_samples"):
        assert k in res
    # every dict access path sees the lazy keys: get, iteration,
    # keys / items, len, dict(res)
    lazy = {"rays_a", "ws", "deltas", "ts", "rm_samples", "vr_samples"}
    assert res.get("ws") is not None and res.get("no such key", 7) == 7
    assert lazy <= set(res) and lazy <= set(res.keys()) and lazy <= {k for k, _ in res.items()}
    assert len(res) == len(list(res)) and lazy <= set(dict(res))
    n = int(res["rm_samples"])
    ra = res["rays_a"].cpu().numpy()
    assert ra.shape == (B, 3) and int(ra[:, 2].sum()) == n
    assert res["ts"].shape == (n,) and res["deltas"].shape == (n,) and res["ws"].shape == (n,)
    # per-ray segments: contiguous, in ray order, the weights of a ray sum to
    # its opacity
    assert np.array_equal(ra[:, 0], np.arange(B))
    ws_np = res["ws"].detach().cpu().numpy()
    op_np = res["opacity"].detach().cpu().numpy()
    seg = np.add.reduceat(ws_np, ra[:, 1]) if n else np.zeros(B)
    has = ra[:, 2] > 0
    assert np.allclose(seg[has], op_np[has], atol=1e-5)
    assert 0 < int(res["vr_samples"]) <= n
    gate_p = np.zeros(LY.gate_params(1), np.float32)    # softmax over one model = 1
    ref = ml_oracle.ml_train_step(o, d, bits, nz, m.xyz_encoder.params.detach().cpu().view(-1, 2),
                                  m.mlp_params.detach().cpu(), gate_p, scale,
                                  seeds=(d_rgb, d_op, d_depth))
    # bit-exact sample counts per ray
    assert np.array_equal(ra[:, 2], ref["counts"][0])
    e_rgb = np.abs(res["rgb"].detach().cpu().numpy() - ref["rgb"]).max()
    e_op = np.abs(res["opacity"].detach().cpu().numpy() - ref["opacity"]).max()
    e_de = np.abs(res["depth"].detach().cpu().numpy() - ref["depth"][:, 0]).max()
    assert e_rgb <= 1e-4 and e_op <= 1e-4 and e_de <= 1e-4, (e_rgb, e_op, e_de)
    check_grads(scale, m.xyz_encoder.params.grad.cpu().view(-1, 2).numpy(), ref["grid_grad"],
                m.mlp_params.grad.cpu().numpy(), ref["mlp_grad"], tag="NGP render")


@pytest.mark.parametrize("K", [1, 2])
def test_test_time_render_matches_train_without_jitter(cuda, K):
    scale, B = 0.5, 700
    sc = S.parity_scene(K, p=0.3, device=cuda)
    m, g = sc.m, sc.g
    o, d = (torch.from_numpy(a).to(cuda) for a in S.rays(B, scale))
    with torch.no_grad():
        tr = ml_render(m, g, o, d, d, noise=torch.zeros(K, B, device=cuda), fused=False)
        te = ml_render(m, g, o, d, d, test_time=True)
    for k in ("rgb", "opacity", "depth"):
        err = (tr[k].float() - te[k].float()).abs().max().item()
        assert err <= 1e-5, (k, err)


def _du_points(seed, seg, cells, c, scale, G):
    """the jittered point of each cell's first draw (field_aux.hip k_du_sample)"""
    sc = np.float32(min(2.0 ** (c - 1), scale))
    hgs = np.float32(sc / np.float32(G))
    xyz = oracle.morton3d_invert(cells.astype(np.int32)).astype(np.float32)
    di = cells.astype(np.uint32) << np.uint32(5)
    jit = np.stack([_du_unit(_du_hash(seed, seg, di, s_)) for s_ in (2, 3, 4)], 1)
    return ((xyz / np.float32(G - 1)) * np.float32(2) - np.float32(1)) * (sc - hgs) \
        + (jit * np.float32(2) - np.float32(1)) * hgs


def test_density_grid_update(cuda):
    """Warm-up update (networks.py:330-343 cells, :375-409): every cell of
    every cascade evaluated once at a jittered point; grid = max(grid * 0.95,
    sigma) with sigma the oracle's at the replayed point; the bitfield is
    packbits(grid > min(mean, thr)) in Morton byte order."""
    scale, K = 0.5, 2
    m = S.parity_scene(K, scale=scale, device=cuda).m
    thr = 0.01 * 1024 / 3 ** 0.5                      # train_ml.py:175
    with torch.no_grad():
        for i in range(K):
            getattr(m, f"density_grid_{i}").fill_(0.5)
    seed = 11
    m.update_density_grid(thr, warmup=True, seed=seed)
    torch.cuda.synchronize()
    G = m.grid_size
    lv = fo.grid_levels(scale)
    gp = m.xyz_encoder.params.detach().cpu().view(-1, 2).half().float()
    cells = np.arange(0, G ** 3, 997, dtype=np.uint32)
    for i in range(K):
        grid = getattr(m, f"density_grid_{i}").cpu().numpy()
        x = _du_points(seed, i * m.cascades + 0, cells, 0, scale, G)
        sig, _ = fo.density_forward(torch.from_numpy(x), gp, _split_field(m.mlp_params.detach().cpu()[i]),
                                    lv, m.xyz_min.cpu(), m.xyz_max.cpu())
        sig = sig.detach().numpy()
        got = grid[0, cells]
        want = np.maximum(np.float32(0.5) * np.float32(0.95), sig)
        e = np.abs(got - want) / (1e-2 + np.abs(want))
        assert e.max() <= 1e-4, e.max()
        dg = getattr(m, f"density_grid_{i}")
        mean = dg[dg > 0].mean().item()
        bits = oracle.packbits(grid.reshape(-1), min(float(mean), thr))
        assert np.array_equal(getattr(m, f"density_bitfield_{i}").cpu().numpy(), bits)


@pytest.mark.parametrize("scale,K,inside", [(0.5, 2, False), (16.0, 2, False), (16.0, 4, False),
                                            (0.5, 2, True), (16.0, 2, True)])
def test_test_time_render_vs_oracle(cuda, scale, K, inside):
    """a10: ml_render(test_time=True) -- raymarching_test with the cascades
    quirk of calc_dt (raymarching.cu:370,399), the host compaction loop of
    ml_rendering.py:81-155, composite_test_fw -- vs the oracle's restatement of
    the same loop; at scale 16 (exp step 1/256, 6 cascades) it differs from the
    training march, so it is checked against the oracle directly."""
    B = 600
    sc = S.parity_scene(K, scale=scale, p=0.3, device=cuda)
    m, g, bits = sc.m, sc.g, sc.bits
    o, d = S.rays(B, scale)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    esf = 1 / 256 if scale > 0.5 else 0.0
    if inside:
        # cameras inside the scene box (360 / free scenes): the AABB entry is
        # behind the origin, t1 < 0, and the test march starts there
        o = (np.random.default_rng(5).uniform(-0.3, 0.3, (B, 3)) * min(scale, 1.0)).astype(np.float32)
    with torch.no_grad():
        te = ml_render(m, g, t(o), t(d), t(d), test_time=True, exp_step_factor=esf)
        lp = ml_render(m, g, t(o), t(d), t(d), test_time=True, exp_step_factor=esf, fused=False)
    ref = ml_oracle.ml_render_test(o, d, bits, m.xyz_encoder.params.detach().cpu().view(-1, 2),
                                   m.mlp_params.detach().cpu(), g.params.detach().cpu(), scale)
    for name, res in (("fused", te), ("loop", lp)):
        errs = {k: float(np.abs(res[k].float().cpu().numpy() - ref[k]).max())
                for k in ("rgb", "opacity", "depth")}
        print(f"test-time render ({name}) scale {scale} K {K} inside {inside}: {errs}, "
              f"opacity mean {ref['opacity'].mean():.3f}")
        assert all(v <= 1e-4 for v in errs.values()), errs
    # rn_render_test vs the host loop (vren.raymarching_test + field +
    # composite_test_fw rounds): the same samples, T restarted from the opacity
    # every 32 samples instead of every round
    # (depth at scale 16 is ~35: a few ulps relative)
    for k in ("rgb", "opacity", "depth"):
        assert torch.allclose(te[k], lp[k], rtol=2e-6, atol=1e-5), k


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_image_gate(cuda, scale):
    """gate_type=image (ml_rendering.py:31-36): the gate sees cat(rays_o,
    imgs_d); fused and drop-in chains vs the oracle, outputs and gradients."""
    from radnerf_amd.fused import ml_render_fused
    dropin = functools.partial(ml_render, fused=False)
    B, K = 384, 2
    esf = 1 / 256 if scale > 0.5 else 0.0
    sc = S.parity_scene(K, B, scale=scale, gate_type="image", device=cuda)
    m, g, o, d, noise, seeds, bits = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bits
    imgs_d = S.rays(B, scale, seed=77)[1]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    outs = []
    for fn in (ml_render_fused, dropin):
        m.zero_grad(); g.zero_grad()
        res = fn(m, g, to(o), to(d), to(imgs_d), noise=to(noise), exp_step_factor=esf)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], [to(s) for s in seeds])
        outs.append((res, g.params.grad.clone()))
    ref = ml_oracle.ml_train_step(o, d, bits, noise, m.xyz_encoder.params.detach().cpu().view(-1, 2),
                                  m.mlp_params.detach().cpu(), g.params.detach().cpu(), scale,
                                  seeds=seeds, gate_in2=imgs_d)
    for res, gg in outs:
        assert np.abs(res["gating_code"].detach().cpu().numpy() - ref["gate"]).max() <= 1e-5
        assert np.abs(res["rgb"].detach().cpu().numpy() - ref["rgb"]).max() <= 1e-4
        e = float(np.linalg.norm(gg.cpu().numpy() - ref["gate_grad"]) / np.linalg.norm(ref["gate_grad"]))
        assert e <= 2e-3, e
    # the image gate differs from the ray gate on these inputs
    assert np.abs(ref["gate"] - ml_oracle.ml_train_step(
        o, d, bits, noise, m.xyz_encoder.params.detach().cpu().view(-1, 2),
        m.mlp_params.detach().cpu(), g.params.detach().cpu(), scale)["gate"]).max() > 1e-3


@pytest.mark.parametrize("scale,K", [(0.5, 2), (16.0, 3)])
def test_density_update_sampled_device(cuda, scale, K):
    """rn_density_update_sampled (networks.py:345-409, warmup False, all
    sub-NeRFs and cascades in one call): per (sub-NeRF, cascade) M = G^3/4
    uniform cells and M cells among the occupied ones.  Coverage of the draws
    per segment (sigma > 0 everywhere, so a sampled cell has tmp > 0): free
    cells 1 - e^-1/4, occupied cells 1 - e^-3/4; a segment without occupied
    cells gets only the uniform draws.  Decay / max, negative cells untouched,
    packbits at min(mean of the positive cells, thr); the same seed gives
    identical grids and bitfields, another seed other cells."""
    m = MNGP(scale, size=K, seed=3).to(cuda)
    C, G3 = m.cascades, m.grid_size ** 3
    thr = 0.01 * 1024 / 3 ** 0.5
    gen = torch.Generator(device=cuda)
    gen.manual_seed(1)
    occ_mask = torch.rand(K, C, G3, generator=gen, device=cuda) < 0.5
    occ_mask[0, 0] = False                       # one segment without occupied cells
    old = torch.where(occ_mask, 2 * thr, 0.0)
    old[:, :, :1000] = -1.0                      # cells the update must leave alone
    outs, tmps = [], []
    for seed in (77, 77, 78):
        with torch.no_grad():
            for i in range(K):
                getattr(m, f"density_grid_{i}").copy_(old[i])
        du = m.update_density_grid(thr, warmup=False, seed=seed)
        torch.cuda.synchronize()
        tmps.append(du["tmp"].view(K, C, G3).clone())
        outs.append([getattr(m, f"density_grid_{i}").clone() for i in range(K)] +
                    [getattr(m, f"density_bitfield_{i}").clone() for i in range(K)])
        thr_dev = du["thr"].cpu().numpy()
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert not torch.equal(tmps[0], tmps[2])
    tmp = tmps[2]
    hit = tmp > 0
    e_u, e_uo = 1 - np.exp(-0.25), 1 - np.exp(-0.75)
    for k in range(K):
        for c in range(C):
            h, o = hit[k, c], occ_mask[k, c]
            f_free = float(h[~o].float().mean())
            assert abs(f_free - e_u) < 0.01, (k, c, f_free)
            if o.any():
                f_occ = float(h[o].float().mean())
                assert abs(f_occ - e_uo) < 0.01, (k, c, f_occ)
    for k in range(K):
        new = getattr(m, f"density_grid_{k}")
        o = old[k]
        assert torch.equal(new[o < 0], o[o < 0])
        assert torch.equal(new[o >= 0], torch.maximum(o[o >= 0] * 0.95, tmp[k][o >= 0]))
        g = new.double().cpu().numpy()
        mean = g[g > 0].mean()
        assert abs(thr_dev[k] - min(mean, thr)) <= 1e-5 * min(mean, thr), (thr_dev[k], mean)
        bits = oracle.packbits(new.cpu().numpy().reshape(-1), float(thr_dev[k]))
        assert np.array_equal(getattr(m, f"density_bitfield_{k}").cpu().numpy(), bits)


@pytest.mark.parametrize("scale,K", [(0.5, 2), (16.0, 2)])
def test_density_update_keeps_one_draw_and_its_sigma(cuda, scale, K):
    """VERDICT r03 item 2.  The reference's index_put keeps ONE draw per cell
    (networks.py:394).  The device update decides per cell whether it is
    drawn (uniform M / G^3 or, when occupied, M / n_occupied, Poisson limit)
    and evaluates sigma once, at its first draw's jitter.  Replaying the
    counter-based draws on the CPU: the drawn cells are exactly the cells
    with tmp > 0 (up to a float exp() rounding at the threshold), and
    tmp[cell] equals the oracle's sigma at the replayed jittered point."""
    m = MNGP(scale, size=K, seed=3).to(cuda)
    C, G = m.cascades, m.grid_size
    G3 = G ** 3
    M = G3 // 4
    thr = 0.01 * 1024 / 3 ** 0.5
    gen = torch.Generator(device=cuda)
    gen.manual_seed(5)
    occ = torch.rand(K, C, G3, generator=gen, device=cuda) < 0.3
    with torch.no_grad():
        for i in range(K):
            getattr(m, f"density_grid_{i}").copy_(torch.where(occ[i], 2 * thr, 0.0))
    seed = 12345
    du = m.update_density_grid(thr, warmup=False, seed=seed)
    torch.cuda.synchronize()
    tmp = du["tmp"].view(K, C, G3).cpu().numpy()
    occ = occ.cpu().numpy()
    gp = m.xyz_encoder.params.detach().cpu().view(-1, 2).half().float()
    lv = fo.grid_levels(scale)
    rng = np.random.default_rng(0)
    cells = np.arange(G3, dtype=np.uint32)
    e_max, n_chk, n_edge = 0.0, 0, 0
    for k in range(K):
        mlp = _split_field(m.mlp_params.detach().cpu()[k])
        for c in range(C):
            seg = k * C + c
            n_o = int(occ[k, c].sum())
            lam_o = np.float32(M) / np.float32(n_o) if n_o else np.float32(0)
            u0 = _du_unit(_du_hash(seed, seg, cells, 0))
            u1 = _du_unit(_du_hash(seed, seg, cells, 1))
            t0, t1 = np.exp(np.float32(-0.25)), np.exp(-lam_o)
            drawn = (u0 >= t0) | (occ[k, c] & (u1 >= t1) & (lam_o > 0))
            got = tmp[k, c] > 0
            diff = np.flatnonzero(drawn != got)
            # only a draw on the exp() threshold may differ (device expf vs numpy)
            edge = (np.abs(u0[diff] - t0) < 1e-6) | (np.abs(u1[diff] - t1) < 1e-6)
            assert edge.all(), (k, c, diff[~edge][:10])
            n_edge += len(diff)
            # sigma at the replayed jitter of a sample of the drawn cells
            pick = rng.choice(np.flatnonzero(drawn & got), 1500, replace=False)
            pos = _du_points(seed, seg, pick, c, scale, G)
            osig, _ = fo.density_forward(torch.from_numpy(pos.astype(np.float32)), gp, mlp, lv,
                                         m.xyz_min.cpu(), m.xyz_max.cpu())
            osig = osig.detach().numpy()
            e = np.abs(tmp[k, c][pick] - osig) / (1e-2 + np.abs(osig))
            e_max = max(e_max, float(e.max()))
            n_chk += len(pick)
    print(f"density update scale {scale}: {n_chk} drawn cells, sigma rel {e_max:.2e}, "
          f"{n_edge} threshold-edge draws")
    assert e_max <= 1e-4


def _ngp_setup(cuda, B, scale=0.5, p=0.5):
    m = NGP(scale, seed=3)
    bits = _init(m, p=p)
    m = m.to(cuda)
    o, d = S.rays(B, scale)
    return m, bits, o, d


def test_ngp_render_fused_full_size(cuda):
    """render() at C2's batch (8192 rays): the fused K = 1 chain vs the
    op-by-op chain on the same jitter -- outputs <= 1e-5, per-sample keys
    bit-identical (same march), gradients <= 1e-3 rel; count conservation."""
    B = 8192
    m, _, o, d = _ngp_setup(cuda, B)
    nz = torch.from_numpy(S.noise(1, B)[0]).to(cuda)
    seeds = [torch.from_numpy(np.ascontiguousarray(s)).to(cuda) for s in S.loss_seeds(B, 1)]
    outs = []
    for fused in (True, False):
        m.zero_grad()
        res = render(m, torch.from_numpy(o).to(cuda), torch.from_numpy(d).to(cuda), noise=nz,
                     fused=fused)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]],
                                [seeds[0], seeds[1], seeds[2][:, 0]])
        keys = {k: res[k].detach().clone() for k in ("rays_a", "ts", "deltas", "ws", "rm_samples")}
        outs.append((res, keys, m.xyz_encoder.params.grad.clone(), m.mlp_params.grad.clone()))
    (rf, kf, gf, mf), (rd, kd, gd, md) = outs
    for k in ("rgb", "opacity", "depth"):
        assert (rf[k].detach() - rd[k].detach()).abs().max().item() <= 1e-5, k
    for k in ("rays_a", "ts", "deltas", "rm_samples"):
        assert torch.equal(kf[k], kd[k]), k
    assert (kf["ws"] - kd["ws"]).abs().max().item() <= 1e-5
    assert int(kf["rays_a"][:, 2].sum()) == int(kf["rm_samples"]) > 0
    for a, b in ((gf, gd), (mf, md)):
        e = ((a - b).norm() / b.norm()).item()
        assert e <= 1e-3, e


def test_ngp_render_test_time_vs_oracle(cuda):
    """a10 + a11: render(test_time=True) of a single NGP (rn_render_test, and
    the host loop with fused=False) vs the oracle's compaction loop (K = 1)."""
    B, scale = 600, 0.5
    m, bits, o, d = _ngp_setup(cuda, B, p=0.3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    with torch.no_grad():
        te = render(m, t(o), t(d), test_time=True)
        lp = render(m, t(o), t(d), test_time=True, fused=False)
    gate_p = np.zeros(LY.gate_params(1), np.float32)
    ref = ml_oracle.ml_render_test(o, d, bits, m.xyz_encoder.params.detach().cpu().view(-1, 2),
                                   m.mlp_params.detach().cpu(), gate_p, scale)
    for name, res in (("fused", te), ("loop", lp)):
        errs = {"rgb": float(np.abs(res["rgb"].float().cpu().numpy() - ref["rgb"]).max()),
                "opacity": float(np.abs(res["opacity"].float().cpu().numpy() - ref["opacity"]).max()),
                "depth": float(np.abs(res["depth"].float().cpu().numpy().reshape(-1)
                                      - np.asarray(ref["depth"]).reshape(-1)).max())}
        assert all(v <= 1e-4 for v in errs.values()), (name, errs)
    assert int(te["total_samples"]) > 0


def test_fused_outputs_without_gradient_raise(cuda):
    """independent_rgbs (ml_render) and ws (render) come out of the fused
    chain as values; a loss on them raises at backward instead of silently
    getting no gradient (fused=False differentiates them)."""
    from radnerf_amd.fused import ml_render_fused
    B, K = 256, 2
    sc = S.parity_scene(K, B, scale=0.5, device=cuda)
    m, g, o, d, noise, seeds, bits = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bits
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    res = ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise))
    assert res["independent_rgbs"][0].requires_grad
    with pytest.raises(RuntimeError, match="independent_rgbs"):
        res["independent_rgbs"][1].sum().backward()
    # the combined outputs still differentiate
    res = ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise))
    res["rgb"].sum().backward()
    assert m.mlp_params.grad is not None
    # render()'s ws
    mn, _, on, dn = _ngp_setup(cuda, B)
    r1 = render(mn, to(on), to(dn))
    with pytest.raises(RuntimeError, match="ws"):
        r1["ws"].sum().backward()
    # a second forward through the same workspace makes the lazy keys stale
    r2 = render(mn, to(on), to(dn))
    with pytest.raises(RuntimeError, match="reused"):
        _ = r1["ts"]
    assert r2["ts"].numel() == int(r2["rm_samples"])


def test_ngp_sampled_density_update_through_dist(cuda):
    """radnerf_amd.dist.update_density_grid on a single NGP with
    warmup=False passes the step's seed through NGP.update_density_grid
    (its override once dropped the keyword: TypeError) to the device-side
    sampled update; the same (seed, step) gives the same grid and bitfield."""
    from radnerf_amd import dist as rdist
    m, _, _, _ = _ngp_setup(cuda, 64)
    thr = 0.01 * 1024 / 3 ** 0.5
    rdist.update_density_grid(m, thr, 0, warmup=True)
    g0 = m.density_grid.clone()
    outs = []
    for _ in range(2):
        with torch.no_grad():
            m.density_grid_0.copy_(g0)
        rdist.update_density_grid(m, thr, 5, warmup=False, seed=3)
        torch.cuda.synchronize()
        outs.append((m.density_grid.clone(), m.density_bitfield.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], g0)
