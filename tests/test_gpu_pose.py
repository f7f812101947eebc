"""GPU: camera pose refinement (--optimize_ext, train_ml.py:90-93, 129-146;
ray_utils.py:73-100) -- rn_get_rays_pose / rn_get_rays_pose_bw, rays.pose_rays,
FusedMLRenderer.train_step(input_grad=True) and Trainer.step_pixels.

The reference is the Rodrigues formula and get_rays restated in torch below
(`_pose_chain`), evaluated in fp64 on the CPU with autograd for the kernel
tests and in fp32 on the device for the chain test.
"""
import pytest
import torch

from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from radnerf_amd.fused import get_renderer, ml_render_fused
from radnerf_amd.losses import NeRFLoss
from radnerf_amd.rays import batch_rays, pose_rays, pose_rays_backward
from radnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

LAMBDAS = dict(lambda_opacity=1e-3, lambda_cv_importance=1e-2, lambda_depth_mutual=5e-2)
MAGS = (0.0, 1e-6, 1e-4, 1e-2, 0.3, 2.5)


def _axisangle_to_R(v):
    """ray_utils.py:73-100"""
    zero = torch.zeros_like(v[:, :1])
    k0 = torch.cat([zero, -v[:, 2:3], v[:, 1:2]], 1)
    k1 = torch.cat([v[:, 2:3], zero, -v[:, 0:1]], 1)
    k2 = torch.cat([-v[:, 1:2], v[:, 0:1], zero], 1)
    K = torch.stack([k0, k1, k2], dim=1)
    n = (torch.norm(v, dim=1) + 1e-7)[:, None, None]
    eye = torch.eye(3, device=v.device, dtype=v.dtype)
    return eye + (torch.sin(n) / n) * K + ((1 - torch.cos(n)) / n ** 2) * (K @ K)


def _pose_chain(dirs, poses, dR, dT, img, pix):
    """train_ml.py:84-96 with optimize_ext: rays_o, rays_d, imgs_d."""
    P = poses[img]
    R = _axisangle_to_R(dR[img]) @ P[..., :3]
    T = P[..., 3] + dT[img]
    rays_d = (dirs[pix][:, None, :] @ R.transpose(1, 2))[:, 0]
    mean = dirs.mean(0)[None, None, :].expand(img.shape[0], 1, 3)
    imgs_d = (mean @ R.transpose(1, 2))[:, 0]
    return T, rays_d, imgs_d


def _rel_max(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------ 1. kernels
@pytest.fixture(scope="module", params=[193, 700])
def kcase(request, cuda):
    """N = 6 images; image 4 holds more than a wave's (193) / more than a
    block's (700: a thread then sums several rays) picks, image 5 none.  193
    and 700 are no multiples of 64 or 256.  Everything is computed once."""
    B, N, P = request.param, 6, 40 * 50
    g = torch.Generator().manual_seed(11)
    dirs = torch.stack([torch.rand(P, generator=g) - 0.5, torch.rand(P, generator=g) - 0.5,
                        torch.ones(P)], -1)
    q, _ = torch.linalg.qr(torch.randn(N, 3, 3, generator=g))
    poses = torch.cat([q, torch.randn(N, 3, 1, generator=g)], 2).contiguous()
    ax = torch.randn(N, 3, generator=g)
    dR = (ax / ax.norm(dim=1, keepdim=True) * torch.tensor(MAGS)[:, None]).contiguous()
    dT = (0.1 * torch.randn(N, 3, generator=g)).contiguous()
    n4 = 100 if B == 193 else 400
    rest = torch.cat([torch.arange(4), torch.randint(4, (B - n4 - 4,), generator=g)])
    img = torch.cat([torch.full((n4,), 4), rest])[torch.randperm(B, generator=g)].contiguous()
    pix = torch.randint(P, (B,), generator=g)
    assert int((img == 4).sum()) == n4 and int((img == 5).sum()) == 0
    assert all(int((img == i).sum()) >= 1 for i in range(4))
    seeds = [torch.randn(B, 3, generator=g) for _ in range(3)]

    # fp64 reference, autograd of the reference formula
    def ref(with_i):
        r64, t64 = dR.double().requires_grad_(True), dT.double().requires_grad_(True)
        out = _pose_chain(dirs.double(), poses.double(), r64, t64, img, pix)
        loss = sum((o * s.double()).sum() for o, s in zip(out[:3 if with_i else 2], seeds))
        loss.backward()
        return [o.detach() for o in out], r64.grad, t64.grad

    outs64, gR64, gT64 = ref(True)
    _, gR64_noi, gT64_noi = ref(False)

    c = lambda t: t.to(cuda).contiguous()
    d = dict(dirs=c(dirs), poses=c(poses), dR=c(dR), dT=c(dT), img=c(img), pix=c(pix),
             seeds=[c(s) for s in seeds])
    d["mean"] = d["dirs"].mean(0).contiguous()
    st = torch.cuda.current_stream(cuda).cuda_stream

    def fw(dR_, dT_):
        o = [torch.full((B, 3), float("nan"), device=cuda) for _ in range(3)]
        lib().get_rays_pose(d["dirs"].data_ptr(), d["poses"].data_ptr(),
                            None if dR_ is None else dR_.data_ptr(),
                            None if dT_ is None else dT_.data_ptr(), d["img"].data_ptr(),
                            d["pix"].data_ptr(), B, d["mean"].data_ptr(), o[0].data_ptr(),
                            o[1].data_ptr(), o[2].data_ptr(), st)
        return o

    def bw(with_i=True):
        # NaN-prefilled: the kernel must write every row and accumulate nothing
        oR = torch.full((N, 3), float("nan"), device=cuda)
        oT = torch.full((N, 3), float("nan"), device=cuda)
        pose_rays_backward(d["dirs"], d["poses"], d["dR"], d["img"], d["pix"], d["mean"],
                           d["seeds"][0], d["seeds"][1], d["seeds"][2] if with_i else None,
                           oR, oT)
        return oR, oT

    d.update(B=B, N=N, cpu=dict(dirs=dirs, poses=poses, dR=dR, dT=dT, img=img, pix=pix),
             outs64=outs64, gR64=gR64, gT64=gT64, gR64_noi=gR64_noi, gT64_noi=gT64_noi,
             out=fw(d["dR"], d["dT"]), out_zero=fw(torch.zeros_like(d["dR"]),
                                                   torch.zeros_like(d["dT"])),
             out_null=fw(None, None), base=batch_rays(d["dirs"], d["poses"], d["img"], d["pix"]),
             g1=bw(), g2=bw(), g_noi=bw(False))
    torch.cuda.synchronize()
    return d


def test_forward_vs_fp64(kcase):
    ro, rd, imd = kcase["out"]
    ro64, rd64, imd64 = kcase["outs64"]
    e_d = float((rd.cpu().double() - rd64).abs().max())
    e_i = float((imd.cpu().double() - imd64).abs().max())
    print(f"pose forward B={kcase['B']}: rays_d L_inf {e_d:.3e}, imgs_d L_inf {e_i:.3e}")
    assert torch.allclose(rd.cpu().double(), rd64, atol=1e-6, rtol=0)
    assert torch.allclose(imd.cpu().double(), imd64, atol=1e-6, rtol=0)
    # rays_o is the fp32 sum T0 + t, exactly
    c = kcase["cpu"]
    assert torch.equal(ro.cpu(), (c["poses"][..., 3] + c["dT"])[c["img"]])


def test_zero_refinement_reproduces_batch_rays(kcase):
    bit = True
    for name, a, z, b in zip(("rays_o", "rays_d", "imgs_d"), kcase["out_null"],
                             kcase["out_zero"], kcase["base"]):
        assert torch.allclose(z, b, atol=1e-6, rtol=0), name
        assert torch.allclose(a, b, atol=1e-6, rtol=0), name
        bit = bit and torch.equal(z, b) and torch.equal(a, b)
    print(f"pose forward B={kcase['B']}: zero dR / dT bit-equal to batch_rays: {bit}")


def test_backward_vs_fp64_autograd(kcase):
    gR, gT = kcase["g1"]
    eR, eT = _rel_max(gR, kcase["gR64"]), _rel_max(gT, kcase["gT64"])
    print(f"pose backward B={kcase['B']}: max|a-b|/max|b| dR {eR:.3e}, dT {eT:.3e}")
    assert eR <= 1e-5 and eT <= 1e-5, (eR, eT)
    # without dL/dimgs_d (NULL together with mean_dir)
    gR, gT = kcase["g_noi"]
    eR, eT = _rel_max(gR, kcase["gR64_noi"]), _rel_max(gT, kcase["gT64_noi"])
    assert eR <= 1e-5 and eT <= 1e-5, (eR, eT)


def test_backward_writes_every_row_and_is_deterministic(kcase):
    (gR, gT), (gR2, gT2) = kcase["g1"], kcase["g2"]
    assert torch.isfinite(gR).all() and torch.isfinite(gT).all()
    assert torch.equal(gR[5], torch.zeros(3, device=gR.device))
    assert torch.equal(gT[5], torch.zeros(3, device=gR.device))
    assert torch.equal(gR, gR2) and torch.equal(gT, gT2)
    # the rotation gradient at |v| = 0 (image 0) is the a <M, E_k> term alone: non-zero
    assert float(gR[0].abs().max()) > 0


def test_empty_batch_zeroes_the_rows(cuda):
    N = 3
    z = torch.zeros(0, 3, device=cuda)
    i = torch.zeros(0, dtype=torch.int64, device=cuda)
    oR = torch.full((N, 3), float("nan"), device=cuda)
    oT = torch.full((N, 3), float("nan"), device=cuda)
    pose_rays_backward(torch.zeros(4, 3, device=cuda), torch.zeros(N, 3, 4, device=cuda), None,
                       i, i, None, z, z, None, oR, oT)
    assert float(oR.abs().max()) == 0 and float(oT.abs().max()) == 0


# ----------------------------------------------------------- 2. through autograd
def test_pose_rays_autograd(kcase, cuda):
    leaf = lambda t: t.clone().requires_grad_(True)
    dirs, poses, dR, dT = (leaf(kcase[k]) for k in ("dirs", "poses", "dR", "dT"))
    out = pose_rays(dirs, poses, dR, dT, kcase["img"], kcase["pix"])
    for a, b in zip(out, kcase["out"]):
        assert torch.equal(a, b)
    torch.autograd.backward(list(out), kcase["seeds"])
    assert torch.equal(dR.grad, kcase["g1"][0]) and torch.equal(dT.grad, kcase["g1"][1])
    assert dirs.grad is None and poses.grad is None
    # two outputs, one of them unused: dL/dimgs_d absent, dL/drays_o zero
    dR2, dT2 = leaf(kcase["dR"]), leaf(kcase["dT"])
    ro, rd = pose_rays(dirs, poses, dR2, dT2, kcase["img"], kcase["pix"], with_imgs_d=False)
    (rd * kcase["seeds"][1]).sum().backward()
    assert float(dT2.grad.abs().max()) == 0
    assert torch.isfinite(dR2.grad).all() and float(dR2.grad.abs().max()) > 0


# ------------------------------------------------------------------- 3. chain
@pytest.mark.parametrize("gate_type", ["ray", "image"])
def test_train_step_pose_gradients_match_autograd(cuda, gate_type):
    """The two chains form their rays with different roundings (measured
    1e-7 apart), and the render is not smooth in the rays at that scale: f16
    roundings and ReLU masks in the field flip, samples cross occupancy
    boundaries.  How far that alone moves the reference was measured as the
    reference against itself -- the torch pose chain + autograd through
    ml_render_fused on its own rays vs on pose_rays' rays (rel. L2 of the dR /
    dT gradients, "ray" gate; the "image" gate is alike):
        hash table U(-0.1, 0.1) (the other tests'), occupancy 0.5:  1.0e-2 / 9.9e-3
        the same table, every cell occupied:                        5.9e-3 / 7.4e-3
        the module's own table init, occupancy 0.5:                 9.2e-5 / 4.9e-4
        the module's own table init, every cell occupied:           2.8e-5 / 2.6e-4
    The test runs the last setting, where the reference's own scatter is a
    quarter of the bar, so the bar measures the gradient chain.  Two tighter
    statements hold in every setting: on identical rays the step's ray
    gradients are autograd's (asserted below), and the pose backward is within
    1e-5 of fp64 (test 1)."""
    B, K, N = 256, 2, 5
    sc = S.parity_scene(K, p=1.0, gate_type=gate_type, rough_grid=False, device=cuda)
    m, g = sc.m, sc.g
    dirs, poses = (t.to(cuda) for t in S.ring_cameras(N, 24))
    gen = torch.Generator().manual_seed(7)
    dR0 = (0.02 * torch.randn(N, 3, generator=gen)).to(cuda)
    dT0 = (0.02 * torch.randn(N, 3, generator=gen)).to(cuda)
    img = torch.randint(N, (B,), generator=gen).to(cuda)
    pix = torch.randint(dirs.shape[0], (B,), generator=gen).to(cuda)
    tgt = torch.rand(B, 3, generator=gen).to(cuda)
    nz = torch.from_numpy(S.noise(K, B)).to(cuda)
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))

    # reference: the torch pose chain -> ml_render_fused (autograd) -> NeRFLoss
    dR, dT = dR0.clone().requires_grad_(True), dT0.clone().requires_grad_(True)
    m.zero_grad(); g.zero_grad()
    ro, rd, imd = _pose_chain(dirs, poses, dR, dT, img, pix)
    res = ml_render_fused(m, g, ro, rd, imd, noise=nz)
    ld = NeRFLoss()(res, {"rgb": tgt}, **LAMBDAS)
    sum(v.mean() for v in ld.values()).backward()
    assert float(dR.grad.abs().max()) > 0 and float(dT.grad.abs().max()) > 0

    # fused: pose_rays -> train_step(input_grad=True) -> pose backward
    r = get_renderer(m, g, B)
    bg = torch.ones(3, device=cuda)
    mean = dirs.mean(0).contiguous()
    with torch.no_grad():
        fo, fd, fi = pose_rays(dirs, poses, dR0, dT0, img, pix, mean_dir=mean)
    second = fi if gate_type == "image" else fd
    out = r.train_step(fo, fd, second, tgt, nz, bg, input_grad=True, **LAMBDAS)
    assert len(out) == 3
    terms, grads, (g_o, g_d, g_2) = out
    if gate_type == "image":
        g_i = g_2.contiguous()
    else:
        g_d, g_i = g_d + g_2, None
    oR, oT = torch.empty_like(dR0), torch.empty_like(dT0)
    pose_rays_backward(dirs, poses, dR0, img, pix, mean, g_o, g_d, g_i, oR, oT)
    eR, eT = rel(oR, dR.grad), rel(oT, dT.grad)
    print(f"chain ({gate_type} gate): rel L2 dR {eR:.3e}, dT {eT:.3e}")
    assert eR <= 1e-3 and eT <= 1e-3, (eR, eT)
    for k in ld:
        want = float(ld[k].mean().detach())
        assert abs(float(terms[k]) - want) <= 1e-5 * max(1.0, abs(want)), k
    # identical rays: the ray gradients of the step are those of autograd.  The
    # same kernels run on both sides; only the loss seeds come from two
    # implementations (rn_nerf_loss vs torch ops) and differ by fp32 roundings
    # (6e-8), which flip an f16 operand rounding (2^-11) once in ~2^13
    # elements: ~5e-6 rel. L2 expected, 1e-4 allowed.
    g_o, g_d = g_o.clone(), g_d.clone()         # g_d may be a view of the workspace
    ao, ad, ai = (t.clone().requires_grad_(True) for t in (fo, fd, fi))
    res = ml_render_fused(m, g, ao, ad, ai, noise=nz)
    sum(v.mean() for v in NeRFLoss()(res, {"rgb": tgt}, **LAMBDAS).values()).backward()
    same = [rel(g_o, ao.grad), rel(g_d, ad.grad)]
    if gate_type == "image":
        same.append(rel(g_i, ai.grad))
    print(f"chain ({gate_type} gate): identical rays, step vs autograd rel L2 "
          + ", ".join(f"{e:.2e}" for e in same))
    assert max(same) <= 1e-4, same

    # the default step: same loss terms, same parameter gradients, two items
    plain = r.train_step(fo, fd, second, tgt, nz, bg, **LAMBDAS)
    assert len(plain) == 2
    terms0, grads0 = plain
    assert set(terms0) == set(terms)
    for k in terms0:
        a, b = float(terms0[k]), float(terms[k])
        if k == "cv_importance":
            # the gate's importance is summed over blocks with fp32 atomics
            # (k_gate_fwd), so CV^2 -- a variance of nearly equal sums --
            # differs between any two forwards of the same inputs (measured
            # 2.12420e-5 vs 2.12421e-5, 1.7e-6 apart).  Worst case for 256
            # adds into sums of ~128: 256 half-ulps = 2e-3 on a difference of
            # the two sums of ~8, squared: 5e-4 relative; 1e-3 allowed
            assert abs(a - b) <= 1e-3 * abs(b), (k, a, b)
        else:
            assert a == b, (k, a, b)
    for a, b in zip(grads, grads0):
        assert rel(a, b) <= 1e-3, rel(a, b)
    assert r.input_grad is False


# ----------------------------------------------------------------- 4. Trainer
@pytest.mark.parametrize("gate_type", ["ray", "image"])
def test_trainer_step_pixels(cuda, gate_type):
    B, K, N, lr = 256, 2, 6, 1e-3
    sc = S.parity_scene(K, gate_type=gate_type, device=cuda)
    m, g = sc.m, sc.g
    dirs, poses = S.ring_cameras(N, 24)
    gen = torch.Generator().manual_seed(8)
    img = torch.randint(4, (B,), generator=gen)            # images 4 and 5: no pick
    pix = torch.randint(dirs.shape[0], (B,), generator=gen)
    tgt = torch.rand(B, 3, generator=gen).to(cuda)
    tr = Trainer(m, g, B, lambda_cv_importance=1e-2, directions=dirs, poses=poses,
                 optimize_ext=True, pose_lr=lr)
    assert tr.dR.shape == (N, 3) and tr.dT.shape == (N, 3)
    assert isinstance(tr.dR, torch.nn.Parameter) and tr.dR.dtype == torch.float32
    assert float(tr.dR.detach().abs().max()) == 0 and float(tr.dT.detach().abs().max()) == 0
    assert [pg["lr"] for pg in tr.opt.param_groups] == [1e-2, lr]
    before = [p.detach().clone() for p in (m.xyz_encoder.params, m.mlp_params, g.params)]
    terms = tr.step_pixels(img.to(cuda), pix.to(cuda), tgt)
    assert torch.isfinite(terms["rgb"])
    for p in (tr.dR, tr.dT):
        assert torch.isfinite(p).all()
        assert float(p.detach().abs().max()) <= lr * (1 + 1e-3)      # Adam's first step
        assert float(p.detach()[:4].abs().max()) > 0
        assert float(p.detach()[4:].abs().max()) == 0                # absent images
    for p, b in zip((m.xyz_encoder.params, m.mlp_params, g.params), before):
        assert not torch.equal(p.detach(), b)
    # the flat buffer: [grid, MLP, gate, dR, dT]
    flat = tr.grads.flat
    assert flat.numel() == sum(b.numel() for b in before) + 6 * N
    assert torch.equal(flat[-6 * N:], torch.cat([tr.dR.grad.view(-1), tr.dT.grad.view(-1)]))
    assert float(flat[-6 * N:-3 * N].abs().max()) > 0 and float(flat[-3 * N:].abs().max()) > 0
    assert float(tr.dR.grad[4:].abs().max()) == 0 and float(tr.dT.grad[4:].abs().max()) == 0
    # finished rays still train (the pose gradients of such a step are zero)
    o, d = (torch.from_numpy(a).to(cuda) for a in S.rays(B, 0.5))
    tr.step(o, d, d, tgt)
    assert float(flat[-6 * N:].abs().max()) == 0


def test_trainer_without_pose_arguments_is_unchanged(cuda):
    B, K = 256, 2
    sc = S.parity_scene(K, device=cuda)
    m, g = sc.m, sc.g
    tr = Trainer(m, g, B)
    assert not hasattr(tr, "dR") and not hasattr(tr, "dT")
    assert len(tr.grads.params) == 3 and len(tr.opt.param_groups) == 1
    assert tr.grads.flat.numel() == sum(p.numel() for p in
                                        (m.xyz_encoder.params, m.mlp_params, g.params))
    o, d = (torch.from_numpy(a).to(cuda) for a in S.rays(B, 0.5))
    tgt = torch.rand(B, 3, generator=torch.Generator().manual_seed(5)).to(cuda)
    terms = tr.step(o, d, d, tgt)
    assert "rgb" in terms
    with pytest.raises(ValueError, match="directions"):
        tr.step_pixels(torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), tgt)
    # cameras without refinement: step_pixels runs on batch_rays' rays
    dirs, poses = S.ring_cameras(4, 24)
    tr2 = Trainer(m, g, B, directions=dirs, poses=poses)
    assert not hasattr(tr2, "dR") and len(tr2.grads.params) == 3
    gen = torch.Generator().manual_seed(3)
    terms = tr2.step_pixels(torch.randint(4, (B,), generator=gen),
                            torch.randint(dirs.shape[0], (B,), generator=gen), tgt)
    assert "rgb" in terms
