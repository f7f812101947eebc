"""GPU: the batch sampler (rn_sample_batch, radnerf_amd.sampler) and
Trainer.step_sampled.

5 images of 23 x 37 pixels, uint8 and fp32, n = 1000 rays (three full
256-thread blocks and a tail of 232) and K = 2, plus n = 1 and n_images = 1.
Picks, jitter and background are compared exactly with the numpy restatement
of the stream (tests/sampler_ref.py), the targets bitwise with torch's gather,
the rays bitwise with rays.batch_rays / rays.pose_rays on the same picks; every
output sits in front of canary rows that must stay untouched.
"""
import math

import numpy as np
import pytest
import torch

import sampler_ref as SR
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.rays import batch_rays, pose_rays
from radnerf_amd.sampler import KEYS, TrainImages, sample_batch
from radnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

N_IMG, WH, N, K, SEED = 5, (37, 23), 1000, 2, 11
N_PIX = WH[0] * WH[1]
CANARY = 8


def _cameras(n_img, radius, half=0.3):
    """n_img cameras on a ring of `radius` looking at the origin (c2w columns
    right / up / forward) and the W x H unit pixel directions"""
    W, H = WH
    y, x = torch.meshgrid(torch.linspace(-half * H / W, half * H / W, H),
                          torch.linspace(-half, half, W), indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    ang = torch.arange(n_img) * (2 * math.pi / n_img) + 0.3
    pos = torch.stack([radius * torch.cos(ang), radius * torch.sin(ang),
                       0.27 * radius * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2)
    return dirs.contiguous(), poses.contiguous()


@pytest.fixture(scope="module")
def scene(cuda):
    gen = torch.Generator().manual_seed(5)
    dirs, poses = _cameras(N_IMG, 1.5)
    u8 = torch.randint(0, 256, (N_IMG, N_PIX, 3), generator=gen, dtype=torch.uint8)
    # every byte value is in the set: the uint8 target is compared on all 256
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    f32 = torch.rand(N_IMG, N_PIX, 3, generator=gen)
    dR = 0.05 * torch.randn(N_IMG, 3, generator=gen)
    dT = 0.05 * torch.randn(N_IMG, 3, generator=gen)
    dirs = dirs.to(cuda)
    return {"dirs": dirs, "poses": poses.to(cuda), "uint8": u8.to(cuda), "fp32": f32.to(cuda),
            "dR": dR.to(cuda), "dT": dT.to(cuda), "mean_dir": dirs.mean(0).contiguous()}


def _guarded(n, k, with_imgs_d, dev):
    """sample_batch's buffers as the leading rows of larger ones filled with a
    canary: (views for out=, [(whole buffer, rows in use)])"""
    i64, f32, rows = torch.int64, torch.float32, n + CANARY
    spec = {"img_idxs": ((rows,), i64, n), "pix_idxs": ((rows,), i64, n),
            "target": ((rows, 3), f32, n), "rays_o": ((rows, 3), f32, n),
            "rays_d": ((rows, 3), f32, n), "imgs_d": ((rows, 3), f32, n),
            "noise": ((k * n + CANARY,), f32, k * n), "bg": ((3 + CANARY,), f32, 3)}
    views, whole = {}, []
    for name, (shape, dtype, used) in spec.items():
        if name == "imgs_d" and not with_imgs_d:
            views[name] = None
            continue
        buf = torch.full(shape, -7, dtype=dtype, device=dev)
        whole.append((name, buf, used))
        views[name] = buf[:used].view(k, n) if name == "noise" else buf[:used]
    return views, whole


def _canaries_intact(whole):
    for name, buf, used in whole:
        assert bool((buf[used:] == -7).all()), name
        if buf.dtype == torch.float32:
            assert not bool((buf[:used] == -7).any()), name       # every row was written


def _ref(step, rank, n, n_img, k=K, seed=SEED):
    img, pix = SR.picks(seed, step, rank, n, n_img, N_PIX)
    return img, pix, SR.noise(seed, step, rank, k, n), SR.bg(seed, step, rank)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _u8_target(images, img, pix):
    """images[img, pix].float() / 255 as torch divides on the host: a true
    division.  (On the device torch divides by a python scalar as a
    multiplication by its reciprocal, which differs on 126 of the 256 byte
    values; a tensor divisor is divided by there too, and is checked to give
    the same bits.)"""
    want = (images.cpu()[img.cpu(), pix.cpu()].float() / 255).to(images.device)
    on_device = images[img, pix].float() / torch.full((), 255.0, device=images.device)
    assert _same_bits(on_device, want)
    return want


@pytest.mark.parametrize("n,n_img", [(N, N_IMG), (1, N_IMG), (N, 1)])
@pytest.mark.parametrize("dtype", ["uint8", "fp32"])
def test_batch_matches_restatement_and_batch_rays(cuda, scene, dtype, n, n_img):
    images = scene[dtype][:n_img].contiguous()
    poses = scene["poses"][:n_img].contiguous()
    ti = TrainImages(images)
    assert ti.images.data_ptr() == images.data_ptr() and ti.images.dtype == images.dtype
    step, rank = 3, 2
    views, whole = _guarded(n, K, True, cuda)
    b = sample_batch(ti, scene["dirs"], poses, n, K, SEED, step, rank=rank,
                     mean_dir=scene["mean_dir"], out=views)
    assert b is views and set(b) == set(KEYS)
    _canaries_intact(whole)
    img, pix, nz, bg = _ref(step, rank, n, n_img)
    assert b["img_idxs"].dtype == torch.int64 and b["pix_idxs"].dtype == torch.int64
    assert np.array_equal(b["img_idxs"].cpu().numpy(), img)
    assert np.array_equal(b["pix_idxs"].cpu().numpy(), pix)
    assert np.array_equal(b["noise"].cpu().numpy(), nz) and b["noise"].shape == (K, n)
    assert np.array_equal(b["bg"].cpu().numpy(), bg)
    if n_img == 1:
        assert int(b["img_idxs"].abs().max()) == 0
    # the target: torch's own gather and division
    if dtype == "uint8":
        want = _u8_target(images, b["img_idxs"], b["pix_idxs"])
    else:
        want = images[b["img_idxs"], b["pix_idxs"]]
    assert _same_bits(b["target"], want)
    if dtype == "uint8" and n == N:
        assert len(torch.unique(images[b["img_idxs"], b["pix_idxs"]])) > 200
    # the rays: rn_get_rays' bits on the same picks
    ro, rd, imd = batch_rays(scene["dirs"], poses, b["img_idxs"], b["pix_idxs"])
    assert _same_bits(b["rays_o"], ro) and _same_bits(b["rays_d"], rd)
    assert _same_bits(b["imgs_d"], imd)
    # without mean_dir: no imgs_d, everything else the same bits
    c = sample_batch(ti, scene["dirs"], poses, n, K, SEED, step, rank=rank)
    assert c["imgs_d"] is None
    for k in KEYS:
        if k != "imgs_d":
            assert torch.equal(c[k], b[k]), k


def test_uint8_target_on_every_byte_value(cuda):
    """(float)v / 255 on all 256 values, bitwise torch's u8.float() / 255: one
    image whose pixel p holds the byte p % 256 in every channel."""
    n_pix = 512
    im = (torch.arange(n_pix) % 256).to(torch.uint8)[None, :, None].expand(1, n_pix, 3)
    im = im.contiguous().to(cuda)
    dirs = torch.nn.functional.normalize(torch.rand(n_pix, 3), dim=1).to(cuda)
    pose = torch.eye(3, 4)[None].contiguous().to(cuda)
    b = sample_batch(TrainImages(im), dirs, pose, 4096, 1, 1, 0)
    vals = im[0, b["pix_idxs"], 0]
    assert len(torch.unique(vals)) == 256
    assert _same_bits(b["target"], _u8_target(im, b["img_idxs"], b["pix_idxs"]))
    assert np.array_equal(b["pix_idxs"].cpu().numpy(), SR.picks(1, 0, 0, 4096, 1, n_pix)[1])


@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("which", ["both", "dR", "dT"])
def test_refined_rays_match_pose_rays(cuda, scene, with_mean, which):
    ti = TrainImages(scene["uint8"])
    dR = scene["dR"] if which in ("both", "dR") else None
    dT = scene["dT"] if which in ("both", "dT") else None
    mean = scene["mean_dir"] if with_mean else None
    views, whole = _guarded(N, K, with_mean, cuda)
    b = sample_batch(ti, scene["dirs"], scene["poses"], N, K, SEED, 9, dR=dR, dT=dT,
                     mean_dir=mean, out=views)
    _canaries_intact(whole)
    img, pix, nz, _ = _ref(9, 0, N, N_IMG)
    assert np.array_equal(b["img_idxs"].cpu().numpy(), img)
    assert np.array_equal(b["pix_idxs"].cpu().numpy(), pix)
    assert np.array_equal(b["noise"].cpu().numpy(), nz)
    zero = torch.zeros_like(scene["dR"])
    with torch.no_grad():
        ref = pose_rays(scene["dirs"], scene["poses"], zero if dR is None else dR,
                        zero if dT is None else dT, b["img_idxs"], b["pix_idxs"],
                        with_imgs_d=with_mean, mean_dir=mean)
    assert _same_bits(b["rays_o"], ref[0]) and _same_bits(b["rays_d"], ref[1])
    if with_mean:
        assert _same_bits(b["imgs_d"], ref[2])
    else:
        assert b["imgs_d"] is None
    # the refinement moved the rays
    plain = batch_rays(scene["dirs"], scene["poses"], b["img_idxs"], b["pix_idxs"])
    assert (dT is None) == torch.equal(b["rays_o"], plain[0])
    assert (dR is None) == torch.equal(b["rays_d"], plain[1])


def test_out_reuse_and_keys(cuda, scene):
    ti = TrainImages(scene["fp32"])
    args = (ti, scene["dirs"], scene["poses"], N, K)
    first = sample_batch(*args, SEED, 4, mean_dir=scene["mean_dir"])
    keep = {k: v.clone() for k, v in first.items()}
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    # another key into the same buffers, then the first key again
    other = sample_batch(*args, SEED, 5, mean_dir=scene["mean_dir"], out=first)
    assert other is first and {k: v.data_ptr() for k, v in other.items()} == ptrs
    cell = lambda b: b["img_idxs"] * N_PIX + b["pix_idxs"]
    assert float((cell(other) == cell(keep)).float().mean()) < 0.01
    assert not torch.equal(other["noise"], keep["noise"])
    assert not torch.equal(other["bg"], keep["bg"])
    again = sample_batch(*args, SEED, 4, mean_dir=scene["mean_dir"], out=first)
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    for k in KEYS:
        assert torch.equal(again[k], keep[k]), k
    # step, rank and seed each select another batch; a fresh call with the
    # same key gives the same bits
    for kw in (dict(seed=SEED, step=5, rank=0), dict(seed=SEED, step=4, rank=1),
               dict(seed=SEED + 1, step=4, rank=0)):
        b = sample_batch(*args, kw["seed"], kw["step"], rank=kw["rank"])
        assert float((cell(b) == cell(keep)).float().mean()) < 0.01, kw
        assert not torch.equal(b["noise"], keep["noise"]), kw
        img, pix, nz, bg = _ref(kw["step"], kw["rank"], N, N_IMG, seed=kw["seed"])
        assert np.array_equal(b["img_idxs"].cpu().numpy(), img), kw
        assert np.array_equal(b["bg"].cpu().numpy(), bg), kw
    same = sample_batch(*args, SEED, 4, mean_dir=scene["mean_dir"])
    assert same["target"].data_ptr() != ptrs["target"]
    for k in KEYS:
        assert torch.equal(same[k], keep[k]), k
    # no ray: nothing is written, empty outputs
    empty = sample_batch(ti, scene["dirs"], scene["poses"], 0, K, SEED, 4)
    assert empty["target"].shape == (0, 3) and empty["noise"].shape == (K, 0)


# ---------------------------------------------------------------- the trainer
def _models(cuda, gate_type, scale):
    m, g = MNGP(scale, size=K, seed=3), Ray_Gate(K, type=gate_type, seed=2)
    with torch.no_grad():
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(K, LY.FIELD_PARAMS)))
        g.params.copy_(torch.from_numpy(S.mlp_params(1, LY.gate_params(K), seed=6)[0]))
    return m.to(cuda), g.to(cuda)


def _check_last_batch(tr, step, images, B):
    b = tr.last_batch
    img, pix, nz, bg = _ref(step, 0, B, N_IMG, seed=tr.seed)
    assert np.array_equal(b["img_idxs"].cpu().numpy(), img), step
    assert np.array_equal(b["pix_idxs"].cpu().numpy(), pix), step
    assert np.array_equal(b["noise"].cpu().numpy(), nz), step
    assert np.array_equal(b["bg"].cpu().numpy(), bg), step
    assert _same_bits(b["target"], _u8_target(images, b["img_idxs"], b["pix_idxs"]))
    return b


@pytest.mark.parametrize("scale,random_bg,gate_type", [(0.5, False, "ray"), (16.0, True, "image")])
def test_trainer_step_sampled(cuda, scene, scale, random_bg, gate_type, monkeypatch):
    B = 256
    m, g = _models(cuda, gate_type, scale)
    dirs, poses = (t.to(cuda) for t in _cameras(N_IMG, 3 * scale))
    tr = Trainer(m, g, B, directions=dirs, poses=poses, images=scene["uint8"], seed=7,
                 random_bg=random_bg)
    assert isinstance(tr.images, TrainImages) and tr.images.images.dtype == torch.uint8
    assert tr.last_batch is None and tr.global_step == 0
    # the background and the jitter the render consumed
    seen = []
    real = tr.renderer.train_step
    def spy(rays_o, rays_d, second, target, noise, bg, **kw):
        seen.append({"o": rays_o, "d": rays_d, "second": second, "target": target,
                     "noise": noise, "bg": bg.clone()})
        return real(rays_o, rays_d, second, target, noise, bg, **kw)
    monkeypatch.setattr(tr.renderer, "train_step", spy)
    before = [p.detach().clone() for p in (m.xyz_encoder.params, m.mlp_params, g.params)]
    ptrs = None
    for step in (0, 1):
        terms = tr.step_sampled()
        assert tr.global_step == step + 1 and torch.isfinite(terms["rgb"])
        b = _check_last_batch(tr, step, scene["uint8"], B)
        ro, rd, imd = batch_rays(dirs, poses, b["img_idxs"], b["pix_idxs"])
        assert _same_bits(b["rays_o"], ro) and _same_bits(b["rays_d"], rd)
        s = seen[-1]
        assert s["o"] is b["rays_o"] and s["d"] is b["rays_d"] and s["target"] is b["target"]
        assert s["noise"] is b["noise"]
        if gate_type == "image":
            assert _same_bits(b["imgs_d"], imd) and s["second"] is b["imgs_d"]
        else:
            assert b["imgs_d"] is None and s["second"] is b["rays_d"]
        if random_bg:                     # esf != 0 at scale 16: the sampled background
            assert tr.esf != 0 and torch.equal(s["bg"], b["bg"])
        else:                             # scale 0.5: white
            assert tr.esf == 0 and torch.equal(s["bg"], torch.ones(3, device=cuda))
        # the buffers are reused from step to step
        now = {k: v.data_ptr() for k, v in b.items() if v is not None}
        assert ptrs is None or now == ptrs
        ptrs = now
    for p, b0 in zip((m.xyz_encoder.params, m.mlp_params, g.params), before):
        assert not torch.equal(p.detach(), b0)
    # a caller's jitter overrides the sampled one
    nz = torch.rand(K, B, device=cuda)
    tr.step_sampled(noise=nz)
    assert seen[-1]["noise"] is nz
    # a second trainer with the same seed at the same global_step draws the same batch
    m2, g2 = _models(cuda, gate_type, scale)
    tr2 = Trainer(m2, g2, B, directions=dirs, poses=poses, images=TrainImages(scene["uint8"]),
                  seed=7, random_bg=random_bg)
    tr2.global_step = tr.global_step - 1
    tr2.step_sampled()
    want, got = tr.last_batch, tr2.last_batch
    for k in KEYS:
        assert (want[k] is None and got[k] is None) or torch.equal(want[k], got[k]), k
    with pytest.raises(ValueError, match="step_sampled needs"):
        Trainer(m2, g2, B, directions=dirs, poses=poses).step_sampled()


@pytest.mark.parametrize("gate_type", ["ray", "image"])
def test_trainer_step_sampled_optimize_ext(cuda, scene, gate_type):
    B, lr = 256, 1e-3
    m, g = _models(cuda, gate_type, 0.5)
    dirs, poses = (t.to(cuda) for t in _cameras(N_IMG, 1.5))
    tr = Trainer(m, g, B, directions=dirs, poses=poses, images=scene["uint8"], seed=3,
                 optimize_ext=True, pose_lr=lr)
    with torch.no_grad():
        tr.dR.copy_(scene["dR"])
        tr.dT.copy_(scene["dT"])
    for step in (0, 1):
        dR, dT = tr.dR.detach().clone(), tr.dT.detach().clone()
        terms = tr.step_sampled()
        assert torch.isfinite(terms["rgb"])
        b = _check_last_batch(tr, step, scene["uint8"], B)
        with torch.no_grad():
            ref = pose_rays(dirs, poses, dR, dT, b["img_idxs"], b["pix_idxs"],
                            with_imgs_d=gate_type == "image", mean_dir=tr.mean_dir)
        assert _same_bits(b["rays_o"], ref[0]) and _same_bits(b["rays_d"], ref[1])
        if gate_type == "image":
            assert _same_bits(b["imgs_d"], ref[2])
        for p in (tr.dR, tr.dT):
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
            assert torch.isfinite(p).all()
        # the poses moved by Adam's step
        assert not torch.equal(tr.dR.detach(), dR) and not torch.equal(tr.dT.detach(), dT)
