"""GPU: Trainer.fit on device-resident uint8 images.

The scene is the analytic sphere of tools/train_demo.py (radius 0.25, coloured
0.5 + 0.5 normal, white background) seen by 8 cameras on a ring, 64 x 48
uint8 images each, plus one held-out pose with its exact fp32 image.  4096
rays, K = 2, fit(num_epochs=3, steps_per_epoch=100):

  * each epoch's lr is sampler.cosine_lr;
  * validation PSNR after fit > before, last epoch's train PSNR > the first's;
  * a second trainer from the same initialisation goes through step_pixels
    with the picks and jitter of the numpy restatement (tests/sampler_ref.py),
    torch-gathered targets and the lr set by hand: identical inputs, so only
    the arrival order of the fp32 weight-gradient sums differs, and its final
    validation PSNR is within 0.5 dB of fit's (the bar of
    tests/test_gpu_train.py for two runs on the same data).

Measured on an MI355X: held-out PSNR 10.46 dB before, 13.56 dB after fit and
13.53 dB on the step_pixels path; train PSNR 19.4 / 40.6 / 49.3 dB per epoch.
The targets of the second trainer are divided by a tensor 255: torch's device
kernel for a python-scalar divisor multiplies by the reciprocal, which is not
the division the sampler performs.
"""
import math

import pytest
import torch

import sampler_ref as SR
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.sampler import cosine_lr
from radnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

WH = (64, 48)
R_SPHERE = 0.25
N_TRAIN, B, K, SEED, LR = 8, 4096, 2, 5, 1e-2
EPOCHS, STEPS = 3, 100


def _cameras(n_poses, half=0.3, radius=1.5):
    """as tests/test_gpu_evaluate.py::_camera: unit pixel directions of a W x H
    pinhole, poses on a ring looking at the origin"""
    W, H = WH
    y, x = torch.meshgrid(torch.linspace(-half * H / W, half * H / W, H),
                          torch.linspace(-half, half, W), indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    ang = torch.arange(n_poses) * (2 * math.pi / n_poses) + 0.3
    pos = radius * torch.stack([torch.cos(ang), torch.sin(ang), 0.3 * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2)
    return dirs, poses.contiguous()


def _images(dirs, poses):
    """the exact images (N, H*W, 3) fp32: sphere hit -> 0.5 + 0.5 n, else white"""
    d = torch.einsum("pj,nij->npi", dirs, poses[:, :, :3])
    o = poses[:, None, :, 3].expand_as(d)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - R_SPHERE ** 2)
    t = -b - torch.sqrt(disc.clamp_min(0))
    hit = (disc > 0) & (t > 0)
    nrm = o + t[..., None] * d
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    return torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.ones_like(nrm)).contiguous()


def _trainer(cuda, dirs, poses, images):
    m = MNGP(0.5, size=K, seed=3).to(cuda)
    g = Ray_Gate(K, seed=4).to(cuda)
    return Trainer(m, g, B, lr=LR, lambda_cv_importance=1e-2, seed=SEED, directions=dirs,
                   poses=poses, img_wh=WH, images=images)


def test_fit_trains_and_matches_the_step_pixels_path(cuda):
    dirs, all_poses = _cameras(N_TRAIN + 1)
    exact = _images(dirs, all_poses)
    # the held-out view sits between two training views
    train_poses, val_poses = all_poses[:N_TRAIN].contiguous(), all_poses[N_TRAIN:].contiguous()
    u8 = (exact[:N_TRAIN] * 255).round().to(torch.uint8).contiguous().to(cuda)
    val_images = exact[N_TRAIN:].contiguous().to(cuda)
    assert 0.05 < float((exact[N_TRAIN] < 1).any(-1).float().mean()) < 0.9   # the sphere is in view
    dirs, train_poses, val_poses = dirs.to(cuda), train_poses.to(cuda), val_poses.to(cuda)

    tr = _trainer(cuda, dirs, train_poses, u8)
    before = float(tr.validate(val_poses, val_images)["psnr"])
    seen = []
    log = tr.fit(num_epochs=EPOCHS, steps_per_epoch=STEPS, val_poses=val_poses,
                 val_images=val_images, callback=seen.append)
    assert tr.global_step == EPOCHS * STEPS and len(log) == EPOCHS and seen == log
    for e, entry in enumerate(log):
        assert entry["epoch"] == e and entry["lr"] == cosine_lr(LR, e, EPOCHS)
        assert set(entry["terms"]) >= {"rgb", "opacity", "cv_importance"}
        assert entry["loss"] == pytest.approx(sum(entry["terms"].values()), rel=1e-12)
        assert entry["train_psnr"] == pytest.approx(-10 * math.log10(entry["terms"]["rgb"]))
        # val_every defaults to min(num_epochs, 10): the last epoch only
        assert ("val" in entry) == (e == EPOCHS - 1)
    assert log[0]["lr"] == LR and log[-1]["lr"] < LR
    assert tr.opt.param_groups[0]["lr"] == log[-1]["lr"]
    after = log[-1]["val"]["psnr"]
    assert after == float(tr.validate(val_poses, val_images)["psnr"])
    print(f"fit: validation PSNR {before:.2f} -> {after:.2f} dB, SSIM {log[-1]['val']['ssim']:.4f}, "
          f"train PSNR per epoch {[round(e['train_psnr'], 2) for e in log]}")
    assert after > before
    assert log[-1]["train_psnr"] > log[0]["train_psnr"]

    # the parent's path on identical inputs
    tr2 = _trainer(cuda, dirs, train_poses, None)
    n_pix = dirs.shape[0]
    # a tensor divisor: on the device torch divides by a python scalar as a
    # multiplication by its reciprocal, which is not the division the sampler
    # (and torch on the host) performs
    d255 = torch.full((), 255.0, device=cuda)
    for step in range(EPOCHS * STEPS):
        if step % STEPS == 0:
            tr2.opt.param_groups[0]["lr"] = cosine_lr(LR, step // STEPS, EPOCHS)
        assert tr2.global_step == step
        img, pix = (torch.from_numpy(a).to(cuda) for a in
                    SR.picks(SEED, step, 0, B, N_TRAIN, n_pix))
        nz = torch.from_numpy(SR.noise(SEED, step, 0, K, B)).to(cuda)
        tgt = u8[img, pix].float() / d255
        tr2.step_pixels(img, pix, tgt, noise=nz)
    # the two consumed the same last batch
    last = tr.last_batch
    assert torch.equal(last["img_idxs"], img) and torch.equal(last["pix_idxs"], pix)
    assert torch.equal(last["noise"], nz) and torch.equal(last["target"], tgt)
    other = float(tr2.validate(val_poses, val_images)["psnr"])
    print(f"fit {after:.3f} dB vs step_pixels on the same inputs {other:.3f} dB")
    assert abs(after - other) <= 0.5, (after, other)


def test_fit_every_epoch_validation_and_eta_min(cuda):
    """val_every=1 validates every epoch; eta_min is passed on; no validation
    set, no "val"; the pose group's lr is left alone."""
    dirs, poses = _cameras(N_TRAIN)
    u8 = (_images(dirs, poses) * 255).round().to(torch.uint8).contiguous().to(cuda)
    dirs, poses = dirs.to(cuda), poses.to(cuda)
    m, g = MNGP(0.5, size=K, seed=3).to(cuda), Ray_Gate(K, seed=4).to(cuda)
    tr = Trainer(m, g, 256, lr=LR, seed=SEED, directions=dirs, poses=poses, img_wh=WH,
                 images=u8, optimize_ext=True, pose_lr=1e-6)
    val = u8[:1].float() / 255
    log = tr.fit(num_epochs=2, steps_per_epoch=3, val_poses=poses[:1], val_images=val,
                 val_every=1, eta_min=1e-3)
    assert [e["lr"] for e in log] == [cosine_lr(LR, e, 2, 1e-3) for e in range(2)]
    assert log[1]["lr"] == pytest.approx((LR + 1e-3) / 2)
    assert all("val" in e and math.isfinite(e["val"]["psnr"]) for e in log)
    assert [pg["lr"] for pg in tr.opt.param_groups] == [log[1]["lr"], 1e-6]
    assert tr.global_step == 6
    log = tr.fit(num_epochs=1, steps_per_epoch=2)
    assert "val" not in log[0] and tr.global_step == 8
