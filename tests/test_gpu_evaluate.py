"""GPU: whole-image validation (radnerf_amd.evaluate, Trainer.validate).

A 24 x 20 image in chunks of 128 rays (three full chunks and one of 96):
ImageEvaluator.render_image against rendering.ml_render(test_time=True) /
render(test_time=True) on the rays of the same pose -- the same render kernel,
so only the combine differs (<= 2e-6); the result does not depend on the chunk
(128 vs 480 bitwise); evaluate() against the fp64 metrics of the rendered image
(tests/metrics_ref.py, the bars of tests/test_gpu_metrics.py); Trainer.validate
over two poses leaves the training state bit-unchanged.
"""
import math

import pytest
import torch

import metrics_ref as MR
from radnerf_amd import synthetic as S
from radnerf_amd.evaluate import ImageEvaluator
from radnerf_amd.networks import NGP
from radnerf_amd.rays import batch_rays
from radnerf_amd.rendering import NEAR_DISTANCE, ml_render, render
from radnerf_amd.trainer import Trainer
from test_gpu_render import _init

pytestmark = pytest.mark.gpu

WH = (24, 20)
CHUNK = 128


def _camera(scale, n_poses=2, half=0.6):
    """Unit pixel directions of a W x H pinhole and poses on a ring of radius
    3 * scale looking at the origin (c2w columns right / up / forward)."""
    W, H = WH
    y, x = torch.meshgrid(torch.linspace(-half * H / W, half * H / W, H),
                          torch.linspace(-half, half, W), indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    ang = torch.arange(n_poses) * (2 * math.pi / 5) + 0.3
    pos = 3 * scale * torch.stack([torch.cos(ang), torch.sin(ang), 0.3 * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2)
    return dirs, poses.contiguous()


def _setup(cuda, K, gate_type, scale):
    if gate_type is None:
        m, g = NGP(scale, seed=3), None
        _init(m, p=0.3)
        m = m.to(cuda)
    else:
        sc = S.parity_scene(K, scale=scale, p=0.3, gate_type=gate_type, device=cuda)
        m, g = sc.m, sc.g
    dirs, poses = _camera(scale)
    return m, g, dirs.to(cuda), poses.to(cuda)


CASES = [(1, None), (2, "ray"), (2, "image")]


def _reference(cuda, m, g, dirs, pose, esf):
    """the public per-ray path on the rays of `pose` (train_ml.py:84-96 for one
    pose, then ml_render / render at test time)"""
    N = dirs.shape[0]
    zero = torch.zeros(N, dtype=torch.int64, device=cuda)
    o, d, i_d = batch_rays(dirs, pose[None].contiguous(), zero, torch.arange(N, device=cuda))
    with torch.no_grad():
        if g is None:
            ref = render(m, o, d, test_time=True, exp_step_factor=esf)
            return ref, ref["depth"][:, None], torch.ones(N, 1, device=cuda)
        ref = ml_render(m, g, o, d, i_d, test_time=True, exp_step_factor=esf)
        return ref, ref["depth"], ref["gating_code"]


@pytest.mark.parametrize("scale", [0.5, 16.0])
@pytest.mark.parametrize("K,gate_type", CASES)
def test_render_image_vs_ml_render(cuda, K, gate_type, scale):
    m, g, dirs, poses = _setup(cuda, K, gate_type, scale)
    esf = 1 / 256 if scale > 0.5 else 0.0
    N = dirs.shape[0]
    ev = ImageEvaluator(m, g, dirs, WH, chunk=CHUNK)
    assert ev.esf == esf and ev.chunk == CHUNK and N == 3 * CHUNK + 96
    # a camera on the ring, and one 0.005 in front of the box's -x face looking
    # in: its rays enter within NEAR_DISTANCE, where the near hit is clamped
    face = torch.tensor([[0.0, 0.0, 1.0, -scale - 0.005], [1.0, 0.0, 0.0, 0.0],
                         [0.0, 1.0, 0.0, 0.0]], device=cuda)
    for name, pose in (("ring", poses[1]), ("face", face)):
        res = {k: v.clone() for k, v in ev.render_image(pose).items()}
        ref, ref_depth_k, gate = _reference(cuda, m, g, dirs, pose, esf)
        assert res["rgb"].shape == (N, 3) and res["depth_k"].shape == (N, K)
        assert res["gating_code"].shape == (N, K) and res["opacity"].shape == (N,)
        errs = {"rgb": float((res["rgb"] - ref["rgb"]).abs().max()),
                "opacity": float((res["opacity"] - ref["opacity"]).abs().max()),
                "depth_k": float((res["depth_k"] - ref_depth_k).abs().max()),
                "gate": float((res["gating_code"] - gate).abs().max())}
        print(f"render_image K={K} gate={gate_type} scale={scale} {name}: {errs}, opacity mean "
              f"{float(ref['opacity'].mean()):.3f}, samples {int(res['total_samples'])}")
        assert all(v <= 2e-6 for v in errs.values()), (name, errs)
        assert int(res["total_samples"]) == int(ref["total_samples"]) > 0, name
        want = (gate.double() * ref_depth_k.double()).sum(1)
        rel = float(((res["depth"].double() - want).abs() / want.abs().clamp_min(1e-6)).max())
        assert rel <= 2e-6, (name, rel)
        if name == "ring":
            # the image is not trivial: some rays hit, some see the background
            assert 0.02 < float(ref["opacity"].mean()) < 0.999
        else:
            assert bool((ev.hits_t[:96, 0, 0] == NEAR_DISTANCE).any())
        # independent of the chunk: one chunk of 480 against four, bitwise
        one = ImageEvaluator(m, g, dirs, WH, chunk=N).render_image(pose)
        for k, v in res.items():
            assert torch.equal(v, one[k]), (name, k)


def test_evaluate_vs_fp64_metrics(cuda):
    m, g, dirs, poses = _setup(cuda, 2, "ray", 0.5)
    ev = ImageEvaluator(m, g, dirs, WH, chunk=CHUNK)
    gt = torch.rand(dirs.shape[0], 3, generator=torch.Generator().manual_seed(9)).to(cuda)
    got = ev.evaluate(poses[0], gt)
    rgb = ev.render_image(poses[0])["rgb"]
    ref_psnr, (ref_ssim, _) = MR.psnr_ref(rgb, gt), MR.ssim_ref(rgb, gt, WH)
    print(f"evaluate: psnr {float(got['psnr']):.6f} vs {ref_psnr:.6f}, ssim "
          f"{float(got['ssim']):.6f} vs {ref_ssim:.6f}")
    assert got["psnr"].device.type == "cuda" and got["ssim"].ndim == 0
    assert abs(float(got["psnr"]) - ref_psnr) <= 1e-4
    assert abs(float(got["ssim"]) - ref_ssim) <= 1e-4
    # against itself: inf and exactly 1
    same = ev.evaluate(poses[0], rgb.clone())
    assert float(same["psnr"]) == float("inf") and float(same["ssim"]) == 1.0
    with pytest.raises(ValueError, match="rgb_gt must be"):
        ev.evaluate(poses[0], gt[:-1])


def test_trainer_validate(cuda):
    m, g, dirs, poses = _setup(cuda, 2, "ray", 0.5)
    tr = Trainer(m, g, 256, directions=dirs, poses=poses, img_wh=WH)
    gt = torch.rand(2, dirs.shape[0], 3, generator=torch.Generator().manual_seed(4)).to(cuda)
    state = lambda: [t.detach().clone() for t in
                     [m.xyz_encoder.params, m.mlp_params, g.params]
                     + [getattr(m, f"density_{k}_{i}") for k in ("grid", "bitfield")
                        for i in range(2)]]
    before, step = state(), tr.global_step
    val = tr.validate(poses, gt)
    assert tr.global_step == step
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    assert len(val["per_image"]) == 2
    for k in ("psnr", "ssim"):
        per = [float(p[k]) for p in val["per_image"]]
        assert abs(float(val[k]) - sum(per) / 2) <= 1e-12 * max(1.0, abs(float(val[k])))
    # the per-image values are evaluate()'s, and the two views differ
    ev = ImageEvaluator(m, g, dirs, WH, exp_step_factor=tr.esf)
    for i in range(2):
        one = ev.evaluate(poses[i], gt[i])
        assert torch.equal(one["psnr"], val["per_image"][i]["psnr"])
        assert torch.equal(one["ssim"], val["per_image"][i]["ssim"])
    assert float(val["per_image"][0]["psnr"]) != float(val["per_image"][1]["psnr"])
    # a second validation gives the same numbers
    again = tr.validate(poses, gt)
    assert torch.equal(again["psnr"], val["psnr"]) and torch.equal(again["ssim"], val["ssim"])
