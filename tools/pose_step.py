"""Whole-step cost of camera pose refinement on the fused chain (dev tool,
GPU): ray generation + render + NeRFLoss + backward (no optimizer) at C3
(K = 2, 8192 rays, scale 0.5), the forms interleaved round by round in one
process (as tools/distortion_step.py), a device synchronise around the timed
steps; one JSON line with the median ms per step.

  default    rays.batch_rays + FusedMLRenderer.train_step: fixed poses;
  raygrad    the same with train_step(input_grad=True): what rn_field_dinput +
             rn_ml_march_bw and the gate's input gradient add on their own
             (they are part of every optimize_ext step below);
  fused      rays.pose_rays + train_step(input_grad=True) +
             rn_get_rays_pose_bw into a (N, 3) pair: Trainer.step_pixels with
             optimize_ext, without the optimizer;
  torch      the same step composed in torch: axisangle_to_R, the pose
             composition and get_rays twice as torch ops with autograd
             (train_ml.py:84-96), ml_render_fused (the same kernels behind
             autograd) and NeRFLoss.

Then the two pose kernels alone (20 back-to-back launches between two events,
median of 15 such bursts, us per launch) at 8192 picks for N = 100, 1000 and
4000 images: the backward reads the batch's image indices once per image, so
its cost grows with N.

usage: python tools/pose_step.py [--out FILE]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd._lib import lib  # noqa: E402
from radnerf_amd.fused import FusedMLRenderer, ml_render_fused  # noqa: E402
from radnerf_amd.losses import NeRFLoss  # noqa: E402
from radnerf_amd.rays import batch_rays, pose_rays, pose_rays_backward  # noqa: E402
from radnerf_amd.synthetic import ring_cameras  # noqa: E402
from steptime import append_jsonl, interleaved_ms  # noqa: E402

LAMBDAS = dict(lambda_opacity=1e-3, lambda_cv_importance=1e-2)


def axisangle_to_R(v):
    """ray_utils.py:73-100, op for op"""
    zero = torch.zeros_like(v[:, :1])
    k0 = torch.cat([zero, -v[:, 2:3], v[:, 1:2]], 1)
    k1 = torch.cat([v[:, 2:3], zero, -v[:, 0:1]], 1)
    k2 = torch.cat([-v[:, 1:2], v[:, 0:1], zero], 1)
    K = torch.stack([k0, k1, k2], dim=1)
    n = (torch.norm(v, dim=1) + 1e-7)[:, None, None]
    eye = torch.eye(3, device=v.device)
    return eye + (torch.sin(n) / n) * K + ((1 - torch.cos(n)) / n ** 2) * (K @ K)


def torch_pose_chain(dirs, poses, dR, dT, img, pix):
    """train_ml.py:84-96 with optimize_ext"""
    P = poses[img]
    rot = (axisangle_to_R(dR[img]) @ P[..., :3]).transpose(1, 2)
    rays_o = P[..., 3] + dT[img]
    rays_d = (dirs[pix][:, None, :] @ rot)[:, 0]
    mean = torch.mean(dirs, 0, keepdim=True).repeat(img.shape[0], 1)
    imgs_d = (mean[:, None, :] @ rot)[:, 0]
    return rays_o, rays_d, imgs_d


def kernel_us(fn, reps=15, burst=20):
    """us per launch: `burst` back-to-back launches between two events (the
    kernel plus the gap between dependent-free launches), median of `reps`."""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / burst)
    return round(float(np.median(ts)), 2)


def run(steps=10, rounds=6, n_img=100, res=400):
    K, B, scale = 2, 8192, 0.5
    dev = torch.device("cuda")
    sc = S.bench_scene(K, B, scale, dev)
    m, g, nz, bg = sc.m, sc.g, sc.noise, sc.bg
    dirs, poses = (t.to(dev) for t in ring_cameras(n_img, res))
    gen = torch.Generator().manual_seed(0)
    img = torch.randint(n_img, (B,), generator=gen).to(dev)
    pix = torch.randint(dirs.shape[0], (B,), generator=gen).to(dev)
    tgt = torch.rand(B, 3, generator=gen).to(dev)
    dR = (1e-2 * torch.randn(n_img, 3, generator=gen)).to(dev)
    dT = (1e-2 * torch.randn(n_img, 3, generator=gen)).to(dev)
    mean = dirs.mean(0).contiguous()
    r = FusedMLRenderer(m, g, B)
    oR, oT = torch.empty_like(dR), torch.empty_like(dT)
    kw = dict(grid_grad=sc.grid_grad, mlp_grad=sc.mlp_grad, gate_grad=sc.gate_grad, **LAMBDAS)
    loss_fn = NeRFLoss()
    leaves = [dR.clone().requires_grad_(True), dT.clone().requires_grad_(True)]

    def default():
        o, d, _ = batch_rays(dirs, poses, img, pix)
        r.train_step(o, d, d, tgt, nz, bg, **kw)

    def raygrad():
        o, d, _ = batch_rays(dirs, poses, img, pix)
        r.train_step(o, d, d, tgt, nz, bg, input_grad=True, **kw)

    def fused():
        with torch.no_grad():
            o, d, _ = pose_rays(dirs, poses, dR, dT, img, pix, mean_dir=mean)
        _, _, (g_o, g_d, g_2) = r.train_step(o, d, d, tgt, nz, bg, input_grad=True, **kw)
        pose_rays_backward(dirs, poses, dR, img, pix, mean, g_o, g_d + g_2, None, oR, oT)

    def composed():
        for p in (m.xyz_encoder.params, m.mlp_params, g.params, *leaves):
            p.grad = None
        o, d, i = torch_pose_chain(dirs, poses, leaves[0], leaves[1], img, pix)
        res = ml_render_fused(m, g, o, d, i, noise=nz)
        sum(v.mean() for v in loss_fn(res, {"rgb": tgt}, **LAMBDAS).values()).backward()

    forms = {"default": default, "raygrad": raygrad, "fused": fused, "torch": composed}
    times = interleaved_ms(forms, steps, rounds)
    out = {"shape": "c3", "K": K, "rays": B, "scale": scale, "images": n_img,
           "pixels_per_image": res * res, "samples": r.ws.n_samples(), "steps": steps,
           "rounds": rounds - 1}
    for k, t in times.items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    # the fused and the composed step agree on what they compute
    fused()
    composed()
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    out["fused_vs_torch_rel_l2"] = {"dR": round(rel(oR, leaves[0].grad), 6),
                                    "dT": round(rel(oT, leaves[1].grad), 6)}
    # the pose kernels alone, by the number of images
    L, st = lib(), torch.cuda.current_stream(dev).cuda_stream
    g_o, g_d = torch.randn(B, 3, device=dev), torch.randn(B, 3, device=dev)
    o3 = [torch.empty(B, 3, device=dev) for _ in range(3)]
    ptr = lambda *ts: [t.data_ptr() for t in ts]
    out["kernels_us"] = {"get_rays": kernel_us(lambda: L.get_rays(
        *ptr(dirs, poses, img, pix), B, *ptr(mean, *o3), st))}
    for n in (100, 1000, 4000):
        P = poses[torch.arange(n, device=dev) % n_img].contiguous()
        im = torch.randint(n, (B,), generator=gen).to(dev)
        vR, vT = 1e-2 * torch.randn(n, 3, device=dev), 1e-2 * torch.randn(n, 3, device=dev)
        bR, bT = torch.empty_like(vR), torch.empty_like(vT)
        fw = kernel_us(lambda: L.get_rays_pose(*ptr(dirs, P, vR, vT, im, pix), B,
                                               *ptr(mean, *o3), st))
        bw = kernel_us(lambda: L.get_rays_pose_bw(*ptr(dirs, P, vR, im, pix), B, n,
                                                  *ptr(mean, g_o, g_d, g_o, bR, bT), st))
        out["kernels_us"][str(n)] = {"get_rays_pose": fw, "get_rays_pose_bw": bw}
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = argv[argv.index("--out") + 1] if "--out" in argv else \
        os.path.join(ROOT, "profiles", "pose", "pose_step.jsonl")
    append_jsonl(path, run())
