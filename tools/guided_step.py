"""Cost and effect of error-guided sampling (dev tool, GPU; DESIGN.md §4
"Error-guided sampling").  Appends JSON lines to profiles/guided/.

time   Trainer.step_sampled at C3 (100 images of 800 x 800, uint8, 8192 rays,
       K = 2, scale 0.5), three trainers interleaved round by round in one
       process, a device synchronise around each round of 16 steps (one
       occupancy-grid update and, for the guided ones, at most one refresh):
         uniform   guided=False: the step the parent commit runs;
         guided    guided=True with the defaults (tile 16, uniform_frac 0.5,
                   refresh every 16 steps);
         one_cell  guided=True, never refreshed, with a map of 300 in one
                   cell and 0 elsewhere (weights 2^24 against 1): the guided
                   half of every batch falls into one cell, the worst case
                   for the epilogue's atomics and for the search.
       Then the four kernels alone on an idle device (events around each),
       on the flat and on the one-cell map.
conv   tools/train_demo.py's analytic sphere as a training set (32 images of
       200 x 200 from cameras on the radius-1.5 sphere), guided against
       uniform at equal steps, three seeds each (model, gate and batch
       stream), PSNR on 32,768 held-out rays (train_demo.batch: fresh random
       rays with exact targets) after 250, 500 and 1000 steps.

usage: python tools/guided_step.py [time] [conv] [--out DIR]
"""
import functools
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radnerf_amd import sampler  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.trainer import Trainer  # noqa: E402
from steptime import alone_ms, append_jsonl, interleaved_ms  # noqa: E402
from train_demo import R_SPHERE, batch  # noqa: E402

DEV = torch.device("cuda")


def cameras(n_img, W, H, half=0.3, seed=0):
    """unit pixel directions (H W, 3) and n_img c2w poses on the radius-1.5
    sphere looking at the origin (columns right / up / forward)"""
    y, x = torch.meshgrid(torch.linspace(-half * H / W, half * H / W, H),
                          torch.linspace(-half, half, W), indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    u = torch.randn(n_img, 3, generator=torch.Generator().manual_seed(seed))
    pos = 1.5 * u / u.norm(dim=1, keepdim=True)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2)
    return dirs.contiguous(), poses.contiguous()


def sphere_images(dirs, poses):
    """the analytic sphere of tools/train_demo.py seen by those cameras, uint8"""
    out = []
    for P in poses:
        d = dirs @ P[:, :3].T
        o = P[:, 3].expand_as(d)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - R_SPHERE ** 2)
        t = -b - torch.sqrt(disc.clamp_min(0))
        hit = (disc > 0) & (t > 0)
        nrm = o + t[:, None] * d
        nrm = nrm / nrm.norm(dim=-1, keepdim=True)
        img = torch.where(hit[:, None], 0.5 + 0.5 * nrm, torch.ones_like(nrm))
        out.append((img * 255).round().to(torch.uint8))
    return torch.stack(out).contiguous()


def _trainer(data, wh, B, seed, **kw):
    dirs, poses, images = data
    m = MNGP(0.5, size=2, seed=3 + seed).to(DEV)
    g = Ray_Gate(2, seed=4 + seed).to(DEV)
    return Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, seed=seed, images=images,
                   directions=dirs, poses=poses, img_wh=wh, **kw)


# ---------------------------------------------------------------- step time
_alone = functools.partial(alone_ms, n=30, skip=3)


def step_time(steps=16, rounds=8):
    W = H = 800
    n_img, B = 100, 8192
    dirs, poses = cameras(n_img, W, H)
    images = torch.randint(0, 256, (n_img, W * H, 3), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(1))
    data = (dirs.to(DEV), poses.to(DEV), images.to(DEV))
    trs = {"uniform": _trainer(data, (W, H), B, 0),
           "guided": _trainer(data, (W, H), B, 0, guided=True),
           "one_cell": _trainer(data, (W, H), B, 0, guided=True, guided_refresh_every=1 << 30)}
    gs = trs["one_cell"].guided
    hot = gs.n_cells // 2 + 7

    def one_cell_map(s):
        s.emap.zero_()
        s.emap[hot] = 300.0
        s.update_weights()
    one_cell_map(gs)
    times = interleaved_ms({k: tr.step_sampled for k, tr in trs.items()}, steps, rounds, warm=False)
    b = trs["one_cell"].last_batch
    in_hot = float((b["cell_idx"] == hot).float().mean())
    out = {"what": "step_sampled", "images": n_img, "wh": [W, H], "rays": B, "K": 2, "scale": 0.5,
           "n_cells": gs.n_cells, "steps_per_round": steps, "rounds": rounds - 1,
           "one_cell_share_of_batch": round(in_hot, 4)}
    for k, t in times.items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    # the four kernels alone, on a flat and on the one-cell map
    tr = trs["guided"]
    s, K = tr.guided, tr.model.size
    rgb = torch.rand(B, 3, device=DEV)
    seeds = (torch.rand(B, 3, device=DEV), torch.rand(B, device=DEV), torch.rand(B, K, device=DEV))
    for name, prepare in (("flat", lambda: s.reset()), ("one_cell", lambda: one_cell_map(s))):
        prepare()
        bt = s.sample(tr.directions, tr.poses, B, K, 0, 5)
        fill = lambda: s.accumulate(rgb, bt["target"], bt["cell_idx"], bt["ray_weight"], K, *seeds)
        out["alone_ms_" + name] = {
            "weights": _alone(s.update_weights),
            "sample_guided": _alone(lambda: s.sample(tr.directions, tr.poses, B, K, 0, 5, out=bt)),
            "sample_uniform": _alone(lambda: sampler.sample_batch(
                s.images, tr.directions, tr.poses, B, K, 0, 5)),
            "epilogue": _alone(fill),
            # each refresh finds the cells of one batch filled
            "fill_and_refresh": _alone(lambda: (fill(), sampler.guided_refresh(
                s.emap, s.acc_sum, s.acc_cnt, s.alpha))),
        }
        out["alone_ms_" + name]["refresh"] = round(
            out["alone_ms_" + name]["fill_and_refresh"] - out["alone_ms_" + name]["epilogue"], 4)
    return out


# ---------------------------------------------------------------- convergence
def _psnr(tr, held):
    mse, n = 0.0, 0
    K, B = tr.model.size, tr.n_rays
    noise = torch.zeros(K, B, device=DEV)
    bg = torch.ones(3, device=DEV)
    with torch.no_grad():
        for o, d, target in held:
            rgb = tr.renderer.forward(o, d, d, noise, bg, 1e-4, tr.esf)[0]
            mse += float(((rgb - target) ** 2).sum())
            n += target.numel()
    return round(-10 * math.log10(max(mse / n, 1e-12)), 3)


def convergence(seeds=(0, 1, 2), marks=(250, 500, 1000)):
    W = H = 200
    n_img, B = 32, 8192
    dirs, poses = cameras(n_img, W, H)
    images = sphere_images(dirs, poses)
    data = (dirs.to(DEV), poses.to(DEV), images.to(DEV))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(99)
    held = [batch(gen, B, DEV, 1.0) for _ in range(4)]
    on_sphere = float((images.float().mean(-1) < 254).float().mean())
    out = {"what": "convergence", "images": n_img, "wh": [W, H], "rays": B, "K": 2, "scale": 0.5,
           "held_out_rays": 4 * B, "sphere_share_of_pixels": round(on_sphere, 4), "runs": []}
    for seed in seeds:
        for mode in ("uniform", "guided"):
            tr = _trainer(data, (W, H), B, seed, guided=mode == "guided")
            run = {"mode": mode, "seed": seed, "psnr": {}}
            for s in range(1, max(marks) + 1):
                tr.step_sampled()
                if s in marks:
                    run["psnr"][str(s)] = _psnr(tr, held)
            if mode == "guided":
                e = tr.guided.emap
                run["emap_min_median_max"] = [float(e.min()), float(e.median()), float(e.max())]
                w = tr.last_batch["ray_weight"]
                run["ray_weight_min_max"] = [round(float(w.min()), 4), round(float(w.max()), 4)]
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    for m in marks:
        for mode in ("uniform", "guided"):
            v = [r["psnr"][str(m)] for r in out["runs"] if r["mode"] == mode]
            out[f"{mode}_psnr_{m}"] = {"mean": round(float(np.mean(v)), 3), "min": min(v),
                                       "max": max(v)}
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    dest = os.path.join(ROOT, "profiles", "guided")
    if "--out" in args:
        i = args.index("--out")
        dest = args[i + 1]
        del args[i:i + 2]
    for name in args or ["time", "conv"]:
        append_jsonl(os.path.join(dest, {"time": "guided_step.jsonl",
                                         "conv": "guided_convergence.jsonl"}[name]),
                     {"time": step_time, "conv": convergence}[name]())
        torch.cuda.empty_cache()
