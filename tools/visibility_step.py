"""Cost and effect of the camera-visibility cull (dev tool, GPU).  100 cameras
on an inward-facing ring of radius 1.5 (tools/pose_demo.py ring_cameras, 800 x
800, half-width 0.3), one JSON line per measurement:

  mark     rn_mark_invisible_cells alone at C3's (K = 2, scale 0.5, one
           cascade) and C5's (K = 8, scale 16, six cascades) grid shapes: us
           per call (bursts of back-to-back launches between two events), the
           culled share per cascade, cell-camera tests per second;
  update   the warm-up and the sampled occupancy update at C5's shape through
           rn_density_update_sampled (old) and rn_density_update_visible
           (new), interleaved call by call in one process, each call between
           two events on the same restored grid state (the state after one
           warm-up update of the seeded model): on an unculled grid (the new
           entry must not cost more than the old one's own spread) and on the
           grid culled by the ring (time next to the culled share and the
           number of listed cells);
  marched  samples per step of a C5-shaped Trainer (8192 rays, 100 seeded 200 x
           200 images) after 256 steps, with and without cull_invisible.

usage: python tools/visibility_step.py [--out FILE] [--rounds N] [--skip-marched]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pose_step import kernel_us  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.synthetic import ring_cameras, set_bitfields  # noqa: E402
from radnerf_amd.trainer import MAX_SAMPLES, Trainer  # noqa: E402

N_CAMS, RES, HALF = 100, 800, 0.3
THR = 0.01 * MAX_SAMPLES / 3 ** 0.5
SHAPES = {"c3": (2, 0.5), "c5": (8, 16.0)}


def ring_intrinsics(res, half=HALF):
    """the pinhole of ring_cameras: x = (i + 0.5 - cx) / fx spans [-half, half]"""
    f = (res - 1) / (2 * half)
    return np.array([[f, 0, 0.5 + half * f], [0, f, 0.5 + half * f], [0, 0, 1]])


def mark_alone(shape, poses):
    K, scale = SHAPES[shape]
    m = MNGP(scale, size=K, seed=3).to("cuda")
    Kmat = ring_intrinsics(RES)
    culled = m.mark_invisible_cells(Kmat, poses, (RES, RES))
    us = kernel_us(lambda: m.mark_invisible_cells(Kmat, poses, (RES, RES)))
    cells = m.cascades * m.grid_size ** 3
    return {"what": "mark", "shape": shape, "K": K, "scale": scale, "cascades": m.cascades,
            "cameras": N_CAMS, "us_per_call": us,
            "culled_share_per_cascade": [round(int(c) / m.grid_size ** 3, 4) for c in culled.cpu()],
            "cell_camera_tests_per_s": round(cells * N_CAMS / (us * 1e-6), 0)}


def _state(m):
    return [(getattr(m, f"density_grid_{i}").clone(), getattr(m, f"density_bitfield_{i}").clone())
            for i in range(m.size)]


def _restore(m, state):
    set_bitfields(m, [b for _, b in state])
    with torch.no_grad():
        for i, (g, _) in enumerate(state):
            getattr(m, f"density_grid_{i}").copy_(g)


def update_ab(poses, culled_grid, rounds):
    K, scale = SHAPES["c5"]
    m = MNGP(scale, size=K, seed=3).to("cuda")
    C, G3 = m.cascades, m.grid_size ** 3
    if culled_grid:
        m.mark_invisible_cells(ring_intrinsics(RES), poses, (RES, RES))
    else:
        m.count_grid = torch.ones(C, G3, device="cuda")     # routes to the new entry; not read
    count = m.count_grid
    m.update_density_grid(THR, warmup=True, seed=1)
    state = _state(m)
    culled_share = float(torch.stack([g < 0 for g, _ in state]).float().mean())
    nb = K * C * G3 // 1024

    def one(entry, warmup, seed):
        _restore(m, state)
        m.count_grid = count if entry == "new" else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        du = m.update_density_grid(THR, warmup=warmup, seed=seed)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), int(du["blk"][2 * nb + 1])

    out = {"what": "update", "shape": "c5", "K": K, "scale": scale, "cascades": C,
           "grid": "culled by the ring" if culled_grid else "unculled",
           "culled_share": round(culled_share, 4), "cells": K * C * G3, "rounds": rounds}
    for warmup in (True, False):
        ts, listed = {"old": [], "new": []}, {}
        for e in ("old", "new"):
            one(e, warmup, 5)                               # warm both entries up
        for r in range(rounds):
            for e in (("old", "new") if r % 2 == 0 else ("new", "old")):
                t, n = one(e, warmup, 100 + r)
                ts[e].append(t)
                listed[e] = n
        leg = "warmup" if warmup else "sampled"
        for e in ("old", "new"):
            out[f"{leg}_{e}_ms"] = round(float(np.median(ts[e])), 4)
            out[f"{leg}_{e}_min_ms"] = round(float(np.min(ts[e])), 4)
            out[f"{leg}_{e}_spread_ms"] = round(float(np.max(ts[e]) - np.min(ts[e])), 4)
            out[f"{leg}_{e}_listed_cells"] = listed[e]
        out[f"{leg}_new_over_old"] = round(out[f"{leg}_new_ms"] / out[f"{leg}_old_ms"], 4)
    m.count_grid = count
    return out


def marched(cull, steps=256, res=200, B=8192):
    from sample_step import make_images
    K, scale = SHAPES["c5"]
    dirs, poses = (t.to("cuda") for t in ring_cameras(N_CAMS, res))
    u8 = make_images(N_CAMS, res).to("cuda")
    m, g = MNGP(scale, size=K, seed=3).to("cuda"), Ray_Gate(K, seed=4).to("cuda")
    kw = dict(intrinsics=ring_intrinsics(res), cull_invisible=True) if cull else {}
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, directions=dirs, poses=poses,
                 img_wh=(res, res), images=u8, seed=1, **kw)
    samples = []
    for s in range(steps + 16):
        tr.step_sampled()
        if s >= steps:
            samples.append(tr.renderer.ws.n_samples())
    bits = torch.stack([getattr(m, f"density_bitfield_{i}") for i in range(K)])
    occupied = int(sum(int(torch.bitwise_and(bits >> j, 1).sum()) for j in range(8)))
    return {"what": "marched", "shape": "c5", "K": K, "scale": scale, "rays": B,
            "cull_invisible": cull, "steps": steps,
            "culled_share": None if tr.n_culled is None else
            round(int(tr.n_culled.sum()) / (m.cascades * m.grid_size ** 3), 4),
            "samples_per_step_mean_of_16": round(float(np.mean(samples)), 1),
            "occupied_bits": occupied}


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = argv[argv.index("--out") + 1] if "--out" in argv else \
        os.path.join(ROOT, "profiles", "visibility", "visibility_step.jsonl")
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 10
    if not torch.cuda.is_available():
        raise SystemExit("visibility_step.py measures on the GPU; no device found")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    poses = ring_cameras(N_CAMS, RES)[1].to("cuda")
    jobs = [lambda: mark_alone("c3", poses), lambda: mark_alone("c5", poses),
            lambda: update_ab(poses, False, rounds), lambda: update_ab(poses, True, rounds)]
    if "--skip-marched" not in argv:
        jobs += [lambda: marched(False), lambda: marched(True)]
    for job in jobs:
        line = json.dumps(job())
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()
