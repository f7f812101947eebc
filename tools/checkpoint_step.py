"""What a checkpoint costs the training loop (dev tool, GPU): sampled steps
(Trainer.step_sampled) at C3 (K = 2, 8192 rays, scale 0.5) and C5's per-GPU
shape (K = 8, 8192 rays, scale 16), the models, gate and occupancy bitfields
built as bench.py builds them (MNGP(seed=3), Ray_Gate(seed=4),
synthetic.bitfields(p=0.5, seed=1)), a small device-resident training set of
ring cameras around the box, in three settings, one after another in one
process:

  nosave      the steps alone;
  blocking    Trainer.save_state(path) every `--every` steps;
  background  Trainer.save_state(path, background=True) every `--every` steps
              (staging copy on the training stream, pinned host copy on a side
              stream, checksums and the file from the writer thread); the last
              write is waited for after the loop and reported as drain_ms.

Each setting runs `--steps` steps in segments of 10 with a device synchronise
around each segment; a save falls between two segments and is timed with
them.  Per setting: the median step (median segment / 10) and the loop's total
time; from the totals, the time one checkpoint adds to the loop ((total -
nosave total) / saves), which for the background save includes whatever the
copy and the writer thread take from the following steps and any wait of a
save for the one before it.  The grid updates are held off (they would
rewrite bench.py's bitfields from the untrained networks), so a step is the
sampled step alone.  One JSON line per shape, with the file's size.

With --ab PARENT_TREE (a checkout of the parent commit with its own built
library) it instead runs the default-path A/B: bench.py of this tree (new) and
of that tree (old) as child processes, alternating per round, C3 and C5, and
writes the figures to profiles/checkpoint/ab_default.txt (--ab-out FILE).

usage: python tools/checkpoint_step.py [c3] [c5] [--steps N] [--every N] [--dir DIR] [--out FILE]
       (FILE, appended to: profiles/checkpoint/checkpoint_step.jsonl)
       python tools/checkpoint_step.py --ab PARENT_TREE [--ab-out FILE]
"""
import math
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402

from steptime import ab_main, append_jsonl  # noqa: E402

SHAPES = {"c3": (2, 8192, 0.5), "c5": (8, 8192, 16.0)}
SEG = 10
N_IMG, RES = 16, 64


def cameras(scale):
    """directions (RES^2, 3) and N_IMG ring poses looking at the box's centre
    from 3 x scale: the frustum spans the box"""
    import torch
    half = 0.3
    y, x = torch.meshgrid(torch.linspace(-half, half, RES), torch.linspace(-half, half, RES),
                          indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(RES * RES)], -1)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    ang = torch.arange(N_IMG) * (2 * math.pi / N_IMG) + 0.3
    pos = 3.0 * scale * torch.stack([torch.cos(ang), torch.sin(ang), 0.3 * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2).contiguous()
    return dirs, poses


def make_trainer(name, dev):
    import torch
    from radnerf_amd import synthetic as S
    from radnerf_amd.trainer import Trainer
    K, B, scale = SHAPES[name]
    sc = S.bench_scene(K, B, scale, dev)
    m, g = sc.m, sc.g
    dirs, poses = cameras(scale)
    u8 = torch.randint(0, 256, (N_IMG, RES * RES, 3), dtype=torch.uint8,
                       generator=torch.Generator().manual_seed(7))
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3,
                 directions=dirs.to(dev), poses=poses.to(dev), images=u8.to(dev), seed=1,
                 update_interval=1 << 40)
    tr.global_step = 1          # no grid update: the bitfields stay bench.py's
    return tr


def loop(tr, steps, every, save):
    """`steps` steps in segments of SEG, save() after every `every` steps;
    (segment ms, save-call ms, total ms)"""
    import torch
    segs, calls = [], []
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for s in range(0, steps, SEG):
        t0 = time.perf_counter()
        for _ in range(SEG):
            tr.step_sampled()
        torch.cuda.synchronize()
        segs.append((time.perf_counter() - t0) * 1e3)
        if save is not None and (s + SEG) % every == 0:
            t0 = time.perf_counter()
            save()
            calls.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return segs, calls, (time.perf_counter() - t_all) * 1e3


def run(name, steps, every, where):
    import torch
    dev = torch.device("cuda")
    tr = make_trainer(name, dev)
    K, B, scale = SHAPES[name]
    path = os.path.join(where, f"checkpoint_step_{name}.pt")
    loop(tr, 5 * SEG, every, None)                              # warm-up
    out = {"shape": name, "K": K, "rays": B, "scale": scale, "steps": steps, "save_every": every,
           "samples": tr.renderer.ws.n_samples(), "scatter_mode": tr.renderer.scatter_mode}
    settings = {"nosave": None, "blocking": lambda: tr.save_state(path),
                "background": lambda: tr.save_state(path, background=True)}
    for k, save in settings.items():
        if save is not None:                                    # buffers and the file exist
            save()
            tr.wait_saves()
        segs, calls, total = loop(tr, steps, every, save)
        res = {"median_step_ms": round(float(np.median(segs)) / SEG, 4),
               "total_ms": round(total, 2)}
        if save is not None:
            res["saves"] = len(calls)
            res["save_call_ms"] = [round(c, 2) for c in calls]
            t0 = time.perf_counter()
            tr.wait_saves()
            res["drain_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        out[k] = res
    out["file_bytes"] = os.path.getsize(path)
    for k in ("blocking", "background"):
        out[k]["added_per_checkpoint_ms"] = round(
            (out[k]["total_ms"] - out["nosave"]["total_ms"]) / max(1, out[k]["saves"]), 2)
    out["background_adds_less"] = (out["background"]["added_per_checkpoint_ms"]
                                   < out["blocking"]["added_per_checkpoint_ms"])
    os.unlink(path)
    return out


def _opt(args, flag, default, kind=str):
    if flag in args:
        i = args.index(flag)
        val = kind(args[i + 1])
        del args[i:i + 2]
        return val
    return default


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--ab" in args:
        ab_main(args, os.path.join(ROOT, "profiles", "checkpoint", "ab_default.txt"))
        sys.exit(0)
    dest = _opt(args, "--out",
                os.path.join(ROOT, "profiles", "checkpoint", "checkpoint_step.jsonl"))
    steps, every = _opt(args, "--steps", 300, int), _opt(args, "--every", 100, int)
    where = _opt(args, "--dir", None)
    import torch
    tmp = where or tempfile.mkdtemp()
    try:
        for name in args or ["c3", "c5"]:
            append_jsonl(dest, run(name, steps, every, tmp))
            torch.cuda.empty_cache()
    finally:
        if where is None:
            shutil.rmtree(tmp, ignore_errors=True)
