"""GPU worker of tests/test_gpu_resume_dp.py (not a test module): one rank of a
two-rank run on ONE GPU over gloo, as tests/train_worker.py.  tests/
resume_ref.py's set-up, deterministic, scale 0.5, K = 2, pose refinement on.

  U  the uninterrupted run: 10 sampled steps, the picks of steps 5..9 kept;
  B  fit_resumable(1, 5, ckpt_dir=argv[2]) on both ranks: rank 0 alone writes the file
     (a rank that saved has a background saver; rank 1 must have none);
  C  a trainer built on models with other seeds: both ranks load that file
     and take 5 more steps.

(The barrier between the write and the load belongs to this worker: rank 1
must not look for the file before rank 0 has put it there.  Saving itself
involves no collective.)  At the end the ranks exchange SHA-256 digests of
their parameters, Adam moments, grids and picks, and rank 0 writes the result
to argv[1]."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import resume_ref as RR  # noqa: E402
from radnerf_amd import dist as rdist  # noqa: E402
from radnerf_amd import train_state as TS  # noqa: E402

CUT, STOP, K, SCALE, EXT = 5, 10, 2, 0.5, True


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(tr, stop):
    """steps up to `stop`; per step the digest of this rank's picks"""
    picks = []
    while tr.global_step < stop:
        tr.step_sampled()
        b = tr.last_batch
        picks.append(digest(torch.stack([b["img_idxs"], b["pix_idxs"]])))
    return picks


def main(out_path, ckpt_dir):
    rank, _, world = rdist.init(backend="gloo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    u = RR.trainer(dev, K, SCALE, EXT)
    want_picks = run(u, STOP)[CUT:]
    want = {k: digest(v) for k, v in RR.full_state(u).items() if not k.startswith("generators")}
    del u
    b = RR.trainer(dev, K, SCALE, EXT)
    b.fit_resumable(1, CUT, ckpt_dir=ckpt_dir)      # one epoch at lr0: U's first five steps
    state_path = os.path.join(ckpt_dir, TS.checkpoint_name(1))
    saved_here = b._saver is not None
    del b
    dist.barrier()
    c = RR.other_trainer(dev, K, SCALE, EXT)
    c.load_state(state_path)
    loaded_step = c.global_step
    picks = run(c, STOP)
    torch.cuda.synchronize()
    mine = {k: digest(v) for k, v in RR.full_state(c).items() if not k.startswith("generators")}
    report = {"rank": rank, "state": mine, "picks": picks, "picks_equal": picks == want_picks,
              "n_picks": len(picks), "equals_uninterrupted": mine == want,
              "loaded_step": loaded_step, "saved_here": saved_here, "world_in_file":
              TS.read_file(state_path)["structure"]["world_size"]}
    allr = [None] * world
    dist.all_gather_object(allr, report)
    if rank == 0:
        moments = [k for k in mine if k.startswith("optimizer/")]
        params = [k for k in mine if k.startswith(("model/", "poses/", "derived/"))]
        res = {"world": world, "saved_here": [a["saved_here"] for a in allr],
               "files": sorted(os.listdir(ckpt_dir)),
               "params_equal": all(a["state"][k] == mine[k] for a in allr for k in params),
               "moments_equal": all(a["state"][k] == mine[k] for a in allr for k in moments),
               "n_params": len(params), "n_moments": len(moments),
               "picks_equal": [a["picks_equal"] for a in allr],
               "n_picks": [a["n_picks"] for a in allr],
               "ranks_differ_in_picks": allr[0]["picks"] != allr[1]["picks"],
               "equals_uninterrupted": [a["equals_uninterrupted"] for a in allr],
               "loaded_step": [a["loaded_step"] for a in allr],
               "world_in_file": [a["world_in_file"] for a in allr]}
        with open(out_path, "w") as f:
            json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
