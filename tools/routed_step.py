"""Whole-step cost of routed training on the fused chain (dev tool, GPU):
train_step (render, fused loss, backward) with no per-launch events, four legs
interleaved round by round in one process (as tools/deterministic_step.py), a
device synchronise around the timed steps; one JSON line per shape with the
median and range of the ms per step and, beside each time, the fraction of the
(ray, sub-NeRF) pairs that are live and of the dense step's samples that are
marched.

  dense     the default step;
  all_live  the routed launches with every pair live (_route_always: the
            selection on the gate's stream, the march waiting for it, the list
            march, the routing backward, the routed loss) -- their overhead;
  top2      gate_topk=2;
  top1      gate_topk=1.

The gate is an untrained Ray_Gate, so which sub-NeRF a ray goes to is
arbitrary; the fractions say how the work was shared out.

Shapes: C3 (K = 2, 8192 rays, scale 0.5) and C5's per-GPU shape (K = 8, 8192
rays, scale 16, exp step 1/256).

With --ab PARENT_TREE it runs the default-path A/B of tools/steptime.py
instead (bench.py of this tree and of a checkout
of the parent commit with its own library, alternating per round) into
profiles/routed/ab_default.txt (--ab-out FILE).

usage: python tools/routed_step.py [c3] [c5] [--out FILE]
       (FILE, appended to: profiles/routed/routed_step.jsonl)
       python tools/routed_step.py --ab PARENT_TREE [--ab-out FILE] [--ab-rounds N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd.fused import FusedMLRenderer  # noqa: E402
from steptime import ab_main, append_jsonl, interleaved_ms  # noqa: E402

SHAPES = {"c3": (2, 8192, 0.5), "c5": (8, 8192, 16.0)}
LAMBDAS = dict(lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3)
LEGS = {"dense": {}, "all_live": {}, "top2": dict(gate_topk=2), "top1": dict(gate_topk=1)}


def run(name, steps=10, rounds=6):
    K, B, scale = SHAPES[name]
    dev = torch.device("cuda")
    sc = S.bench_scene(K, B, scale, dev)
    m, g, o, d, nz, bg, esf = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.bg, sc.esf
    gg, mg, ag = sc.grid_grad, sc.mlp_grad, sc.gate_grad
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    rs = {k: FusedMLRenderer(m, g, B) for k in LEGS}
    rs["all_live"]._route_always = True

    def step(k):
        rs[k].train_step(o, d, d, target, nz, bg, exp_step_factor=esf, grid_grad=gg, mlp_grad=mg,
                         gate_grad=ag, **LAMBDAS, **LEGS[k])

    times = interleaved_ms({k: (lambda k=k: step(k)) for k in rs}, steps, rounds)
    dense_samples = rs["dense"].ws.n_samples()
    out = {"shape": name, "K": K, "rays": B, "scale": scale, "steps": steps, "rounds": rounds - 1,
           "dense_samples": dense_samples, "legs": {}}
    for k, r in rs.items():
        routed = r._routed is not None
        leg = {**times[k], "routed_launches": routed, "scatter_mode": r.scatter_mode,
               "live_pairs": (float(r.ws.route_buffers()["count"].sum()) / (B * K)
                              if routed else 1.0),
               "live_samples": round(r.ws.n_samples() / max(dense_samples, 1), 4)}
        if routed:
            leg["route_count"] = r.ws.route_buffers()["count"].tolist()
        leg["ms_over_dense"] = round(leg["ms"] / times["dense"]["ms"], 4)
        out["legs"][k] = leg
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--ab" in args:
        ab_main(args, os.path.join(ROOT, "profiles", "routed", "ab_default.txt"))
        sys.exit(0)
    dest = os.path.join(ROOT, "profiles", "routed", "routed_step.jsonl")
    if "--out" in args:
        i = args.index("--out")
        dest = args[i + 1]
        del args[i:i + 2]
    for name in args or ["c3", "c5"]:
        append_jsonl(dest, run(name))
        torch.cuda.empty_cache()
