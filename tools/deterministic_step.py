"""Whole-step cost of the deterministic mode on the fused chain (dev tool,
GPU): train_step (render, fused loss, backward) with no per-launch events,
three forms interleaved round by round in one process (as
tools/distortion_step.py), a device synchronise around the timed steps; one
JSON line per shape with the median ms per step.

  default   the default step (fixed-point / binned grid scatter, fp32 atomics
            for dW, the gate's dW and importance and the loss terms);
  intgrad   the default step with int_grad = True alone (exact integer grid
            gradient on the ticket queue, everything else as default);
  det       FusedMLRenderer(deterministic=True): the integer grid form on the
            static chunk schedule with per-block dW slots, the ordered
            reductions, the ordered importance and loss sums.

Then a few traced steps of `det` give the added launches' event spans
(seed_scale, dw_reduce, igrad_to_f32 on the main stream; gate_colsum and
gate_reduce on the gate's side stream, where a span includes the wait for a CU
beside the persistent field_bwd blocks) next to field_bwd and gate_bwd of
`det` and of `default`; and the added kernels and the two loss entries are
timed alone on an idle device (`alone_ms`), which is their own cost.

Shapes: C3 (K = 2, 8192 rays, scale 0.5) and C5's per-GPU shape (K = 8, 8192
rays, scale 16, exp step 1/256).

With --ab PARENT_TREE (a checkout of the parent commit with its own built
library) it instead runs the default-path A/B: `bench.py` of this tree (new)
and of that tree (old) as child processes, alternating per round, C3 and C5,
and writes the interleaved figures to profiles/deterministic/ab_default.txt
(--ab-out FILE), with one more --dump-outputs run of each compared array by
array.  (The parent's library cannot be loaded by this tree's binding, which
refuses a library without the new entries, so each side runs its own tree.)

usage: python tools/deterministic_step.py [c3] [c5] [--out FILE]
       (FILE, appended to: profiles/deterministic/deterministic_step.jsonl)
       python tools/deterministic_step.py --ab PARENT_TREE [--ab-out FILE]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd._lib import lib  # noqa: E402
from radnerf_amd.fused import FusedMLRenderer  # noqa: E402
from radnerf_amd.losses import fused_nerf_loss  # noqa: E402
from steptime import ab_main, alone_ms, append_jsonl, interleaved_ms  # noqa: E402

SHAPES = {"c3": (2, 8192, 0.5), "c5": (8, 8192, 16.0)}
LAMBDAS = dict(lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3)
ADDED_MAIN = ("seed_scale", "dw_reduce", "igrad_to_f32")
ADDED_SIDE = ("gate_colsum", "gate_reduce")
TRACED = ADDED_MAIN + ADDED_SIDE + ("field_bwd", "gate_bwd", "gate_fwd")


def _median(x):
    return round(float(np.median(x)), 4)


def run(name, steps=10, rounds=6):
    K, B, scale = SHAPES[name]
    dev = torch.device("cuda")
    sc = S.bench_scene(K, B, scale, dev)
    m, g, o, d, nz, bg, esf = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.bg, sc.esf
    gg, mg, ag = sc.grid_grad, sc.mlp_grad, sc.gate_grad
    target = torch.rand(B, 3, generator=torch.Generator().manual_seed(7)).to(dev)
    rs = {"default": FusedMLRenderer(m, g, B), "intgrad": FusedMLRenderer(m, g, B),
          "det": FusedMLRenderer(m, g, B, deterministic=True)}
    rs["intgrad"].int_grad = True

    def step(r):
        r.train_step(o, d, d, target, nz, bg, exp_step_factor=esf, grid_grad=gg, mlp_grad=mg,
                     gate_grad=ag, **LAMBDAS)

    times = interleaved_ms({k: (lambda r=r: step(r)) for k, r in rs.items()}, steps, rounds)
    out = {"shape": name, "K": K, "rays": B, "scale": scale,
           "samples": rs["det"].ws.n_samples(), "steps": steps, "rounds": rounds - 1,
           "scatter_mode": {k: r.scatter_mode for k, r in rs.items()},
           "merged_blocks": rs["det"].merged_blocks, "chunks": int(rs["det"].ws.queue[1]),
           "dw_part_bytes": rs["det"].ws.dw_part.numel() * 4,
           "gate_part_bytes": 0 if K == 1 else rs["det"].ws.gate_part.numel() * 4}
    for k, t in times.items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    # the launches' own times (events around each, so the step itself is slower)
    for k in ("default", "det"):
        r = rs[k]
        r.trace, r.events = set(TRACED), {}
        for _ in range(steps):
            step(r)
        ms = r.kernel_times_ms()
        r.trace, r.events = False, {}
        out[k + "_launch_ms"] = {n: _median(v) for n, v in sorted(ms.items())}
    out["added_main_stream_ms"] = round(
        sum(out["det_launch_ms"].get(n, 0.0) for n in ADDED_MAIN), 4)
    # the added kernels and the loss entries alone on an idle device
    r = rs["det"]
    w, L = r.ws, lib()
    rgb, opacity, depth, gate, imp = r.forward(o, d, d, nz, bg, 1e-4, esf)
    st = torch.cuda.current_stream(dev).cuda_stream
    alone = {
        "dw_reduce": lambda: L.reduce_partials(w.dw_part.data_ptr(), w.dw_part.shape[0],
                                               w.dw_part.shape[1], mg.data_ptr(), st),
        "loss_default": lambda: fused_nerf_loss(rgb, target, opacity, depth, gate, imp,
                                                **LAMBDAS),
        "loss_det": lambda: fused_nerf_loss(rgb, target, opacity, depth, gate, imp,
                                            deterministic=True, **LAMBDAS),
    }
    if K > 1:
        alone["gate_reduce"] = lambda: L.reduce_partials(
            w.gate_part.data_ptr(), w.gate_part.shape[0], w.gate_part.shape[1], ag.data_ptr(), st)
        alone["gate_colsum"] = lambda: L.colsum_ordered(gate.data_ptr(), B, K, imp.data_ptr(), st)
    out["alone_ms"] = {k: alone_ms(fn, steps, 2) for k, fn in alone.items()}
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--ab" in args:
        ab_main(args, os.path.join(ROOT, "profiles", "deterministic", "ab_default.txt"))
        sys.exit(0)
    dest = os.path.join(ROOT, "profiles", "deterministic", "deterministic_step.jsonl")
    if "--out" in args:
        i = args.index("--out")
        dest = args[i + 1]
        del args[i:i + 2]
    for name in args or ["c3", "c5"]:
        append_jsonl(dest, run(name))
        torch.cuda.empty_cache()
