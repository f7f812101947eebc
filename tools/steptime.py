"""How the tools/*_step.py cost tools take their times (every step figure in
README.md and DESIGN.md section 4 comes through here), written once:

  interleaved_ms   whole steps of several forms, interleaved round by round;
  alone_ms         one launch on an idle device, events around it;
  ab_bench         bench.py of this tree against a parent tree, alternating;
  append_jsonl     one result line.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ms(x):
    return round(float(x), 4)


def interleaved_ms(forms, steps, rounds, warm=True, sync=torch.cuda.synchronize,
                   clock=time.perf_counter):
    """ms per call of every form of `forms` ({name: callable}), the forms
    interleaved round by round in one process: per round and form one untimed
    call (warm), then `steps` calls between two device synchronises.
    -> {name: {"ms": median over the rounds, "range_ms": [min, max]}}"""
    if rounds < 2:
        raise ValueError("round 0 is discarded: at least 2 rounds")
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k, fn in forms.items():
            if warm:
                fn()                                # warm-up of this form
            sync()
            t0 = clock()
            for _ in range(steps):
                fn()
            sync()
            if rnd:                                 # the first round warms everything up
                times[k].append((clock() - t0) / steps * 1e3)
    return {k: {"ms": _ms(np.median(t)), "range_ms": [_ms(min(t)), _ms(max(t))]}
            for k, t in times.items()}


def alone_ms(fn, n, skip):
    """ms of one call of fn on an idle device (events around it, a device
    synchronise after it): the median of n calls after `skip` untimed ones"""
    ts = []
    for _ in range(skip + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return _ms(np.median(ts[skip:]))


AB_SHAPES = {"c3": ["--steps", "40", "--warmup", "5"],
             "c5": ["--steps", "20", "--warmup", "3", "--models", "8", "--scale", "16",
                    "--rays", "8192"]}


def ab_bench(parent_tree, dest, shapes=AB_SHAPES, rounds=3):
    """The default-path A/B: bench.py of this tree (new) and of `parent_tree`
    (old: a checkout of the parent commit with its own built library, which
    this tree's binding could not load), alternating per round, each run a
    child process of its own (this process never touches the GPU); then one
    --dump-outputs run of each, compared array by array.  Written to `dest`."""
    trees = {"new": ROOT, "old": os.path.abspath(parent_tree)}
    vals = {(c, v): [] for c in shapes for v in trees}
    for _ in range(rounds):
        for v, tree in trees.items():
            for c, extra in shapes.items():
                res = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1"]
                                     + extra, capture_output=True, text=True, timeout=300)
                if res.returncode != 0:
                    raise SystemExit(f"bench.py ({v}, {c}) failed: {res.stderr[-2000:]}")
                d = json.loads(res.stdout.strip().splitlines()[-1])
                vals[(c, v)].append((d["value"], d["ms_per_step"]))
                print(f"{c} {v}: {d['value']:.2f}", file=sys.stderr, flush=True)
    lines = ["# the default step, bench.py --gpus 1 and per shape: "
             + "; ".join(f"{c}: {' '.join(extra)}" for c, extra in shapes.items()),
             "# the parent commit's tree with its own library (old) and this tree (new),",
             "# alternating new / old per round in one job on one MI355X; M samples/s fwd+bwd, "
             "ms per step"]
    for c in shapes:
        for v in ("old", "new"):
            xs = [a for a, _ in vals[(c, v)]]
            lines.append(f"{c} {v}: " + "  ".join(f"{a:.2f} ({b:.4f} ms)" for a, b in vals[(c, v)])
                         + f"  median {np.median(xs):.2f}  spread {min(xs):.2f}-{max(xs):.2f}")
    tmp = tempfile.mkdtemp()
    try:
        for v, tree in trees.items():
            subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
                            "--steps", "5", "--warmup", "2", "--dump-outputs",
                            os.path.join(tmp, v)], capture_output=True, check=True, timeout=300)
        eq = {n[:-4]: bool(np.array_equal(np.load(os.path.join(tmp, "new", n)),
                                          np.load(os.path.join(tmp, "old", n))))
              for n in sorted(os.listdir(os.path.join(tmp, "new")))}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lines.append("# --dump-outputs of one more C3 run each, bitwise equal old vs new (mlp_grad and "
                 "gate_grad are fp32")
    lines.append("# atomics in arrival order, which differ between any two default runs): "
                 + ", ".join(f"{k} {'yes' if e else 'no'}" for k, e in eq.items()))
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def ab_main(args, default_dest):
    """the tools' `--ab PARENT_TREE [--ab-out FILE] [--ab-rounds N]` command line"""
    dest = args[args.index("--ab-out") + 1] if "--ab-out" in args else default_dest
    rounds = int(args[args.index("--ab-rounds") + 1]) if "--ab-rounds" in args else 3
    ab_bench(args[args.index("--ab") + 1], dest, rounds=rounds)


def append_jsonl(path, record):
    """print `record` as one JSON line and append it to `path`"""
    line = json.dumps(record)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")
