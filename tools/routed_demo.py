"""What routed training does to a model (dev tool / evidence, GPU).

tools/train_demo.py's scene (the analytic sphere, fresh random rays every
step), K sub-NeRFs, trained four ways from the same initialisation and ray
stream with the importance loss:

  dense            the default step;
  top2             Trainer(gate_topk=2);
  top1             Trainer(gate_topk=1);
  top1_from250     Trainer(gate_topk=1, route_from_step=250).

Each model is then rendered on the same 65,536 held-out rays of the scene by
the training render (FusedMLRenderer.forward, jitter noise 0.5, no gradient),
dense and under its own routing, and scored against the analytic colours
(PSNR).  The gate's histogram over those rays, the share of the rays whose
largest gate is each sub-NeRF, and the smallest and mean largest gate go with
it.  One JSON line, appended to profiles/routed/routed_demo.jsonl.

    python tools/routed_demo.py [steps] [rays] [K] [scale] [--out FILE]
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from radnerf_amd.fused import FusedMLRenderer  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.trainer import Trainer  # noqa: E402
from train_demo import batch  # noqa: E402

WAYS = {"dense": {}, "top2": dict(gate_topk=2), "top1": dict(gate_topk=1),
        "top1_from250": dict(gate_topk=1, route_from_step=250)}
EDGES = [0.0, 1e-3, 1e-2, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0]
EVAL_RAYS, EVAL_CHUNK = 65536, 8192


def psnr(mse):
    return round(-10 * math.log10(max(mse, 1e-12)), 2)


def evaluate(m, g, dev, scale, routing):
    """PSNR of the training render on held-out rays, dense and under `routing`"""
    esf = 1 / 256 if scale > 0.5 else 0.0
    bgv = 1.0 if scale <= 0.5 else 0.0
    bg = torch.full((3,), bgv, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    r = FusedMLRenderer(m, g, EVAL_CHUNK)
    nz = torch.full((m.size, EVAL_CHUNK), 0.5, device=dev)
    sse = {"dense": 0.0, "routed": 0.0}
    gates, live = [], 0
    with torch.no_grad():
        for _ in range(EVAL_RAYS // EVAL_CHUNK):
            o, d, target = batch(gen, EVAL_CHUNK, dev, bgv)
            for name, kw in (("dense", {}), ("routed", routing)):
                rgb, _, _, gate, _ = r.forward(o, d, d, nz, bg, exp_step_factor=esf, **kw)
                sse[name] += float(((rgb - target) ** 2).sum())
                if name == "routed" and r._routed is not None:
                    live += int(r.ws.route_buffers()["count"].sum())
            gates.append(gate.clone())
    gate = torch.cat(gates)
    n = EVAL_RAYS * 3
    hist = torch.histc(gate.clamp(0, 1), bins=1000, min=0, max=1)
    cum = torch.cumsum(hist, 0)
    at = lambda e: 0 if e <= 0 else int(cum[min(999, int(round(e * 1000)) - 1)])
    top = gate.argmax(1)
    return {"psnr_dense": psnr(sse["dense"] / n), "psnr_routed": psnr(sse["routed"] / n),
            "live_pairs": round(live / (EVAL_RAYS * m.size), 4) if routing else 1.0,
            "gate_hist": {f"{a:g}-{b:g}": at(b) - at(a) for a, b in zip(EDGES[:-1], EDGES[1:])},
            "top1_share": [round(float((top == i).float().mean()), 4) for i in range(m.size)],
            "gate_min": float(gate.min()), "mean_largest_gate": round(float(gate.max(1)[0].mean()), 4)}


def train(way, steps, B, K, scale, dev):
    torch.manual_seed(0)
    m = MNGP(scale, size=K, seed=3).to(dev)
    g = Ray_Gate(K, seed=4).to(dev)
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, **WAYS[way])
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    tail = []
    torch.cuda.synchronize()
    t0 = time.time()
    for s in range(steps):
        o, d, target = batch(gen, B, dev, 1.0 if scale <= 0.5 else 0.0)
        terms = tr.step(o, d, d, target)
        if s >= steps - 200:
            tail.append(terms["rgb"])
    torch.cuda.synchronize()
    out = {"seconds": round(time.time() - t0, 2),
           "train_psnr_last200": psnr(float(torch.stack(tail).mean()))}
    lf = tr.renderer.last_forward
    if "route_count" in lf:
        out["last_step_route_count"] = lf["route_count"].tolist()
    out.update(evaluate(m, g, dev, scale, tr.routing if WAYS[way] else {}))
    return out


def main():
    args = sys.argv[1:]
    dest = os.path.join(ROOT, "profiles", "routed", "routed_demo.jsonl")
    if "--out" in args:
        i = args.index("--out")
        dest = args[i + 1]
        del args[i:i + 2]
    steps = int(args[0]) if len(args) > 0 else 1000
    B = int(args[1]) if len(args) > 1 else 8192
    K = int(args[2]) if len(args) > 2 else 4
    scale = float(args[3]) if len(args) > 3 else 0.5
    dev = torch.device("cuda")
    res = {"scene": "tools/train_demo.py's sphere, fresh random rays every step; scored on "
                    f"{EVAL_RAYS} held-out rays by the training render",
           "steps": steps, "rays": B, "models": K, "scale": scale, "lambda_cv_importance": 1e-2,
           "ways": {}}
    for way in WAYS:
        res["ways"][way] = train(way, steps, B, K, scale, dev)
        print(way, json.dumps(res["ways"][way]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
