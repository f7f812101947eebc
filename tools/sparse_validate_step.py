"""Cost and error of the gate-sparse test-time render (dev tool, GPU).

One 800 x 800 view per configuration through ImageEvaluator.render_image:

  synthetic  C3 (K = 2, scale 0.5) and C5's branch (K = 8, scale 16), synthetic
             weights and gate as tools/validate_step.py: the dense render;
             gate_min at the 25 / 50 / 75 / 90 % quantiles of that image's gate
             values; gate_topk 1 and 2 (2 only where K > 2); and the sparse chain
             forced with every pair live (this tool's FORCE switch: gate_min 0,
             gate_topk K sent through rn_gate_select and rn_render_test_list),
             which isolates the cost of the selection and of the list
             indirection;
  trained    models trained here as tools/train_demo.py does (1000 steps on its
             sphere scene; C3, and K = 4 at scale 16): dense, gate_min 1e-4 /
             1e-3 / 1e-2 and gate_topk 1, with the PSNR of the sparse image
             against the dense one and the difference of their PSNRs against
             the analytic ground truth where the camera allows it.

The runs of one model are interleaved round by round in one process (as
tools/validate_step.py), a device synchronise around the timed images; one JSON
line per run: median ms per image, live pairs / all pairs, the selection's own
time (rn_gate_select alone on one chunk's gate, events around 20 calls), the
largest |d rgb| against the dense image next to the largest dead gate mass, and
whether every ray is inside the bound mass (1 + 2^-20) + K 2^-23.

usage: python tools/sparse_validate_step.py [--out FILE] [--res N] [--only synthetic|trained]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radnerf_amd import layout as LY  # noqa: E402
from radnerf_amd import sparse_gate  # noqa: E402
from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd.evaluate import ImageEvaluator  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.synthetic import ring_cameras  # noqa: E402
from radnerf_amd.trainer import Trainer  # noqa: E402
from steptime import append_jsonl, interleaved_ms  # noqa: E402
from train_demo import batch  # noqa: E402

FORCE = "forced-all-live"


def synthetic_model(K, scale, dev):
    m, g = MNGP(scale, size=K, seed=3), Ray_Gate(K, seed=4)
    S.set_bitfields(m, S.bitfields(K, m.cascades, p=0.5, seed=1))
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(K, LY.FIELD_PARAMS)))
    return m.to(dev), g.to(dev)


def trained_model(K, scale, dev, steps=1000, B=8192):
    """tools/train_demo.py's run(), keeping the model"""
    torch.manual_seed(0)
    m, g = MNGP(scale, size=K, seed=3).to(dev), Ray_Gate(K, seed=4).to(dev)
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    for _ in range(steps):
        o, d, target = batch(gen, B, dev, 1.0 if scale <= 0.5 else 0.0)
        tr.step(o, d, d, target)
    torch.cuda.synchronize()
    return m, g


def select_us(gate, kw):
    """rn_gate_select alone on one chunk's gate rows"""
    n = min(gate.shape[0], 1 << 18)
    rows = gate[:n].contiguous()
    out = sparse_gate.select(rows, **kw)
    out["work"] = torch.empty(1 << 16, dtype=torch.uint8, device=gate.device)
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            sparse_gate.select(rows, out=out, **kw)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / 20)
    return round(float(np.median(ts)), 2), n


def measure(tag, m, g, K, scale, radius, runs_of, res, rounds=4, steps=2, gt_of=None):
    """runs_of(gate) -> {name: keywords}; the first run is the dense one"""
    dev = m.mlp_params.device
    dirs, poses = (t.to(dev) for t in ring_cameras(4, res, radius=radius))
    pose = poses[1].contiguous()
    ev = ImageEvaluator(m, g, dirs, (res, res))
    dense = {k: v.clone() for k, v in ev.render_image(pose).items()}
    gate = dense["gating_code"]
    runs = runs_of(gate)
    real_is_dense = sparse_gate.is_dense

    def render(kw):
        if kw.get("force"):
            sparse_gate.is_dense = lambda *a: False
        try:
            return ev.render_image(pose, **{k: v for k, v in kw.items() if k != "force"})
        finally:
            sparse_gate.is_dense = real_is_dense

    times = interleaved_ms({k: (lambda kw=kw: render(kw)) for k, kw in runs.items()}, steps, rounds)
    N = gate.shape[0]
    gt = None if gt_of is None else gt_of(dirs, pose)
    psnr = lambda a, b: float(-10 * torch.log10(((a.double() - b.double()) ** 2).mean()))
    lines = []
    for name, kw in runs.items():
        out = {"model": tag, "K": K, "scale": scale, "img_wh": [res, res], "run": name,
               "keywords": {k: v for k, v in kw.items() if k != "force"},
               "ms_per_image": round(times[name]["ms"], 3),
               "spread_ms": [round(x, 3) for x in times[name]["range_ms"]],
               "over_dense": round(times[name]["ms"] / times["dense"]["ms"], 4),
               "rounds": rounds - 1, "images_per_round": steps}
        r = render(kw)
        out["samples"] = int(r["total_samples"])
        if "pairs" in r:
            live = r["gating_live"] != 0
            out["live_pairs"], out["all_pairs"] = int(r["pairs"]), N * K
            out["live_fraction"] = round(int(r["pairs"]) / (N * K), 5)
            # the sub-NeRF with the most live rays: its share of the image's rays
            out["largest_model_share"] = round(int(live.sum(0).max()) / N, 5)
            out["select_us"], out["select_rays"] = select_us(
                gate, {k: v for k, v in kw.items() if k != "force"})
            mass = torch.where(live, 0.0, gate).double().sum(1)
            d_rgb = (r["rgb"].double() - dense["rgb"].double()).abs().amax(1)
            d_op = (r["opacity"].double() - dense["opacity"].double()).abs()
            out["max_abs_d_rgb"], out["max_abs_d_opacity"] = float(d_rgb.max()), float(d_op.max())
            out["max_dead_mass"], out["mean_dead_mass"] = float(mass.max()), float(mass.mean())
            if not kw.get("renormalize"):
                bound = mass * (1 + 2.0 ** -20) + K * 2.0 ** -23
                out["within_bound"] = bool((d_rgb <= bound).all() and (d_op <= bound).all())
            if float(d_rgb.max()) > 0:
                out["psnr_vs_dense"] = round(psnr(r["rgb"], dense["rgb"]), 3)
        else:
            out["live_fraction"] = 1.0
        if gt is not None:
            out["psnr_vs_truth"] = round(psnr(r["rgb"], gt), 4)
            out["psnr_vs_truth_minus_dense"] = round(out["psnr_vs_truth"] - psnr(dense["rgb"], gt), 4)
        lines.append(out)
    return lines


def synthetic_runs(K):
    def runs_of(gate):
        q = torch.quantile(gate.flatten()[:: max(1, gate.numel() // 1000000)],
                           torch.tensor([0.25, 0.5, 0.75, 0.9], device=gate.device))
        runs = {"dense": {}}
        for p, v in zip((25, 50, 75, 90), q.tolist()):
            runs[f"gate_min-q{p}"] = {"gate_min": min(float(v), 0.999)}
        runs["gate_topk-1"] = {"gate_topk": 1}
        if K > 2:                       # at K = 2 it is the dense render
            runs["gate_topk-2"] = {"gate_topk": 2}
        runs[FORCE] = {"gate_min": 0.0, "gate_topk": K, "force": True}
        return runs
    return runs_of


def trained_runs(gate):
    runs = {"dense": {}}
    for tau in (1e-4, 1e-3, 1e-2):
        runs[f"gate_min-{tau:g}"] = {"gate_min": tau}
    runs["gate_topk-1"] = {"gate_topk": 1}
    runs["gate_topk-1-renorm"] = {"gate_topk": 1, "renormalize": True}
    return runs


def sphere_truth(bg):
    """train_demo.batch's analytic target for the camera's own rays"""
    def gt_of(dirs, pose):
        d = dirs @ pose[:, :3].T
        o = pose[:, 3].expand_as(d)
        b = (o * d).sum(1)
        c = (o * o).sum(1) - 0.25 ** 2
        disc = b * b - c
        t = -b - torch.sqrt(disc.clamp_min(0))
        hit = (disc > 0) & (t > 0)
        nrm = o + t[:, None] * d
        nrm = nrm / nrm.norm(dim=1, keepdim=True)
        return torch.where(hit[:, None], 0.5 + 0.5 * nrm, torch.full_like(nrm, bg))
    return gt_of


def main():
    argv = sys.argv[1:]
    path = argv[argv.index("--out") + 1] if "--out" in argv else \
        os.path.join(ROOT, "profiles", "sparse", "sparse_validate_step.jsonl")
    res = int(argv[argv.index("--res") + 1]) if "--res" in argv else 800
    only = argv[argv.index("--only") + 1] if "--only" in argv else None
    dev = torch.device("cuda")

    def emit(lines):
        for l in lines:
            append_jsonl(path, l)

    if only in (None, "synthetic"):
        for tag, K, scale in (("c3-synthetic", 2, 0.5), ("c5-synthetic", 8, 16.0)):
            m, g = synthetic_model(K, scale, dev)
            emit(measure(tag, m, g, K, scale, 3 * scale, synthetic_runs(K), res))
    if only in (None, "trained"):
        for tag, K, scale in (("c3-trained-1000", 2, 0.5), ("s16k4-trained-1000", 4, 16.0)):
            m, g = trained_model(K, scale, dev)
            emit(measure(tag, m, g, K, scale, 1.5, trained_runs, res,
                         gt_of=sphere_truth(1.0 if scale <= 0.5 else 0.0)))


if __name__ == "__main__":
    main()
