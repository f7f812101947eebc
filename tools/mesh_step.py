"""Cost of the mesh export (dev tool, GPU), one JSON line per (model, lattice):

  (a) mesh.density_lattice (rn_density_lattice: one launch, points from the
      lattice index, one encode per point for all sub-NeRFs) against the
      composition it replaces: a torch-made xyz buffer in chunks of 2^22
      points, model.density per sub-NeRF, a torch weighted sum -- the two
      forms interleaved round by round (tools/steptime.py);
  (b) mesh.surface_nets on two lattices of that size -- an analytic sphere
      (a surface as a trained model has it: V ~ n^2) and the synthetic model's
      own lattice at its median (noise: a vertex in most cells, the worst
      case) -- in ms and in bytes of lattice per second, beside a
      device-to-device copy of the same lattice timed in the same run;
  (c) V, F and the workspace's size.

Models: C3 (K = 2, scale 0.5) and K = 8 at scale 16, synthetic weights
(synthetic.parity_scene).  `--ab PARENT_TREE`: bench.py of this tree against
the parent's (steptime.ab_main) -> profiles/mesh/ab_default.txt.

usage: python tools/mesh_step.py [--out FILE] [--res 256,512] [--rounds N]
       python tools/mesh_step.py --ab PARENT_TREE
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from steptime import ab_main, append_jsonl, interleaved_ms  # noqa: E402

SHAPES = {"c3": (2, 0.5), "k8s16": (8, 16.0)}
CHUNK = 1 << 22


def composed_lattice(model, n, out):
    """the lattice as it could be made before rn_density_lattice"""
    dev = out.device
    lo = model._h_min
    step = (model._h_ext / np.float32(n)).astype(np.float32)
    px = n + 1
    flat = out.view(-1)
    w = 1.0 / model.size
    for a in range(0, flat.numel(), CHUNK):
        p = torch.arange(a, min(a + CHUNK, flat.numel()), device=dev)
        i, j, k = p % px, (p // px) % px, p // (px * px)
        xyz = torch.stack([i.float() * float(step[0]) + float(lo[0]),
                           j.float() * float(step[1]) + float(lo[1]),
                           k.float() * float(step[2]) + float(lo[2])], 1)
        acc = None
        for q in range(model.size):
            s = model.density(xyz, ind=q)
            acc = w * s if acc is None else acc + w * s
        flat[a:a + len(p)] = acc
    return out


def sphere_lattice(n, dev):
    ax = torch.arange(n + 1, device=dev, dtype=torch.float32) * (2.0 / n) - 1.0
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    r2 = (x - 0.07) ** 2 + (y + 0.11) ** 2 + (z - 0.05) ** 2
    return (20.0 * torch.exp(-3.0 * r2 / 0.36)).contiguous()


def run(shape, n, rounds):
    from radnerf_amd import mesh
    from radnerf_amd import synthetic as S
    K, scale = SHAPES[shape]
    dev = torch.device("cuda")
    with torch.no_grad():
        m = S.parity_scene(K, scale=scale, device=dev).m
        pts = (n + 1) ** 3
        rec = {"shape": shape, "K": K, "scale": scale, "resolution": n, "points": pts,
               "lattice_bytes": 4 * pts}
        buf = torch.empty(n + 1, n + 1, n + 1, device=dev)
        holder = {}

        def fused():
            holder["s"] = mesh.density_lattice(m, n)

        t = interleaved_ms({"lattice": fused, "composed": lambda: composed_lattice(m, n, buf)},
                           1, rounds)
        rec["equal"] = bool(torch.equal(holder["s"], buf))
        rec["lattice_ms"], rec["lattice_range_ms"] = t["lattice"]["ms"], t["lattice"]["range_ms"]
        rec["composed_ms"], rec["composed_range_ms"] = t["composed"]["ms"], t["composed"]["range_ms"]
        rec["points_per_s"] = round(pts / (t["lattice"]["ms"] * 1e-3), 1)
        # ---- extraction
        box = (m._h_min, m._h_min + m._h_ext)
        lattices = {"sphere": (sphere_lattice(n, dev), float(20.0 * np.exp(-3.0)),
                               ((-1.0,) * 3, (1.0,) * 3)),
                    "model": (holder["s"], float(holder["s"].view(-1)[::7].median()), box)}
        rec["work_bytes"] = mesh.surface_work_bytes(n)
        for name, (sig, iso, aabb) in lattices.items():
            dst = torch.empty_like(sig)
            out = {}

            def extract():
                out["m"] = mesh.surface_nets(sig, iso, aabb)

            t = interleaved_ms({"extract": extract, "copy": lambda: dst.copy_(sig)}, 3, rounds)
            ms = t["extract"]["ms"]
            rec[name] = {"iso": round(iso, 6), "V": int(out["m"].vertices.shape[0]),
                         "F": int(out["m"].faces.shape[0]), "extract_ms": ms,
                         "extract_range_ms": t["extract"]["range_ms"],
                         "lattice_GB_per_s": round(4 * pts / (ms * 1e-3) / 1e9, 2),
                         "copy_ms": t["copy"]["ms"], "copy_range_ms": t["copy"]["range_ms"],
                         "copy_GB_per_s": round(4 * pts / (t["copy"]["ms"] * 1e-3) / 1e9, 2)}
            del dst, out
        return rec


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--ab" in args:
        ab_main(args, os.path.join(ROOT, "profiles", "mesh", "ab_default.txt"))
        sys.exit(0)
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    dest = opt("--out", os.path.join(ROOT, "profiles", "mesh", "mesh_step.jsonl"))
    for shape in opt("--shapes", "c3,k8s16").split(","):
        for n in (int(x) for x in opt("--res", "256,512").split(",")):
            append_jsonl(dest, run(shape, n, int(opt("--rounds", "4"))))
            torch.cuda.empty_cache()
