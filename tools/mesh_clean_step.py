"""Cost of the mesh clean-up (dev tool, GPU), one JSON line per measurement:

  (a) mesh.components + mesh.filter_components(keep_largest=1), warm, on the
      512^3 sphere's mesh (one component) and on a noise lattice's mesh (many
      components), against the same rounds composed from torch ops on the
      device -- scatter_reduce_('amin') for the hooks, gathers for the jumps, a
      flag read per batch of mesh.LABEL_ROUNDS rounds, boolean-mask compaction
      -- the forms interleaved round by round (tools/steptime.py); with the
      rounds the labelling needs (found by batches of one round), the batches
      and the host synchronisations a call makes;
  (b) mesh.density_lattice at 512^3 with occupancy=True against occupancy=False,
      for C3 (K = 2, scale 0.5) and K = 8 at scale 16, synthetic weights
      (synthetic.parity_scene): bitfields with a ball of occupancy of radius
      0.25 / 0.5 / 0.75 of the box's half-width in every sub-NeRF, and all
      ones; with the share of the lattice's points the ball holds.

`--ab PARENT_TREE`: bench.py of this tree against the parent's
(steptime.ab_main) -> profiles/mesh_clean/ab_default.txt.

usage: python tools/mesh_clean_step.py [--out FILE] [--res 512] [--rounds N] [--only a|b]
       python tools/mesh_clean_step.py --ab PARENT_TREE
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_step import SHAPES, sphere_lattice  # noqa: E402
from steptime import ab_main, append_jsonl, interleaved_ms  # noqa: E402

G = 128


# ---- (a) components and the filter ------------------------------------------------------
def torch_clean(m, rounds, batches):
    """components + filter_components(keep_largest=1) from torch ops, in the
    kernels' shape: the same rounds, one flag read per batch"""
    V = m.vertices.shape[0]
    f = m.faces.long()
    L = torch.arange(V, device=f.device)
    for _ in range(batches):
        for _ in range(rounds):
            l = L[f]
            low = l.min(1, keepdim=True).values.expand(-1, 6).reshape(-1)
            L.scatter_reduce_(0, torch.cat([f, l], 1).reshape(-1), low, "amin")
            L = torch.minimum(L, L[L[L]])
        l = L[f]
        if bool(((l == l[:, :1]).all() & (L[L] == L).all()).item()):     # the batch's sync
            break
    else:
        raise RuntimeError("torch_clean: no fixed point")
    ids = torch.cumsum(L == torch.arange(V, device=f.device), 0) - 1
    label = ids[L]
    nv = torch.bincount(label)
    keep = torch.zeros_like(nv, dtype=torch.bool)
    keep[torch.sort(nv, descending=True, stable=True).indices[:1]] = True
    kv = keep[label]
    new = torch.cumsum(kv, 0) - 1
    kf = kv[f[:, 0]]
    return (m.vertices[kv], new[f[kf]].int(), m.normals[kv])   # the masks synchronise


def run_clean(name, sig, iso, aabb, rounds):
    from radnerf_amd import mesh
    m = mesh.surface_nets(sig, iso, aabb)
    V, F = m.vertices.shape[0], m.faces.shape[0]
    work = mesh._mesh_work(V, F, sig.device)
    _, C, need = mesh._label("mesh_clean_step", m.faces, V, work, rounds=1, batches=1024)
    _, _, batches = mesh._label("mesh_clean_step", m.faces, V, work)
    out = {}

    def kernels():
        out["comp"] = mesh.components(m)
        out["mesh"] = mesh.filter_components(m, keep_largest=1)

    def composed():
        out["torch"] = torch_clean(m, mesh.LABEL_ROUNDS, mesh.LABEL_BATCHES)

    t = interleaved_ms({"kernels": kernels, "torch": composed,
                        "components": lambda: mesh.components(m),
                        "filter": lambda: mesh.filter_components(m, keep_largest=1)}, 3, rounds)
    tv, tf, tn = out["torch"]
    return {"what": "components+filter", "mesh": name, "V": V, "F": F, "components": C,
            "kept_V": int(out["mesh"].vertices.shape[0]), "rounds_needed": need,
            "rounds_per_batch": mesh.LABEL_ROUNDS, "batches": batches,
            "syncs": {"components": batches, "filter_components": batches + 1},
            "equal_torch": bool(torch.equal(out["mesh"].vertices, tv)
                                and torch.equal(out["mesh"].faces, tf)
                                and torch.equal(out["mesh"].normals, tn)),
            "kernels_ms": t["kernels"]["ms"], "kernels_range_ms": t["kernels"]["range_ms"],
            "torch_ms": t["torch"]["ms"], "torch_range_ms": t["torch"]["range_ms"],
            "components_ms": t["components"]["ms"], "filter_ms": t["filter"]["ms"],
            "work_bytes": int(work.numel())}


def clean_records(n, rounds, dev):
    yield run_clean(f"sphere{n}", sphere_lattice(n, dev), float(20.0 * np.exp(-3.0)),
                    ((-1.0,) * 3, (1.0,) * 3), rounds)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    noise = torch.rand(161, 161, 161, device=dev, generator=gen)
    yield run_clean("noise160", noise, 0.8, ((-1.0,) * 3, (1.0,) * 3), rounds)


# ---- (b) the masked lattice -------------------------------------------------------------
def _expand(v):
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    return (v | (v << 2)) & 0x09249249


def ball_bitfield(cascades, scale, radius, dev):
    """one sub-NeRF's bitfield with the cells whose centre lies within
    `radius` (world units) of the origin set, on every cascade"""
    n = torch.arange(G, device=dev)
    z, y, x = torch.meshgrid(n, n, n, indexing="ij")
    idx = (_expand(x) | (_expand(y) << 1) | (_expand(z) << 2)).reshape(-1)
    out = []
    for mip in range(cascades):
        mb = min(2.0 ** (mip - 1), scale)
        c = ((n.float() + 0.5) / G * 2 - 1) * mb
        cz, cy, cx = torch.meshgrid(c, c, c, indexing="ij")
        flat = torch.zeros(G ** 3, dtype=torch.bool, device=dev)
        flat[idx] = ((cx * cx + cy * cy + cz * cz) <= radius * radius).reshape(-1)
        w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device=dev)
        out.append((flat.view(-1, 8) * w).sum(1).to(torch.uint8))
    return torch.cat(out)


def run_mask(shape, n, rounds):
    from radnerf_amd import mesh
    from radnerf_amd import synthetic as S
    K, scale = SHAPES[shape]
    dev = torch.device("cuda")
    m = S.parity_scene(K, scale=scale, device=dev).m
    fields = {f"ball{int(100 * r)}": ball_bitfield(m.cascades, scale, r * scale, dev)
              for r in (0.25, 0.5, 0.75)}
    fields["ones"] = torch.full_like(fields["ball25"], 255)
    holder = {}

    def masked(bits):
        def fn():
            for k in range(K):
                setattr(m, f"density_bitfield_{k}", bits)
            holder["s"] = mesh.density_lattice(m, n, occupancy=True)
        return fn

    forms = {"unmasked": lambda: holder.__setitem__("u", mesh.density_lattice(m, n))}
    forms.update({k: masked(b) for k, b in fields.items()})
    t = interleaved_ms(forms, 2, rounds)
    pts = (n + 1) ** 3
    rec = {"what": "masked lattice", "shape": shape, "K": K, "scale": scale, "resolution": n,
           "points": pts, "unmasked_ms": t["unmasked"]["ms"],
           "unmasked_range_ms": t["unmasked"]["range_ms"]}
    for k, b in fields.items():
        masked(b)()
        rec[k] = {"ms": t[k]["ms"], "range_ms": t[k]["range_ms"],
                  "vs_unmasked": round(t[k]["ms"] / t["unmasked"]["ms"], 4),
                  "live_point_share": round(float((holder["s"] != 0).float().mean()), 4)}
        if k == "ones":
            rec[k]["equal_unmasked"] = bool(torch.equal(holder["s"], holder["u"]))
        else:
            r = int(k[4:]) / 100
            rec[k]["ball_share_of_box"] = round(4 / 3 * math.pi * r ** 3 / 8, 4)
    return rec


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--ab" in args:
        ab_main(args, os.path.join(ROOT, "profiles", "mesh_clean", "ab_default.txt"))
        sys.exit(0)
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    dest = opt("--out", os.path.join(ROOT, "profiles", "mesh_clean", "mesh_clean_step.jsonl"))
    n, rounds, only = int(opt("--res", "512")), int(opt("--rounds", "4")), opt("--only", "ab")
    with torch.no_grad():
        if "a" in only:
            for rec in clean_records(n, rounds, torch.device("cuda")):
                append_jsonl(dest, rec)
                torch.cuda.empty_cache()
        if "b" in only:
            for shape in opt("--shapes", "c3,k8s16").split(","):
                append_jsonl(dest, run_mask(shape, n, rounds))
                torch.cuda.empty_cache()
