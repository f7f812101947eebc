"""Mesh export of a trained model (dev tool / evidence, GPU).

Trains tools/train_demo.py's scene -- a sphere of radius 0.25 at the origin in
front of a white background, K = 2 sub-NeRFs, fresh rays every step -- then
exports the geometry at 128^3 with the default level (the training density
threshold) and reports, for the mean of the sub-NeRFs and for each sub-NeRF
alone (one-hot weights): V, F, the Euler characteristic, the number of
connected components, and for the largest component its share of the vertices
and its radius error max|r - 0.25|, and over all used vertices the mean radius
and the worst vertex.  The first export filters nothing: whatever floats
beside the sphere is in the counts.  Then the same model is exported with the
occupancy mask alone (occupancy=True) and with the mask and the component
filter (occupancy=True, keep_largest=1), whose one derivable bar is exactly
one component (counted on the device by mesh.components).

    python tools/mesh_demo.py [steps] [rays] [resolution] [--out FILE] [--ply FILE]
"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from steptime import append_jsonl  # noqa: E402
from train_demo import R_SPHERE, batch  # noqa: E402


def components(n_vertices, faces):
    """labels of the vertices' connected components (minimum-label
    propagation with pointer jumping)"""
    lab = np.arange(n_vertices)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    while True:
        m = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        new = lab.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        new = new[new]
        if (new == lab).all():
            return lab
        lab = new


def describe(mesh):
    v = mesh.vertices.cpu().numpy().astype(np.float64)
    f = mesh.faces.cpu().numpy().astype(np.int64)
    out = {"V": len(v), "F": len(f)}
    if len(f) == 0:
        return out
    und = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    used = np.unique(f)
    lab = components(len(v), f)[used]
    ids, counts = np.unique(lab, return_counts=True)
    big = used[lab == ids[np.argmax(counts)]]
    r = np.linalg.norm(v[big], axis=1)
    ra = np.linalg.norm(v[used], axis=1)
    out.update({"radius_mean_all": round(float(ra.mean()), 5),
                "worst_vertex_err": round(float(np.abs(ra - R_SPHERE).max()), 5)})
    # per-component Euler characteristic of the largest one
    fb = f[np.isin(f[:, 0], big)]
    eb = np.unique(np.sort(np.concatenate([fb[:, [0, 1]], fb[:, [1, 2]], fb[:, [2, 0]]]), 1), axis=0)
    out.update({"euler": int(len(used) - len(und) + len(f)), "components": int(len(ids)),
                "component_sizes": sorted((int(c) for c in counts), reverse=True)[:8],
                "largest": {"vertex_share": round(float(len(big) / len(used)), 4),
                            "euler": int(len(big) - len(eb) + len(fb)),
                            "radius_mean": round(float(r.mean()), 5),
                            "radius_err_max": round(float(np.abs(r - R_SPHERE).max()), 5),
                            "normal_dot_radial_min": None}})
    if mesh.normals is not None:
        n = mesh.normals.cpu().numpy().astype(np.float64)[big]
        out["largest"]["normal_dot_radial_min"] = round(
            float(((n * v[big]).sum(1) / np.maximum(r, 1e-12)).min()), 4)
    return out


def main():
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    pos = [a for i, a in enumerate(args) if not a.startswith("--")
           and (i == 0 or not args[i - 1].startswith("--"))]
    steps = int(pos[0]) if len(pos) > 0 else 1000
    B = int(pos[1]) if len(pos) > 1 else 8192
    res = int(pos[2]) if len(pos) > 2 else 128
    from radnerf_amd import mesh
    from radnerf_amd.networks import MNGP, Ray_Gate
    from radnerf_amd.trainer import Trainer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    K = 2
    m, g = MNGP(0.5, size=K, seed=3).to(dev), Ray_Gate(K, seed=4).to(dev)
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    t0 = time.time()
    tail = []
    for s in range(steps):
        o, d, target = batch(gen, B, dev, 1.0)
        terms = tr.step(o, d, d, target)
        if s >= steps - 100:
            tail.append(float(terms["rgb"]))
    torch.cuda.synchronize()
    rec = {"scene": f"sphere r={R_SPHERE}, white background, K={K}, scale 0.5",
           "steps": steps, "rays": B, "train_seconds": round(time.time() - t0, 2),
           "psnr_last100": round(float(-10 * np.log10(max(np.mean(tail), 1e-12))), 2),
           "resolution": res, "iso": round(mesh.DEFAULT_ISO, 4),
           "cell_edge": round(1.0 / res, 6)}
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        ply = opt("--ply", os.path.join(tmp, "mesh_demo.ply"))
        mean = tr.export_mesh(ply, resolution=res, colors=True)
        torch.cuda.synchronize()
        rec["export_seconds"] = round(time.time() - t0, 3)
        rec["ply_bytes"] = os.path.getsize(ply)
    rec["mean"] = describe(mean)
    for k in range(K):
        w = [1.0 if q == k else 0.0 for q in range(K)]
        rec[f"sub_nerf_{k}"] = describe(mesh.extract_mesh(m, resolution=res, weights=w))
    rec["masked"] = describe(mesh.extract_mesh(m, resolution=res, occupancy=True))
    clean = mesh.extract_mesh(m, resolution=res, occupancy=True, keep_largest=1)
    rec["masked_largest"] = describe(clean)
    rec["masked_largest"]["device_components"] = int(mesh.components(clean).n_vertices.shape[0])
    rec["unmasked_largest"] = describe(mesh.extract_mesh(m, resolution=res, keep_largest=1))
    append_jsonl(opt("--out", os.path.join(ROOT, "profiles", "mesh_clean", "mesh_demo.jsonl")), rec)


if __name__ == "__main__":
    main()
