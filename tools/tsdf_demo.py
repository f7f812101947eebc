"""TSDF export against the density export on a trained model (dev tool /
evidence, GPU).

Trains tools/train_demo.py's scene as tools/mesh_demo.py does -- a sphere of
radius 0.25 in front of a white background, K = 2 sub-NeRFs, fresh rays every
step from origins on the radius-1.5 sphere -- then exports the geometry at
128^3 three ways and describes each with mesh_demo.describe (components, the
largest one's size, mean and worst radius error):

    density          mesh.extract_mesh, nothing filtered
    density_clean    mesh.extract_mesh(occupancy=True, keep_largest=1)
    tsdf             depth images rendered from N cameras on that same
                     radius-1.5 sphere (a Fibonacci lattice of eyes looking at
                     the origin: the demo trains on rays, not images, so these
                     stand in for its training cameras), fused by
                     TSDFVolume.integrate, extracted by TSDFVolume.extract;
                     nothing filtered

with the time of each TSDF stage (render, integrate, extract; a device
synchronise after each).

    python tools/tsdf_demo.py [steps] [rays] [resolution] [cameras] [image side] [--out FILE]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_demo import describe  # noqa: E402
from steptime import append_jsonl  # noqa: E402
from train_demo import R_SPHERE, batch  # noqa: E402


def sphere_cameras(n, side, radius=1.5, half=0.3):
    """n eyes on a Fibonacci lattice of the radius sphere looking at the
    origin (c2w columns right / down / front), the pinhole's directions
    (side * side, 3) with pixel centres at +0.5, and its 3x3 matrix"""
    f = side / (2 * half)
    K = np.array([[f, 0, side / 2], [0, f, side / 2], [0, 0, 1]])
    j, i = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    dirs = np.stack([(i + 0.5 - side / 2) / f, (j + 0.5 - side / 2) / f, np.ones_like(i, float)],
                    -1).reshape(-1, 3)
    poses = []
    for q in range(n):
        z = 1 - (2 * q + 1) / n
        a = q * np.pi * (3 - np.sqrt(5))
        eye = radius * np.array([np.sqrt(1 - z * z) * np.cos(a), np.sqrt(1 - z * z) * np.sin(a), z])
        front = -eye / np.linalg.norm(eye)
        right = np.cross(front, [0.13, -0.21, 0.97])
        right /= np.linalg.norm(right)
        poses.append(np.stack([right, np.cross(front, right), front, eye], 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return t(dirs), t(np.stack(poses)), K


def main():
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    pos = [a for i, a in enumerate(args) if not a.startswith("--")
           and (i == 0 or not args[i - 1].startswith("--"))]
    num = lambda i, d: int(pos[i]) if len(pos) > i else d
    steps, B, res, n_cam, side = num(0, 1000), num(1, 8192), num(2, 128), num(3, 24), num(4, 200)
    from radnerf_amd import mesh, tsdf
    from radnerf_amd.evaluate import ImageEvaluator
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
    for s in range(steps):
        o, d, target = batch(gen, B, dev, 1.0)
        tr.step(o, d, d, target)
    torch.cuda.synchronize()
    rec = {"scene": f"sphere r={R_SPHERE}, white background, K={K}, scale 0.5", "steps": steps,
           "rays": B, "train_seconds": round(time.time() - t0, 2), "resolution": res,
           "cell_edge": round(1.0 / res, 6), "cameras": n_cam, "image": [side, side]}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, round((time.perf_counter() - t) * 1e3, 2)

    dens, ms = timed(lambda: mesh.extract_mesh(m, resolution=res))
    rec["density"] = dict(describe(dens), export_ms=ms)
    clean, ms = timed(lambda: mesh.extract_mesh(m, resolution=res, occupancy=True, keep_largest=1))
    rec["density_clean"] = dict(describe(clean), export_ms=ms)

    dirs, poses, Kmat = sphere_cameras(n_cam, side)
    dirs, poses = dirs.to(dev), poses.to(dev)
    ev = ImageEvaluator(m, g, dirs, (side, side), exp_step_factor=tr.esf)
    N = side * side
    depth, opac = torch.empty(n_cam, N, device=dev), torch.empty(n_cam, N, device=dev)
    rgb = torch.empty(n_cam, N, 3, device=dev)

    def render():
        for q in range(n_cam):
            out = ev.render_image(poses[q])
            depth[q].copy_(out["depth"])
            opac[q].copy_(out["opacity"])
            rgb[q].copy_(out["rgb"])

    render()                                             # warm-up: buffers, fragments
    _, t_render = timed(render)
    vol = tsdf.TSDFVolume(res, mesh._model_box(m), device=dev)
    integrate = lambda: vol.integrate(depth, opac, poses, Kmat, dirs, (side, side), rgb=rgb)
    integrate()
    vol.reset()
    _, t_int = timed(integrate)
    vol.extract()
    fused, t_ext = timed(vol.extract)
    rec["tsdf"] = dict(describe(fused), trunc=round(vol.trunc, 6), render_ms=t_render,
                       integrate_ms=t_int, extract_ms=t_ext,
                       opaque_pixel_share=round(float((opac >= 0.5).float().mean()), 4),
                       observed_point_share=round(float((vol.w > 0).float().mean()), 4),
                       device_components=int(mesh.components(fused).n_vertices.shape[0]))
    whole = tsdf.fuse_mesh(m, g, poses, dirs, (side, side), Kmat, resolution=res,
                           exp_step_factor=tr.esf)
    rec["tsdf"]["fuse_mesh_equal"] = bool(torch.equal(whole.vertices, fused.vertices)
                                          and torch.equal(whole.faces, fused.faces)
                                          and torch.equal(whole.colors, fused.colors))
    ply = opt("--ply", None)
    if ply:
        fused.save(ply)
    append_jsonl(opt("--out", os.path.join(ROOT, "profiles", "tsdf", "tsdf_demo.jsonl")), rec)


if __name__ == "__main__":
    main()
