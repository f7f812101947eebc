"""Few-view training with and without depth supervision (dev tool / evidence,
GPU; DESIGN.md §4 "Depth supervision").  Appends JSON lines to
profiles/depth/depth_demo.jsonl.

The scene is tools/train_demo.py's: a sphere of radius 0.25 coloured 0.5 +
0.5 n in front of a white background, K = 2 sub-NeRFs, scale 0.5.  The
training set is `views` images (4 and 8) of side x side pixels from eyes on
the radius-1.5 sphere (tools/tsdf_demo.sphere_cameras: a pinhole whose
directions have z = 1 and are not normalised, so the analytic z-depth of a
hit is the ray parameter, TrainDepths(kind="t", scale 1); a miss has no
measurement).  Trainer.step_sampled draws the batches.  Three configurations
from the same initialisation and batch stream:

    none        no depth term
    mean        lambda_depth      (the expected-depth term)
    var         lambda_depth_var  (the ray-termination term, in the composite)

and per configuration: PSNR and rendered-depth RMSE (over the rays that hit)
on held-out rays (train_demo.batch: fresh random rays with exact targets),
and the TSDF export's mean radius and component count (tsdf.fuse_mesh from 24
cameras, mesh_demo.describe; nothing filtered).

    python tools/depth_demo.py [steps] [rays] [side] [--views 4,8] [--out FILE]
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from mesh_demo import describe  # noqa: E402
from steptime import append_jsonl  # noqa: E402
from train_demo import R_SPHERE, batch  # noqa: E402
from tsdf_demo import sphere_cameras  # noqa: E402

CONFIGS = {"none": {}, "mean": dict(lambda_depth=0.1), "var": dict(lambda_depth_var=0.1)}


def sphere_views(dirs, poses):
    """uint8 images (N, P, 3) and fp32 depth maps (N, P) of the analytic
    sphere: the ray parameter of the first hit (the directions are not
    normalised), 0 where the ray misses"""
    d = torch.einsum("pj,nij->npi", dirs, poses[:, :, :3])
    o = poses[:, None, :, 3].expand_as(d)
    a, b = (d * d).sum(-1), (o * d).sum(-1)
    disc = b * b - a * ((o * o).sum(-1) - R_SPHERE ** 2)
    t = (-b - torch.sqrt(disc.clamp_min(0))) / a
    hit = (disc > 0) & (t > 0)
    nrm = o + t[..., None] * d
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    img = torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.ones_like(nrm))
    return ((img * 255).round().to(torch.uint8).contiguous(),
            torch.where(hit, t, torch.zeros_like(t)).contiguous())


def held_out(tr, held):
    """PSNR over all held-out rays, depth RMSE over those that hit the sphere"""
    dev = tr.device
    K, B = tr.model.size, tr.n_rays
    noise, bg = torch.zeros(K, B, device=dev), torch.ones(3, device=dev)
    mse = n = se = nd = 0.0
    with torch.no_grad():
        for o, d, target in held:
            rgb, _, depth, gate, _ = tr.renderer.forward(o, d, d, noise, bg, 1e-4, tr.esf)
            mse += float(((rgb - target) ** 2).sum())
            n += target.numel()
            b = (o * d).sum(1)
            disc = b * b - ((o * o).sum(1) - R_SPHERE ** 2)
            t = -b - torch.sqrt(disc.clamp_min(0))
            hit = (disc > 0) & (t > 0)
            e = ((gate * depth).sum(1) - t)[hit]
            se += float((e * e).sum())
            nd += int(hit.sum())
    return (round(-10 * math.log10(max(mse / n, 1e-12)), 3),
            round(math.sqrt(se / max(nd, 1)), 5))


def run(views, steps, B, side, res=128, n_cam=24):
    from radnerf_amd import tsdf
    from radnerf_amd.networks import MNGP, Ray_Gate
    from radnerf_amd.sampler import TrainDepths
    from radnerf_amd.trainer import Trainer
    dev = torch.device("cuda")
    dirs, poses, _ = sphere_cameras(views, side)
    images, depths = sphere_views(dirs, poses)
    dirs, poses, images, depths = (x.to(dev).contiguous() for x in (dirs, poses, images, depths))
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    held = [batch(gen, B, dev, 1.0) for _ in range(4)]
    cdirs, cposes, Kmat = sphere_cameras(n_cam, 200)
    cdirs, cposes = cdirs.to(dev), cposes.to(dev)
    rec = {"scene": f"sphere r={R_SPHERE}, white background, K=2, scale 0.5", "views": views,
           "image": [side, side], "steps": steps, "rays": B, "held_out_rays": 4 * B,
           "hit_share_of_pixels": round(float((depths > 0).float().mean()), 4),
           "tsdf": {"resolution": res, "cameras": n_cam}, "configs": {}}
    for name, lam in CONFIGS.items():
        torch.manual_seed(0)
        m, g = MNGP(0.5, size=2, seed=3).to(dev), Ray_Gate(2, seed=4).to(dev)
        tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, seed=1, images=images,
                     directions=dirs, poses=poses, img_wh=(side, side),
                     depths=TrainDepths(depths), **lam)
        t0 = time.time()
        terms = {}
        for _ in range(steps):
            terms = tr.step_sampled()
        torch.cuda.synchronize()
        psnr, rmse = held_out(tr, held)
        fused = tsdf.fuse_mesh(m, g, cposes, cdirs, (200, 200), Kmat, resolution=res,
                               exp_step_factor=tr.esf)
        d = describe(fused)
        out = {"lambdas": lam, "train_seconds": round(time.time() - t0, 2),
               "last_terms": {k: round(float(v), 6) for k, v in terms.items()},
               "held_out_psnr": psnr, "held_out_depth_rmse": rmse,
               "tsdf_components": d.get("components"), "tsdf_radius_mean_all": d.get("radius_mean_all"),
               "tsdf_largest_radius_mean": (d.get("largest") or {}).get("radius_mean"),
               "tsdf_vertices": d["V"]}
        rec["configs"][name] = out
        print(name, out, flush=True)
        del tr, m, g
        torch.cuda.empty_cache()
    return rec


def main():
    args = sys.argv[1:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    pos = [a for i, a in enumerate(args) if not a.startswith("--")
           and (i == 0 or not args[i - 1].startswith("--"))]
    num = lambda i, d: int(pos[i]) if len(pos) > i else d
    steps, B, side = num(0, 1000), num(1, 8192), num(2, 100)
    dest = opt("--out", os.path.join(ROOT, "profiles", "depth", "depth_demo.jsonl"))
    for views in (int(v) for v in opt("--views", "4,8").split(",")):
        append_jsonl(dest, run(views, steps, B, side))


if __name__ == "__main__":
    main()
