"""What TSDF fusion costs (dev tool / evidence, GPU), on tools/steptime.py's
harness.

An analytic sphere of radius 0.3 seen by 8 cameras of 800 x 800 pixels on a
ring of radius 1.2; per lattice (256^3 and 512^3 cells, box [-0.5, 0.5]^3,
with colours, default trunc):
  * rn_tsdf_integrate, all 8 cameras in one launch and as 8 launches of one:
    ms per launch and per camera, and the achieved bytes/s of the batched
    launch against its algorithmic traffic -- the volume read once (24 B per
    point), written once where observed (8 B, 24 B where coloured), plus the
    images (20 B per pixel and camera) and the directions;
  * the same update composed from torch ops on the device (one camera after
    the other, whole-volume tensors), with w compared exactly and phi within
    3 ulp(2) / trunc: tv and d are below 2, the composition's two divisions and
    square root may each be an ulp off, and s / trunc scales that by 1 / trunc;
  * TSDFVolume.extract against mesh.surface_nets on the same phi lattice.

    python tools/tsdf_step.py [--res 256,512] [--out FILE]
    python tools/tsdf_step.py --ab PARENT_TREE [--ab-out FILE]   (bench.py A/B)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from steptime import ab_main, alone_ms, append_jsonl  # noqa: E402

RADIUS, SIDE, N_CAM, F = 0.3, 800, 8, 900.0
BOX = ((-0.5,) * 3, (0.5,) * 3)


def scene(dev):
    """poses (8, 3, 4), K, directions, depth / opacity / rgb of the sphere"""
    K = np.array([[F, 0, 400.37], [0, F, 399.71], [0, 0, 1]])
    j, i = torch.meshgrid(torch.arange(SIDE, dtype=torch.float64),
                          torch.arange(SIDE, dtype=torch.float64), indexing="ij")
    dirs = torch.stack([(i + 0.5 - K[0, 2]) / F, (j + 0.5 - K[1, 2]) / F, torch.ones_like(i)],
                       -1).reshape(-1, 3)
    poses = []
    for q in range(N_CAM):
        a = 0.3 + 2 * np.pi * q / N_CAM
        eye = 1.2 * np.array([np.cos(a) * 0.9, np.sin(a) * 0.9, 0.436 * (-1) ** q])
        front = -eye / np.linalg.norm(eye)
        right = np.cross(front, [0.13, -0.21, 0.97])
        right /= np.linalg.norm(right)
        poses.append(np.stack([right, np.cross(front, right), front, eye], 1))
    poses = torch.from_numpy(np.stack(poses))
    depth, opac, rgb = [], [], []
    for P in poses:
        o, dw = P[:, 3], dirs @ P[:, :3].T
        a, b = (dw * dw).sum(1), dw @ o
        disc = b * b - a * (o @ o - RADIUS ** 2)
        hit = disc > 0
        t = torch.where(hit, (-b - disc.clamp_min(0).sqrt()) / a, torch.zeros_like(a))
        depth.append(t)
        opac.append(hit.double())
        rgb.append(torch.where(hit[:, None], 0.5 + 0.5 * (o + t[:, None] * dw) / RADIUS, 0.0))
    f = lambda x: x.to(dev, torch.float32).contiguous()
    return (f(poses), K, f(dirs), f(torch.stack(depth)), f(torch.stack(opac)),
            f(torch.stack(rgb)))


def torch_integrate(vol, poses, K, dirs, depth, opac, near=0.01, opacity_min=0.5):
    """rn_tsdf_integrate's update (geometry, carve) from torch ops"""
    dev = vol.phi.device
    ax = [torch.arange(vol.res[d] + 1, device=dev, dtype=torch.float32) * float(vol.step[d])
          + float(vol.lo[d]) for d in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    X = [x.reshape(-1), y.reshape(-1), z.reshape(-1)]
    phi, w = torch.zeros_like(X[0]), torch.zeros_like(X[0])
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    for c in range(poses.shape[0]):
        P = poses[c].cpu().numpy()
        d = [X[k] - float(P[k, 3]) for k in range(3)]
        cam = [(float(P[0, k]) * d[0] + float(P[1, k]) * d[1]) + float(P[2, k]) * d[2]
               for k in range(3)]
        u = torch.floor((fx * cam[0]) / cam[2] + cx)
        v = torch.floor((fy * cam[1]) / cam[2] + cy)
        ok = (cam[2] >= near) & (u >= 0) & (u < SIDE) & (v >= 0) & (v < SIDE)
        pix = torch.where(ok, v * SIDE + u, torch.zeros_like(u)).long()
        o = opac[c][pix]
        hit = ok & (o >= opacity_min)
        e = dirs[pix]
        n2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        tv = ((cam[0] * e[:, 0] + cam[1] * e[:, 1]) + cam[2] * e[:, 2]) / n2
        s = (tv - depth[c][pix] / o) * torch.sqrt(n2)
        hit &= s <= vol.trunc
        obs = torch.where(hit, torch.clamp_min(s / vol.trunc, -1.0), torch.full_like(s, -1.0))
        fold = hit | (ok & ~(o >= opacity_min))
        phi = torch.where(fold, (phi * w + obs) / (w + 1), phi)
        w = torch.where(fold, w + 1, w)
    return phi, w


def main():
    args = sys.argv[1:]
    if "--ab" in args:
        return ab_main(args, os.path.join(ROOT, "profiles", "tsdf", "ab_default.txt"))
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    out = opt("--out", os.path.join(ROOT, "profiles", "tsdf", "tsdf_step.jsonl"))
    from radnerf_amd import mesh, tsdf
    dev = torch.device("cuda")
    poses, K, dirs, depth, opac, rgb = scene(dev)
    wh, n_pix = (SIDE, SIDE), SIDE * SIDE
    for res in (int(r) for r in opt("--res", "256,512").split(",")):
        vol = tsdf.TSDFVolume(res, BOX, device=dev)
        n_pts = vol.phi.numel()
        batched = lambda: vol.integrate(depth, opac, poses, K, dirs, wh, rgb=rgb)
        singles = lambda: [vol.integrate(depth[c:c + 1], opac[c:c + 1], poses[c:c + 1], K, dirs,
                                         wh, rgb=rgb[c:c + 1]) for c in range(N_CAM)]
        geometry = lambda: vol.integrate(depth, opac, poses, K, dirs, wh)
        ms = {}
        for name, fn in (("batch8", batched), ("batch1_x8", singles), ("batch8_geometry", geometry)):
            # a fresh volume per timed call would time the memset too: the
            # update's cost does not depend on the state it folds into
            ms[name] = alone_ms(fn, 5, 2)
        vol.reset()
        batched()
        torch.cuda.synchronize()
        seen, col = int((vol.w > 0).sum()), int((vol.wc > 0).sum())
        traffic = 24 * n_pts + 8 * seen + 16 * col + N_CAM * n_pix * 20 + n_pix * 12
        tphi, tw = torch_integrate(vol, poses, K, dirs, depth, opac)
        t_torch = alone_ms(lambda: torch_integrate(vol, poses, K, dirs, depth, opac), 2, 1)
        dphi = float((tphi - vol.phi.view(-1)).abs().max())
        w_off = int((tw != vol.w.view(-1)).sum())
        bound = 3 * 2.0 ** -22 / vol.trunc
        t_valid = alone_ms(lambda: vol.extract(), 5, 2)
        t_plain = alone_ms(lambda: mesh.surface_nets(vol.phi, 0.0, BOX), 5, 2)
        m = vol.extract()
        append_jsonl(out, {
            "resolution": res, "points": n_pts, "cameras": N_CAM, "image": list(wh),
            "trunc": round(vol.trunc, 6), "observed_points": seen, "coloured_points": col,
            "integrate_ms": ms, "per_camera_ms": {k: round(v / N_CAM, 4) for k, v in ms.items()},
            "algorithmic_bytes": traffic,
            "achieved_GBps_batch8": round(traffic / ms["batch8"] / 1e6, 1),
            "torch_composition_ms": t_torch,
            "torch_vs_kernel": {"w_differs": w_off, "max_abs_dphi": dphi, "bound": bound},
            "extract_valid_ms": t_valid, "surface_nets_plain_ms": t_plain,
            "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0])})
        assert w_off == 0 and dphi <= bound, (w_off, dphi, bound)
        del vol, tphi, tw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
