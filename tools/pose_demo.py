"""Camera pose refinement on a synthetic scene (dev tool / evidence).

tools/train_demo.py's analytic scene (a sphere of radius 0.25 coloured
0.5 + 0.5 * normal before a white background) seen by N cameras on a ring of
radius 1.5.  The target colours come from the true poses; the trainer is given
perturbed ones (every camera rotated by a random axis-angle of `rot_deg`
degrees and shifted by a random vector of length `shift`).  The same
initialisation and pick stream run twice through trainer.Trainer.step_pixels:
with optimize_ext (rays.pose_rays + the fused chain's ray gradients +
rn_get_rays_pose_bw, dR / dT in the trainer's Adam at `pose_lr`) and without.

Reported per run: the rgb PSNR of the first and the last 100 steps, and the
pose error before and after -- the rotation angle between the trainer's
rotation and the true one (degrees, mean over cameras) and the distance of the
camera centres, raw and after the best rigid alignment of the camera centres
(Kabsch): scene and cameras can drift together, which no image can see.

pose_lr: the reference hard-codes 1e-8 (train_ml.py:146), at which Adam moves
a pose by at most 1e-8 per step -- 2e-5 over 2000 steps, nothing against a
perturbation of 1e-2.  The demo's default is 5e-4.

    python tools/pose_demo.py [steps] [rays] [pose_lr] [--out FILE]  -> one JSON line
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.synthetic import ring_cameras  # noqa: E402
from radnerf_amd.trainer import Trainer  # noqa: E402
from train_demo import R_SPHERE  # noqa: E402


def rodrigues(v):
    """ray_utils.py:73-100 (axisangle_to_R) in float64, (N, 3) -> (N, 3, 3)."""
    v = v.double()
    z = torch.zeros_like(v[:, 0])
    K = torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], 1),
                     torch.stack([v[:, 2], z, -v[:, 0]], 1),
                     torch.stack([-v[:, 1], v[:, 0], z], 1)], 1)
    n = (v.norm(dim=1) + 1e-7)[:, None, None]
    return torch.eye(3, dtype=v.dtype, device=v.device) + torch.sin(n) / n * K \
        + (1 - torch.cos(n)) / n ** 2 * (K @ K)


def sphere_target(o, d, bg=1.0):
    """train_demo.batch's analytic colours for rays (o, d); d need not be unit."""
    d = d / d.norm(dim=1, keepdim=True)
    b = (o * d).sum(1)
    disc = b * b - ((o * o).sum(1) - R_SPHERE ** 2)
    t = -b - torch.sqrt(disc.clamp_min(0))
    hit = (disc > 0) & (t > 0)
    nrm = o + t[:, None] * d
    nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return torch.where(hit[:, None], 0.5 + 0.5 * nrm, torch.full_like(nrm, bg)).contiguous()


def pose_error(R, T, R_true, T_true):
    """Mean rotation angle (degrees) and mean camera-centre distance, raw and
    after the rigid alignment (Kabsch on the centres) of the estimate."""
    def angle(Ra, Rb):
        tr = (Ra.transpose(1, 2) @ Rb).diagonal(dim1=1, dim2=2).sum(1)
        return torch.rad2deg(torch.acos(((tr - 1) / 2).clamp(-1, 1))).mean()
    R, T, R_true, T_true = (x.double().cpu() for x in (R, T, R_true, T_true))
    raw = (float(angle(R, R_true)), float((T - T_true).norm(dim=1).mean()))
    ca, cb = T.mean(0), T_true.mean(0)
    U, _, Vt = torch.linalg.svd((T - ca).T @ (T_true - cb))
    D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.det(Vt.T @ U.T)))],
                                dtype=torch.float64))
    Q = Vt.T @ D @ U.T                                   # estimate -> truth
    Ta = (T - ca) @ Q.T + cb
    return {"rot_deg": round(raw[0], 4), "centre": round(raw[1], 5),
            "rot_deg_aligned": round(float(angle(Q @ R, R_true)), 4),
            "centre_aligned": round(float((Ta - T_true).norm(dim=1).mean()), 5)}


def run(steps, B, pose_lr, optimize_ext, dev, n_img=24, res=64, rot_deg=1.5, shift=0.02,
        K=2, seed=1234):
    torch.manual_seed(0)
    dirs, true = ring_cameras(n_img, res)
    gen = torch.Generator().manual_seed(seed)
    ax = torch.randn(n_img, 3, generator=gen)
    e_R = ax / ax.norm(dim=1, keepdim=True) * math.radians(rot_deg)
    sh = torch.randn(n_img, 3, generator=gen)
    e_T = sh / sh.norm(dim=1, keepdim=True) * shift
    noisy = torch.cat([(rodrigues(e_R) @ true[..., :3].double()).float(),
                       (true[..., 3] + e_T)[:, :, None]], 2).contiguous()
    dirs, true, noisy = dirs.to(dev), true.to(dev), noisy.to(dev)
    m = MNGP(0.5, size=K, seed=3).to(dev)
    g = Ray_Gate(K, seed=4).to(dev)
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, directions=dirs, poses=noisy,
                 optimize_ext=optimize_ext, pose_lr=pose_lr)

    def estimate():
        if not optimize_ext:
            return noisy[..., :3], noisy[..., 3]
        return (rodrigues(tr.dR.detach()) @ noisy[..., :3].double()).float(), \
            noisy[..., 3] + tr.dT.detach()

    before = pose_error(*estimate(), true[..., :3], true[..., 3])
    dgen = torch.Generator(device=dev)
    dgen.manual_seed(seed)
    losses = []
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        img = torch.randint(n_img, (B,), generator=dgen, device=dev)
        pix = torch.randint(dirs.shape[0], (B,), generator=dgen, device=dev)
        # the photographs: what the true cameras saw at these pixels
        P = true[img]
        d_true = (dirs[pix][:, None, :] @ P[..., :3].transpose(1, 2))[:, 0]
        target = sphere_target(P[..., 3], d_true)
        losses.append(tr.step_pixels(img, pix, target)["rgb"])
    torch.cuda.synchronize()
    secs = time.time() - t0
    losses = torch.stack(losses).cpu()
    psnr = lambda x: round(-10 * math.log10(max(float(x.mean()), 1e-12)), 2)
    n = min(100, steps)
    return {"optimize_ext": optimize_ext, "seconds": round(secs, 2),
            "ms_per_step": round(secs / steps * 1e3, 3),
            "psnr_first": psnr(losses[:n]), "psnr_last": psnr(losses[-n:]),
            "pose_error_before": before,
            "pose_error_after": pose_error(*estimate(), true[..., :3], true[..., 3])}


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    steps = int(argv[0]) if len(argv) > 0 else 2000
    B = int(argv[1]) if len(argv) > 1 else 4096
    pose_lr = float(argv[2]) if len(argv) > 2 else 5e-4
    dev = torch.device("cuda")
    res = {"scene": f"sphere r={R_SPHERE} coloured 0.5+0.5n, white background; 24 ring cameras "
                    "of 64x64 pixels, every pose off by 1.5 degrees and 0.02",
           "steps": steps, "rays": B, "models": 2, "scale": 0.5, "pose_lr": pose_lr,
           "on": run(steps, B, pose_lr, True, dev), "off": run(steps, B, pose_lr, False, dev)}
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
