"""Cost of validating one image (dev tool, GPU): an 800 x 800 view at C3
(K = 2, scale 0.5, synthetic weights) rendered and scored with PSNR and SSIM,
two forms interleaved round by round in one process (as tools/pose_step.py), a
device synchronise around the timed images; one JSON line with the median ms
per image.

  evaluator  ImageEvaluator.evaluate: per chunk rn_get_rays, the gate, the box
             interval, rn_render_test and rn_ml_combine_test into the image
             buffers, then rn_image_sse and rn_ssim;
  composed   the same chunks through the public per-ray API: rays.get_rays and
             the gate's mean direction in torch, ml_render(test_time=True), the
             chunk's rgb copied into the image, then PSNR (torch mse) and a
             torch conv2d SSIM (the same Gaussian window, valid windows, fp32).

Both forms run the same render kernel on the same rays; the JSON also holds
how far their numbers are apart.

usage: python tools/validate_step.py [--out FILE] [--res N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from radnerf_amd import layout as LY  # noqa: E402
from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd.evaluate import DEFAULT_CHUNK, ImageEvaluator  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.rays import get_rays  # noqa: E402
from radnerf_amd.rendering import ml_render  # noqa: E402
from radnerf_amd.synthetic import ring_cameras  # noqa: E402
from steptime import append_jsonl, interleaved_ms  # noqa: E402


def torch_ssim(pred, target, H, W):
    """StructuralSimilarityIndexMeasure(data_range=1) over the valid windows,
    composed from torch ops in fp32: five grouped conv2d with the 11 x 11
    Gaussian (sigma 1.5) on (1, 3, H, W) views."""
    C = pred.shape[1]
    d = torch.arange(11, device=pred.device, dtype=torch.float32) - 5
    g = torch.exp(-(d / 1.5) ** 2 / 2)
    g = g / g.sum()
    k = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1)
    p = pred.view(H, W, C).permute(2, 0, 1)[None]
    t = target.view(H, W, C).permute(2, 0, 1)[None]
    E = lambda x: F.conv2d(x, k, groups=C)
    mp, mt = E(p), E(t)
    spp, stt, spt = E(p * p) - mp * mp, E(t * t) - mt * mt, E(p * t) - mp * mt
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    v = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    return v.mean()


def run(res=800, steps=5, rounds=6, chunk=DEFAULT_CHUNK):
    K, scale = 2, 0.5
    dev = torch.device("cuda")
    m = MNGP(scale, size=K, seed=3)
    g = Ray_Gate(K, seed=4)
    S.set_bitfields(m, S.bitfields(K, m.cascades, p=0.5, seed=1))
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(K, LY.FIELD_PARAMS)))
    m, g = m.to(dev), g.to(dev)
    dirs, poses = (t.to(dev) for t in ring_cameras(4, res))
    pose = poses[1].contiguous()
    N = dirs.shape[0]
    gt = torch.rand(N, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    ev = ImageEvaluator(m, g, dirs, (res, res), chunk=chunk)
    image = torch.empty(N, 3, device=dev)
    last = {}

    def evaluator():
        last["evaluator"] = ev.evaluate(pose, gt)

    def composed():
        with torch.no_grad():
            for r0 in range(0, N, ev.chunk):
                o, d = get_rays(dirs[r0:r0 + ev.chunk], pose)
                res_c = ml_render(m, g, o, d, d, test_time=True, exp_step_factor=ev.esf)
                image[r0:r0 + ev.chunk] = res_c["rgb"]
            mse = ((image - gt) ** 2).mean()
            last["composed"] = {"psnr": -10.0 * torch.log10(mse),
                                "ssim": torch_ssim(image, gt, res, res)}

    forms = {"evaluator": evaluator, "composed": composed}
    times = interleaved_ms(forms, steps, rounds)
    out = {"shape": "c3", "K": K, "scale": scale, "img_wh": [res, res], "chunk": ev.chunk,
           "chunks": -(-N // ev.chunk), "steps": steps, "rounds": rounds - 1,
           "samples": int(ev.render_image(pose)["total_samples"])}
    for k, t in times.items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    out["evaluator_over_composed"] = round(out["evaluator_ms"] / out["composed_ms"], 4)
    for k in ("psnr", "ssim"):
        a, b = float(last["evaluator"][k]), float(last["composed"][k])
        out[k] = {"evaluator": round(a, 6), "composed": round(b, 6), "abs_diff": abs(a - b)}
    # the metric kernels alone: 20 back-to-back calls between two events
    from radnerf_amd import metrics
    rgb = ev.out["rgb"]
    for name, fn in (("psnr_us", lambda: metrics.psnr(rgb, gt)),
                     ("ssim_us", lambda: metrics.ssim(rgb, gt, (res, res)))):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(15):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / 20)
        out[name] = round(float(np.median(ts)), 2)
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = argv[argv.index("--out") + 1] if "--out" in argv else \
        os.path.join(ROOT, "profiles", "validate", "validate_step.jsonl")
    res = int(argv[argv.index("--res") + 1]) if "--res" in argv else 800
    append_jsonl(path, run(res=res))
