"""Cost of saving validation images (dev tool, GPU): 800 x 800 views at C3
(K = 2, scale 0.5, synthetic weights), validated with and without their
pictures, two forms interleaved round by round in one process (as
tools/validate_step.py), a device synchronise around the timed validations;
one JSON line with the median ms per image.

  plain     Trainer.validate without save_dir: render, PSNR, SSIM;
  device    Trainer.validate(save_dir=...): the same, then
            ImageEvaluator.images8 (rn_quantize_u8, rn_minmax_finite +
            rn_colormap_u8, rn_gate_map_u8), three uint8 copies into pinned
            buffers, and imageout.ImageSaver's deferred write_png;
  composed  the same validation with the pictures made by hand: three
            .cpu().numpy() copies of the fp32 buffers (rgb, depth, gating
            code), numpy quantise, numpy depth2img with the same table, a
            numpy gate blend, and the same write_png, image after image.

The split of the two saving forms (the map kernels between events, the copies,
zlib and the file write timed on their own) is in the same line.

  --validate-only   time `plain` alone: with --tree DIR on the package of
                    another tree (an A/B against an older checkout, no
                    older than synthetic.set_bitfields)

usage: python tools/imageout_step.py [--out FILE] [--res N] [--images N]
                                     [--validate-only] [--tree DIR]
"""
import os
import shutil
import sys
import tempfile
import time
import zlib

_argv = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(_argv[_argv.index("--tree") + 1]) if "--tree" in _argv else ROOT
sys.path[:0] = [TREE, os.path.join(TREE, "rad-nerf_amd"), os.path.join(TREE, "tools"),
                os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radnerf_amd import layout as LY  # noqa: E402
from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.synthetic import ring_cameras  # noqa: E402
from radnerf_amd.trainer import Trainer  # noqa: E402
from steptime import append_jsonl, interleaved_ms  # noqa: E402


def setup(res, n_img):
    K, scale = 2, 0.5
    dev = torch.device("cuda")
    m = MNGP(scale, size=K, seed=3)
    g = Ray_Gate(K, seed=4)
    S.set_bitfields(m, S.bitfields(K, m.cascades, p=0.5, seed=1))
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(K, LY.FIELD_PARAMS)))
    m, g = m.to(dev), g.to(dev)
    dirs, poses = (t.to(dev) for t in ring_cameras(n_img, res))
    gt = torch.rand(n_img, dirs.shape[0], 3, generator=torch.Generator().manual_seed(0)).to(dev)
    tr = Trainer(m, g, 8192, directions=dirs, poses=poses.contiguous(), img_wh=(res, res))
    return tr, poses.contiguous(), gt


def timed(forms, n_img, rounds=6):
    """median ms per image of each form, the forms alternating per round"""
    out = {}
    for k, t in interleaved_ms(forms, 1, rounds, warm=False).items():
        out[k + "_ms"] = round(t["ms"] / n_img, 4)
        out[k + "_spread_ms"] = [round(x / n_img, 4) for x in t["range_ms"]]
    return out


def numpy_maps(rgb, depth, gate, lut, pal):
    """the pictures from the fp32 host arrays, as a user would write them"""
    rgb8 = np.clip(rgb * 255, 0, 255).astype(np.uint8)
    fin = depth[np.isfinite(depth)]
    mn, mx = (fin.min(), fin.max()) if fin.size else (0.0, 0.0)
    t = (depth - mn) / (mx - mn) if mx > mn else np.zeros_like(depth)
    d8 = lut[np.clip(np.nan_to_num(t) * 255, 0, 255).astype(np.uint8)]
    g8 = np.clip(gate @ pal.astype(np.float32) + 0.5, 0, 255).astype(np.uint8)
    return rgb8, d8, g8


def host_ms(fn, reps=5):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4)


def run(res=800, n_img=4, validate_only=False):
    tr, poses, gt = setup(res, n_img)
    out = {"shape": "c3", "K": 2, "scale": 0.5, "img_wh": [res, res], "images": n_img,
           "tree": os.path.relpath(TREE, ROOT)}
    plain = lambda: tr.validate(poses, gt)
    if validate_only:
        out.update(timed({"plain": plain}, n_img))
        return out
    from radnerf_amd import imageout
    from radnerf_amd.metrics import ImageMetrics
    lut, pal = imageout.TURBO_LUT, imageout.default_palette(2)
    W = H = res
    tmp = tempfile.mkdtemp(prefix="imageout_step_")
    try:
        d_dev, d_cmp = os.path.join(tmp, "device"), os.path.join(tmp, "composed")
        os.makedirs(d_cmp)
        plain()
        ev = tr._evaluator

        def device():
            tr.validate(poses, gt, save_dir=d_dev, epoch=0)

        def composed():
            acc = ImageMetrics()
            for i in range(n_img):
                res_i = ev.render_image(poses[i])
                acc.update(res_i["rgb"], gt[i], (W, H))
                rgb, depth, gate = (res_i[k].cpu().numpy() for k in ("rgb", "depth", "gating_code"))
                for tail, im in zip(("", "_d", "_g"), numpy_maps(rgb, depth, gate, lut, pal)):
                    imageout.write_png(os.path.join(d_cmp, f"{i:03d}epoch0{tail}.png"),
                                       im.reshape(H, W, 3))
            acc.compute()

        out.update(timed({"plain": plain, "device": device, "composed": composed}, n_img))
        out["device_saving_ms"] = round(out["device_ms"] - out["plain_ms"], 4)
        out["composed_saving_ms"] = round(out["composed_ms"] - out["plain_ms"], 4)
        # the files of the two forms (rgb and depth byte for byte; the numpy blend
        # is a matrix product, not the kernel's sequential one)
        same, size = {}, {}
        for kind, tail in (("rgb", ""), ("depth", "_d"), ("gate", "_g")):
            a, b = (open(os.path.join(d, f"000epoch0{tail}.png"), "rb").read()
                    for d in (d_dev, d_cmp))
            same[kind], size[kind] = a == b, len(a)
        out["files_equal"], out["file_bytes"] = same, size
        # ---- the split, one image ----------------------------------------------------
        res0 = ev.render_image(poses[0])

        def events(fn, inner=20, reps=15):
            for _ in range(3):
                fn()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / inner)
            return round(float(np.median(ts)), 2)

        f32 = {k: res0[k] for k in ("rgb", "depth", "gating_code")}
        o8 = {k: torch.empty(H, W, 3, dtype=torch.uint8, device=gt.device)
              for k in ("rgb", "depth", "gate")}
        split = {"kernels_us": {
            "images8": events(ev.images8),
            "quantize_u8": events(lambda: imageout.to_uint8(f32["rgb"], out=o8["rgb"])),
            "minmax_colormap": events(lambda: imageout.depth2img(f32["depth"], out=o8["depth"])),
            "gate_map": events(lambda: imageout.gate2img(f32["gating_code"], out=o8["gate"]))}}
        im8 = ev.images8()
        pinned = {k: torch.empty(v.shape, dtype=torch.uint8, pin_memory=True)
                  for k, v in im8.items()}

        def copy8():
            for k, v in im8.items():
                pinned[k].copy_(v, non_blocking=True)

        split["copy_u8_pinned_us"] = events(copy8, inner=5)
        split["copy_u8_bytes"] = sum(v.numel() for v in im8.values())

        def copy32():
            torch.cuda.synchronize()
            return [v.cpu().numpy() for v in f32.values()]

        split["copy_f32_pageable_ms"] = host_ms(copy32)
        split["copy_f32_bytes"] = sum(4 * v.numel() for v in f32.values())
        host = copy32()
        split["numpy_maps_ms"] = host_ms(lambda: numpy_maps(*host, lut, pal))
        arrs = [v.cpu().numpy() for v in im8.values()]

        def rows(a):
            r = np.empty((H, 1 + 3 * W), dtype=np.uint8)
            r[:, 0] = 0
            r[:, 1:] = a.reshape(H, -1)
            return r.tobytes()

        raw = [rows(a) for a in arrs]
        split["zlib_ms"] = host_ms(lambda: [zlib.compress(r, 6) for r in raw])
        split["write_png_ms"] = host_ms(lambda: [
            imageout.write_png(os.path.join(tmp, f"s{j}.png"), a) for j, a in enumerate(arrs)])
        out["split_per_image"] = split
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


if __name__ == "__main__":
    opt = lambda name, default: type(default)(_argv[_argv.index(name) + 1]) \
        if name in _argv else default
    path = opt("--out", os.path.join(ROOT, "profiles", "imageout", "imageout_step.jsonl"))
    append_jsonl(path, run(res=opt("--res", 800), n_img=opt("--images", 4),
                           validate_only="--validate-only" in _argv))
