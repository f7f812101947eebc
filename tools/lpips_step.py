"""Cost of LPIPS (dev tool, GPU): one 800 x 800 image pair through
radnerf_amd.lpips.LPIPS (synthetic weights of the real shapes) against the
same network composed from torch's conv2d / max_pool2d on the device, the forms
interleaved round by round in one process (tools/steptime.py interleaved_ms),
every form warm; then one C3 validation image (K = 2, scale 0.5, as
tools/validate_step.py) with and without lpips.  One JSON line.

  hip            LPIPS.__call__: rn_lpips_prepare x 2, 13 rn_conv3x3_relu_f16,
                 4 rn_maxpool2_f16, 5 rn_lpips_layer; both images per launch;
  torch_f16_cl   the same operation in torch ops, f16 channels_last (MIOpen
                 picks its algorithms on the untimed first call);
  torch_fp32     the same in fp32, contiguous.

The per-convolution times of the HIP stack (events around 10 launches each)
and the arithmetic rate they amount to are in the same line, as are the three
scores (they differ by the f16 storage and the summation order only).

usage: python tools/lpips_step.py [--out FILE] [--res N] [--images N] [--no-validate]
"""
import os
import sys

_argv = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from radnerf_amd import lpips as LP  # noqa: E402
from radnerf_amd._lib import lib  # noqa: E402
from steptime import append_jsonl, interleaved_ms  # noqa: E402


def torch_chain(weights, dev, dtype, channels_last):
    """the operation of lpips.py in torch ops on the device -> callable(pred,
    target, img_wh) -> fp64 scalar"""
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    conv = [(w.to(dev, dtype).contiguous(memory_format=fmt), b.to(dev, dtype))
            for w, b in weights["conv"]]
    lin = [v.to(dev, torch.float32).view(1, -1, 1, 1) for v in weights["lin"]]
    shift = torch.tensor(LP.SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(LP.SCALE, device=dev).view(1, 3, 1, 1)

    @torch.no_grad()
    def run(pred, target, img_wh):
        W, H = img_wh
        x = torch.stack([pred, target]).view(2, H, W, 3).permute(0, 3, 1, 2)
        x = (((2 * x - 1).clamp(-1, 1) - shift) / scale).to(dtype).contiguous(memory_format=fmt)
        total, i, tap = 0, 0, 0
        for item in LP.VGG16:
            if item == "P":
                x = F.max_pool2d(x, 2)
                continue
            x = F.relu(F.conv2d(x, conv[i][0], conv[i][1], padding=1))
            if i == LP.TAPS[tap]:
                f = x.float()
                n = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                d = (lin[tap] * (n[0:1] - n[1:2]).pow(2)).sum(1)
                total = total + d.double().mean()
                tap += 1
            i += 1
        return total
    return run


def conv_layers_ms(lp, inner=10):
    """ms per launch of each of the 13 convolutions at the LPIPS object's size
    (two images), on whatever the buffers hold"""
    L, dev = lib(), lp.device
    st = torch.cuda.current_stream(dev).cuda_stream
    W, H = lp.img_wh
    out, h, w, i = [], H, W, 0
    for item in LP.VGG16:
        if item == "P":
            h, w = h // 2, w // 2
            continue
        cin, cout = item
        src = lp.x.data_ptr() if cin == 3 else lp.buf[0].data_ptr()
        call = lambda: L.conv3x3_relu_f16(src, lp.frags[i].data_ptr(), lp.bias[i].data_ptr(), 2,
                                          h, w, cin, cout, lp.buf[1].data_ptr(), st)
        for _ in range(2):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            call()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / inner
        flop = 2.0 * 2 * h * w * cout * 9 * cin
        out.append({"cin": cin, "cout": cout, "h": h, "w": w, "ms": round(ms, 4),
                    "tflops": round(flop / ms * 1e-9, 2)})
        i += 1
    return out


def validation_setup(res, n_img):
    from radnerf_amd import layout as LY
    from radnerf_amd import synthetic as S
    from radnerf_amd.networks import MNGP, Ray_Gate
    from radnerf_amd.synthetic import ring_cameras
    from radnerf_amd.trainer import Trainer
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


def run(res=800, n_img=2, validate=True, rounds=5, steps=40):
    dev = torch.device("cuda", torch.cuda.current_device())
    wts = LP.synthetic_weights(0)
    lp = LP.LPIPS(wts, (res, res), device=dev)
    g = torch.Generator().manual_seed(1)
    target = torch.rand(res * res, 3, generator=g)
    pred = (target + 0.1 * torch.randn(res * res, 3, generator=g)).clamp(0, 1).contiguous()
    pred, target = pred.to(dev), target.to(dev)
    out = {"img_wh": [res, res], "device": torch.cuda.get_device_name(dev),
           "flop_per_pair": 2 * sum(2.0 * 9 * c["cin"] * c["cout"] * c["h"] * c["w"]
                                    for c in conv_layers_ms(lp, inner=1))}
    forms = {"hip": lambda: lp(pred, target)}
    scores = {"hip": float(lp(pred, target))}
    for name, dtype, cl in (("torch_f16_cl", torch.float16, True),
                            ("torch_fp32", torch.float32, False)):
        try:
            chain = torch_chain(wts, dev, dtype, cl)
            scores[name] = float(chain(pred, target, (res, res)))       # the untimed first call
            forms[name] = lambda chain=chain: chain(pred, target, (res, res))
        except RuntimeError as e:                   # a yardstick torch cannot run here
            out[name + "_error"] = str(e)[:200]
    out["scores"] = scores
    for k, t in interleaved_ms(forms, steps, rounds).items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    for k in ("torch_f16_cl", "torch_fp32"):
        if k + "_ms" in out:
            out[f"hip_over_{k}"] = round(out["hip_ms"] / out[k + "_ms"], 3)
    out["hip_tflops"] = round(out["flop_per_pair"] / out["hip_ms"] * 1e-9, 2)
    out["conv_layers"] = conv_layers_ms(lp)
    if validate:
        tr, poses, gt = validation_setup(res, n_img)
        val = interleaved_ms({"plain": lambda: tr.validate(poses, gt),
                              "with_lpips": lambda: tr.validate(poses, gt, lpips=lp)},
                             1, rounds, warm=False)
        out["validate"] = {"shape": "c3", "images": n_img,
                           **{k + "_ms_per_image": round(t["ms"] / n_img, 4)
                              for k, t in val.items()},
                           **{k + "_spread_ms": [round(x / n_img, 4) for x in t["range_ms"]]
                              for k, t in val.items()}}
    return out


if __name__ == "__main__":
    opt = lambda name, default: type(default)(_argv[_argv.index(name) + 1]) \
        if name in _argv else default
    path = opt("--out", os.path.join(ROOT, "profiles", "lpips", "lpips_step.jsonl"))
    append_jsonl(path, run(res=opt("--res", 800), n_img=opt("--images", 2),
                           validate="--no-validate" not in _argv))
