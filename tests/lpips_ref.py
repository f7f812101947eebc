"""fp64 torch restatement of the LPIPS-VGG distance (lpips 0.1, net vgg), the
yardstick of tests/test_gpu_lpips.py; tests/test_lpips_ref.py checks it.

    lpips_ref(pred, target, weights, img_wh, round_f16=False) -> (score, [5 terms])

pred / target (H*W, 3) in [0, 1], weights {"conv": 13 (w, b), "lin": 5 (C,)}.
Everything is double (F.conv2d in double).  round_f16 rounds the prepared
input, the weights and every post-ReLU activation to f16 -- the storage points
of the kernels (csrc/lpips.hip) -- and leaves every sum in double.
"""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# VGG16 features: output widths, "P" a 2 x 2 stride-2 max-pool; "T" a tap
CFG = (64, 64, "T", "P", 128, 128, "T", "P", 256, 256, 256, "T", "P", 512, 512, 512, "T", "P",
       512, 512, 512, "T")


def r16(t):
    """round to f16, back in double"""
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def prepare(rgb, img_wh, round_f16=False):
    """(H*W, 3) in [0, 1] -> (1, 3, H, W) double: clip(2x - 1, -1, 1), then
    (v - shift) / scale per channel"""
    W, H = img_wh
    x = rgb.detach().cpu().double().reshape(H, W, 3)
    v = (2.0 * x - 1.0).clamp(-1.0, 1.0)
    shift = torch.tensor(SHIFT, dtype=torch.float32).double()
    scale = torch.tensor(SCALE, dtype=torch.float32).double()
    y = (v - shift) / scale
    if round_f16:
        y = r16(y)
    return y.permute(2, 0, 1)[None]


def conv3x3_relu(x, w, b):
    """x (N, Cin, H, W) double; stride 1, zero padding 1, bias, ReLU"""
    return F.relu(F.conv2d(x, w.double(), b.double(), padding=1))


def pool2(x):
    """2 x 2 stride-2 max-pool, floor sizes"""
    return F.max_pool2d(x, 2)


def features(x, weights, round_f16=False):
    """the five taps (relu1_2, 2_2, 3_3, 4_3, 5_3) of x (N, 3, H, W)"""
    taps, i = [], 0
    for item in CFG:
        if item == "T":
            taps.append(x)
        elif item == "P":
            x = pool2(x)
        else:
            w, b = weights["conv"][i]
            w = w.detach().cpu().double()
            x = conv3x3_relu(x, r16(w) if round_f16 else w, b.detach().cpu())
            if round_f16:
                x = r16(x)
            i += 1
    return taps


def tap_distance(f0, f1, lin_w):
    """f0, f1 (1, C, h, w) double, lin_w (C,): d per pixel (h, w) --
    n = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (n0_c - n1_c)^2"""
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (lin_w.detach().cpu().double().view(1, -1, 1, 1) * (n0 - n1).pow(2)).sum(1)[0]


def lpips_ref(pred, target, weights, img_wh, round_f16=False):
    """-> (score, [the five per-tap means]) as python floats"""
    x = torch.cat([prepare(pred, img_wh, round_f16), prepare(target, img_wh, round_f16)])
    terms = [float(tap_distance(t[0:1], t[1:2], lw).mean())
             for t, lw in zip(features(x, weights, round_f16), weights["lin"])]
    return sum(terms), terms
