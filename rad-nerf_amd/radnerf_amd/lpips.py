"""LPIPS (VGG) on the device: the third number of the reference's validation
step (train_ml.py:64-70, --eval_lpips), the distance of the `lpips` package
0.1 with net `vgg` -- what LearnedPerceptualImagePatchSimilarity('vgg')
computes on clip(rgb * 2 - 1, -1, 1) -- on the renderer's own layout: rgb
(H*W, 3) fp32 in [0, 1], img_wh = (W, H).

    lp = LPIPS.from_files("vgg16.pth", "lpips_vgg.pth", img_wh)   # the user's files
    lp = LPIPS(synthetic_weights(0), img_wh)                      # tests, timing
    d = lp(pred, target)             # device fp64 scalar
    t = lp.layers(pred, target)      # the five per-tap terms, (5,) fp64; d = t.sum()

The operation (include/radnerf.h "LPIPS" has the kernels' operation order):
v = clip(2 x - 1, -1, 1), (v - shift) / scale per channel; VGG16 `features`
(13 3 x 3 convolutions with bias and ReLU, a 2 x 2 max-pool between the five
groups) with taps after relu1_2, 2_2, 3_3, 4_3, 5_3; per tap and pixel
n = f / (sqrt(sum f^2) + 1e-10) for both images, d = sum_c w_c (n0_c - n1_c)^2
with the non-negative `lin` weights, the mean of d over the tap's pixels; the
score is the sum of the five means.  Activations are stored as f16 (the
prepared input, the weights and every post-ReLU activation are the rounding
points), accumulation is fp32, the pixel sums are fixed-order doubles.

The constructor packs the weights into MFMA fragments and allocates the
activation buffers for its image size once; a call is 24 library calls on the
current stream (both images in every convolution, pool and distance), allocates
only its five-double result and never synchronises with the host.  Two calls on the same inputs
give the same bits.  Argument errors raise ValueError naming the argument
before the library is touched.  Nothing is fetched from anywhere: the two
weight files are the user's (INTEGRATION.md says where they come from).
"""
import torch

from . import metrics
from ._lib import METRICS_WORK_BYTES, lib

# VGG16 `features`: (Cin, Cout) per convolution, "P" a 2 x 2 max-pool
VGG16 = ((3, 64), (64, 64), "P", (64, 128), (128, 128), "P", (128, 256), (256, 256), (256, 256),
         "P", (256, 512), (512, 512), (512, 512), "P", (512, 512), (512, 512), (512, 512))
CONVS = tuple(c for c in VGG16 if c != "P")
TAPS = (1, 3, 6, 9, 12)                     # convolution index of relu1_2 ... relu5_3
TAP_CHANNELS = tuple(CONVS[i][1] for i in TAPS)
# torchvision's vgg16().features indices of the 13 convolutions
FEATURE_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
MIN_SIDE = 16                               # four pools: relu5_3 has a pixel
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def synthetic_weights(seed=0):
    """Weights of the real shapes from a seed (tests, timing): He-normal
    convolutions (std sqrt(2 / (9 Cin))), biases uniform in +-0.1, `lin`
    uniform in [0, 1) normalised to sum 1 per tap.  CPU fp32."""
    g = torch.Generator().manual_seed(int(seed))
    conv = []
    for cin, cout in CONVS:
        w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        b = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
        conv.append((w, b))
    lin = []
    for c in TAP_CHANNELS:
        v = torch.rand(c, generator=g)
        lin.append(v / v.sum())
    return {"conv": conv, "lin": lin}


def check_weights(fn, weights):
    """{"conv": 13 (weight (Cout, Cin, 3, 3), bias (Cout,)), "lin": 5 (C,)},
    fp32 CPU copies of it; ValueError naming what is wrong."""
    if not isinstance(weights, dict) or "conv" not in weights or "lin" not in weights:
        raise ValueError(f'{fn}: weights must be a dict {{"conv": [...], "lin": [...]}}')
    conv, lin = weights["conv"], weights["lin"]
    if len(conv) != len(CONVS):
        raise ValueError(f'{fn}: weights["conv"] must hold {len(CONVS)} (weight, bias) pairs, '
                         f"got {len(conv)}")
    if len(lin) != len(TAPS):
        raise ValueError(f'{fn}: weights["lin"] must hold {len(TAPS)} vectors, got {len(lin)}')
    out = {"conv": [], "lin": []}
    for i, ((cin, cout), pair) in enumerate(zip(CONVS, conv)):
        try:
            w, b = pair
        except (TypeError, ValueError):
            raise ValueError(f'{fn}: weights["conv"][{i}] must be a (weight, bias) pair') from None
        if not torch.is_tensor(w) or tuple(w.shape) != (cout, cin, 3, 3):
            raise ValueError(f'{fn}: weights["conv"][{i}] weight must be ({cout}, {cin}, 3, 3), '
                             f"got {tuple(getattr(w, 'shape', ()))}")
        if not torch.is_tensor(b) or tuple(b.shape) != (cout,):
            raise ValueError(f'{fn}: weights["conv"][{i}] bias must be ({cout},), got '
                             f"{tuple(getattr(b, 'shape', ()))}")
        out["conv"].append((w.detach().to("cpu", torch.float32), b.detach().to("cpu", torch.float32)))
    for i, (c, v) in enumerate(zip(TAP_CHANNELS, lin)):
        if not torch.is_tensor(v) or v.numel() != c or v.ndim not in (1, 4) or \
                (v.ndim == 4 and tuple(v.shape) != (1, c, 1, 1)):
            raise ValueError(f'{fn}: weights["lin"][{i}] must be ({c},), got '
                             f"{tuple(getattr(v, 'shape', ()))}")
        v = v.detach().to("cpu", torch.float32).reshape(c)
        if not bool((v >= 0).all()):
            raise ValueError(f'{fn}: weights["lin"][{i}] has a negative (or NaN) weight; the '
                             "lin layers of LPIPS are non-negative")
        out["lin"].append(v)
    return out


def weights_from_state_dicts(backbone, lin, fn="LPIPS.from_files"):
    """A torchvision VGG16 state dict (features.{0,2,...,28}.{weight,bias})
    and the lpips package's vgg.pth (lin{0..4}.model.1.weight, (1, C, 1, 1))
    -> the weights dict.  A missing key, a wrong shape or a negative lin
    weight is a ValueError naming it."""
    conv = []
    for (cin, cout), k in zip(CONVS, FEATURE_KEYS):
        pair = []
        for part, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = f"features.{k}.{part}"
            if key not in backbone:
                raise ValueError(f"{fn}: the backbone file has no {key}")
            t = backbone[key]
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"{fn}: {key} must be {shape}, got "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            pair.append(t)
        conv.append(tuple(pair))
    vec = []
    for i, c in enumerate(TAP_CHANNELS):
        key = f"lin{i}.model.1.weight"
        if key not in lin:
            raise ValueError(f"{fn}: the lin file has no {key}")
        t = lin[key]
        if not torch.is_tensor(t) or tuple(t.shape) != (1, c, 1, 1):
            raise ValueError(f"{fn}: {key} must be (1, {c}, 1, 1), got "
                             f"{tuple(getattr(t, 'shape', ()))}")
        if not bool((t >= 0).all()):
            raise ValueError(f"{fn}: {key} has a negative (or NaN) weight")
        vec.append(t.reshape(c))
    return check_weights(fn, {"conv": conv, "lin": vec})


def pack_conv(w):
    """(Cout, Cin, 3, 3) fp32 -> the f16 MFMA fragments rn_conv3x3_relu_f16
    reads (include/radnerf.h has the index formula), a flat CPU tensor."""
    cout, cin = w.shape[:2]
    h = w.to(torch.float16)
    if cin == 3:
        k = torch.zeros(cout, 32, dtype=torch.float16)
        k[:, :27] = h.permute(0, 2, 3, 1).reshape(cout, 27)          # k = 3 tap + c
        # (ct, r, ks, h, j) -> (ct, ks, h, r, j)
        return k.reshape(cout // 32, 32, 2, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    # (ct, r, chunk, ks, h, j, tap) -> (ct, chunk, tap, ks, h, r, j)
    f = h.reshape(cout // 32, 32, cin // 64, 4, 2, 8, 9)
    return f.permute(0, 2, 6, 3, 4, 1, 5).contiguous().view(-1)


def _check_wh(fn, img_wh):
    try:
        W, H = (int(v) for v in img_wh)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: img_wh must be (W, H), got {img_wh!r}") from None
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"{fn}: img_wh {W} x {H}: H and W must be at least {MIN_SIDE} (four "
                         "2 x 2 pools leave relu5_3 one pixel)")
    return W, H


def check_metric(fn, lp, img_wh=None):
    """The `lpips=` argument of ImageMetrics / ImageEvaluator.evaluate /
    Trainer.validate: None or an LPIPS, built for this image size (if given)."""
    if lp is None:
        return
    if not isinstance(lp, LPIPS):
        raise ValueError(f"{fn}: lpips must be None or a radnerf_amd.lpips.LPIPS, got "
                         f"{type(lp).__name__}")
    if img_wh is not None and tuple(int(v) for v in img_wh) != lp.img_wh:
        raise ValueError(f"{fn}: lpips was built for img_wh {lp.img_wh}, the images are "
                         f"{tuple(int(v) for v in img_wh)}")


class LPIPS:
    """The LPIPS-VGG distance of two (H*W, 3) fp32 images in [0, 1] of one
    size.  weights: {"conv": 13 (weight, bias) pairs, "lin": 5 vectors}
    (synthetic_weights, weights_from_state_dicts); img_wh = (W, H), both at
    least 16; device: a GPU (None: the current one)."""

    def __init__(self, weights, img_wh, device=None):
        W, H = _check_wh("LPIPS", img_wh)
        wts = check_weights("LPIPS", weights)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"LPIPS: device must be a GPU, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.img_wh, self.device = (W, H), dev
        self.frags = [pack_conv(w).to(dev) for w, _ in wts["conv"]]
        self.bias = [b.contiguous().to(dev) for _, b in wts["conv"]]
        self.lin = [v.contiguous().to(dev) for v in wts["lin"]]
        f16 = dict(device=dev, dtype=torch.float16)
        # both images side by side: the prepared input and two buffers the
        # layers alternate between (the first group, 64 channels at full size,
        # is the largest activation)
        self.x = torch.empty(2, H, W, 3, **f16)
        self.buf = [torch.empty(2 * H * W * 64, **f16) for _ in range(2)]
        self.work = torch.empty(METRICS_WORK_BYTES // 8, dtype=torch.float64, device=dev)
        sizes, h, w = [], H, W
        for _ in TAPS:
            sizes.append(h * w)
            h, w = h // 2, w // 2
        self.tap_pixels = torch.tensor(sizes, dtype=torch.float64, device=dev)

    @classmethod
    def from_files(cls, backbone_path, lin_path, img_wh, device=None):
        """backbone_path: a torchvision VGG16 state dict; lin_path: the lpips
        package's weights/v0.1/vgg.pth.  Both are read with weights_only=True."""
        _check_wh("LPIPS.from_files", img_wh)
        backbone = torch.load(backbone_path, map_location="cpu", weights_only=True)
        lin = torch.load(lin_path, map_location="cpu", weights_only=True)
        for name, d in (("backbone_path", backbone), ("lin_path", lin)):
            if not isinstance(d, dict):
                raise ValueError(f"LPIPS.from_files: {name} must hold a state dict, got "
                                 f"{type(d).__name__}")
        return cls(weights_from_state_dicts(backbone, lin), img_wh, device)

    def _check(self, fn, pred, target):
        W, H = metrics._check_image(fn, pred, target, self.img_wh)
        if pred.shape[1] != 3:
            raise ValueError(f"{fn}: pred must be (H*W, 3), got {tuple(pred.shape)}")
        metrics._check_device(fn, pred)
        if pred.device != self.device:
            raise ValueError(f"{fn}: pred is on {pred.device}, this LPIPS on {self.device}")
        return W, H

    def layers(self, pred, target):
        """The five per-tap terms (relu1_2 ... relu5_3), a (5,) device fp64
        tensor; their sum is the score."""
        W, H = self._check("LPIPS.layers", pred, target)
        L, dev = lib(), self.device
        st = torch.cuda.current_stream(dev).cuda_stream
        n = H * W
        L.lpips_prepare(pred.data_ptr(), n, self.x.data_ptr(), st)
        L.lpips_prepare(target.data_ptr(), n, self.x.data_ptr() + 6 * n, st)
        sums = torch.empty(len(TAPS), dtype=torch.float64, device=dev)
        src, which, h, w, conv, tap = self.x.data_ptr(), 0, H, W, 0, 0
        for item in VGG16:
            dst = self.buf[which].data_ptr()
            if item == "P":
                c = CONVS[conv - 1][1]
                L.maxpool2_f16(src, 2, h, w, c, dst, st)
                h, w = h // 2, w // 2
            else:
                cin, cout = item
                L.conv3x3_relu_f16(src, self.frags[conv].data_ptr(), self.bias[conv].data_ptr(),
                                   2, h, w, cin, cout, dst, st)
                if conv == TAPS[tap]:
                    L.lpips_layer(dst, dst + 2 * h * w * cout, self.lin[tap].data_ptr(), h * w,
                                  cout, self.work.data_ptr(), sums.data_ptr() + 8 * tap, st)
                    tap += 1
                conv += 1
            src, which = dst, 1 - which
        # a tensor divisor, as metrics.ssim: an exact quotient, not a product
        # with a rounded reciprocal
        return sums / self.tap_pixels

    def __call__(self, pred, target):
        """The LPIPS distance, a device fp64 scalar (the five terms added in
        tap order)."""
        self._check("LPIPS", pred, target)
        t = self.layers(pred, target)
        return (((t[0] + t[1]) + t[2]) + t[3]) + t[4]
