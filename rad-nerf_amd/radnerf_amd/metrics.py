"""Image metrics of validation_step (train_ml.py:214-250) on the device:
PSNR and SSIM as train_ml.py:64-66 sets them up
(PeakSignalNoiseRatio(data_range=1), StructuralSimilarityIndexMeasure(
data_range=1)), on the renderer's own layout -- rgb (H*W, C) row-major, C = 3.

    psnr(pred, target)                         -> device scalar (fp64)
    ssim(pred, target, img_wh, return_map=False)
    ImageMetrics().update(pred, target, img_wh) / .compute() / .reset()
    ImageMetrics(lpips=lp): also "lpips" (lpips.py), off by default

rn_image_sse and rn_ssim (csrc/metrics.hip) sum fixed-order block partials in
double without atomics: two calls give the same bits, and nothing synchronises
with the host.  Argument errors raise ValueError naming the argument before
the library is touched.
"""
import torch

from ._lib import METRICS_WORK_BYTES, lib

WIN = 11          # the SSIM window: 11 x 11, sigma 1.5


def _check_pair(fn, pred, target):
    for name, t in (("pred", pred), ("target", target)):
        if not torch.is_tensor(t):
            raise ValueError(f"{fn}: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous")
    if pred.shape != target.shape:
        raise ValueError(f"{fn}: target shape {tuple(target.shape)} differs from pred "
                         f"{tuple(pred.shape)}")
    if pred.device != target.device:
        raise ValueError(f"{fn}: target is on {target.device}, pred on {pred.device}")


def _check_image(fn, pred, target, img_wh):
    _check_pair(fn, pred, target)
    try:
        W, H = (int(v) for v in img_wh)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: img_wh must be (W, H), got {img_wh!r}") from None
    if pred.ndim != 2 or not 1 <= pred.shape[1] <= 4:
        raise ValueError(f"{fn}: pred must be (H*W, C) with C <= 4, got {tuple(pred.shape)}")
    if H * W != pred.shape[0]:
        raise ValueError(f"{fn}: img_wh {W} x {H} = {H * W} pixels, pred has {pred.shape[0]} "
                         "rows")
    if H < WIN or W < WIN:
        raise ValueError(f"{fn}: img_wh {W} x {H}: H and W must be at least {WIN} (one "
                         f"{WIN} x {WIN} window)")
    return W, H


def _check_device(fn, pred):
    # last of the checks: the kernels take device pointers only
    if not pred.is_cuda:
        raise ValueError(f"{fn}: pred and target must be on the GPU, got {pred.device}")


_scratch = {}


def _work(dev):
    """Per-device scratch of the two kernels (block partials); calls on one
    device are ordered by its current stream."""
    w = _scratch.get(dev)
    if w is None:
        w = _scratch[dev] = torch.empty(METRICS_WORK_BYTES // 8, dtype=torch.float64, device=dev)
    return w


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def sse(pred, target):
    """Sum of squared differences, a device fp64 scalar (rn_image_sse)."""
    _check_pair("sse", pred, target)
    _check_device("sse", pred)
    out = torch.empty((), dtype=torch.float64, device=pred.device)
    lib().image_sse(pred.data_ptr(), target.data_ptr(), pred.numel(),
                    _work(pred.device).data_ptr(), out.data_ptr(), _stream(pred.device))
    return out


def psnr(pred, target):
    """PeakSignalNoiseRatio(data_range=1): 10 log10(n / sse) over all elements,
    a device fp64 scalar; inf for identical inputs, as torchmetrics gives."""
    _check_pair("psnr", pred, target)
    return 10.0 * torch.log10(pred.numel() / sse(pred, target))


def ssim(pred, target, img_wh, return_map=False):
    """StructuralSimilarityIndexMeasure(data_range=1) of two (H*W, C) images,
    img_wh = (W, H): the mean over the valid 11 x 11 Gaussian windows (what
    torchmetrics keeps after cropping its reflection-padded border), a device
    fp64 scalar.  return_map: also the (H-10, W-10, C) fp32 per-pixel map."""
    W, H = _check_image("ssim", pred, target, img_wh)
    _check_device("ssim", pred)
    C, dev = pred.shape[1], pred.device
    out = torch.empty((), dtype=torch.float64, device=dev)
    smap = torch.empty(H - WIN + 1, W - WIN + 1, C, device=dev) if return_map else None
    lib().ssim(pred.data_ptr(), target.data_ptr(), H, W, C, _work(dev).data_ptr(),
               out.data_ptr(), None if smap is None else smap.data_ptr(), _stream(dev))
    # a tensor divisor: torch divides by a python scalar as a multiplication
    # by its reciprocal, which turns an exact sum of ones into 1 - 2^-53
    score = out / torch.full_like(out, C * (H - WIN + 1) * (W - WIN + 1))
    return (score, smap) if return_map else score


class ImageMetrics:
    """Accumulator over validation images (the per-image logging and the mean
    of train_ml.py:214-258): update() per image, compute() -> {"psnr": mean,
    "ssim": mean, "per_image": [{"psnr", "ssim"}, ...]} (device fp64 scalars;
    the means are of the per-image values), reset().  lpips: a
    radnerf_amd.lpips.LPIPS of the images' size adds "lpips" to every entry
    and to the mean; None (the default) launches and returns nothing more."""

    def __init__(self, lpips=None):
        if lpips is not None:
            from .lpips import check_metric
            check_metric("ImageMetrics", lpips)
        self.lpips = lpips
        self.reset()

    def reset(self):
        self.per_image = []

    def update(self, pred, target, img_wh):
        _check_image("ImageMetrics.update", pred, target, img_wh)
        if self.lpips is not None:
            from .lpips import check_metric
            check_metric("ImageMetrics.update", self.lpips, img_wh)
        m = {"psnr": psnr(pred, target), "ssim": ssim(pred, target, img_wh)}
        if self.lpips is not None:
            m["lpips"] = self.lpips(pred, target)
        self.per_image.append(m)
        return m

    def compute(self):
        if not self.per_image:
            raise ValueError("ImageMetrics.compute: no image was given to update()")
        keys = ("psnr", "ssim") if self.lpips is None else ("psnr", "ssim", "lpips")
        out = {k: torch.stack([m[k] for m in self.per_image]).mean() for k in keys}
        out["per_image"] = list(self.per_image)
        return out
