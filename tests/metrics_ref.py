"""fp64 restatements of validation_step's image metrics (train_ml.py:64-66,
214-250) for the tests: PeakSignalNoiseRatio(data_range=1) and
StructuralSimilarityIndexMeasure(data_range=1) written out in torch on the
CPU, on the renderer's (H*W, C) layout."""
import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def psnr_ref(pred, target):
    """10 log10(n / sum (p - t)^2) in fp64 (a python float; inf when equal)."""
    d = pred.detach().double().cpu() - target.detach().double().cpu()
    sse = float((d * d).sum())
    return float("inf") if sse == 0 else float(10.0 * torch.log10(torch.tensor(d.numel() / sse,
                                                                              dtype=torch.float64)))


def gaussian_window(dtype=torch.float64):
    d = torch.arange(WIN, dtype=dtype) - (WIN - 1) / 2
    g = torch.exp(-(d / SIGMA) ** 2 / 2)
    return g / g.sum()


def ssim_ref(pred, target, img_wh, dtype=torch.float64):
    """Gaussian-window SSIM over the valid windows: (mean, map (H-10, W-10,
    C)) in `dtype` on the CPU.  mu = E[x], s_xy = E[xy] - mu_x mu_y with E the
    11 x 11 Gaussian (sigma 1.5, sum 1) average."""
    W, H = img_wh
    C = pred.shape[1]
    to = lambda a: a.detach().cpu().to(dtype).view(H, W, C).permute(2, 0, 1)[:, None]
    p, t = to(pred), to(target)
    g = gaussian_window(dtype)
    k = torch.outer(g, g)[None, None]
    E = lambda x: F.conv2d(x, k)
    mp, mt = E(p), E(t)
    spp, stt, spt = E(p * p) - mp * mp, E(t * t) - mt * mt, E(p * t) - mp * mt
    v = ((2 * mp * mt + C1) * (2 * spt + C2)) / ((mp * mp + mt * mt + C1) * (spp + stt + C2))
    smap = v[:, 0].permute(1, 2, 0).contiguous()
    return float(smap.double().mean()), smap


def images(kind, img_wh, C, seed=0):
    """The tests' image pairs, fp32 (H*W, C) in [0, 1]: uniform noise; a smooth
    ramp with 5 % noise; a constant image with one outlier pixel (flat regions
    are where E[x^2] - mu^2 cancels worst)."""
    W, H = img_wh
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.rand(H * W, C, generator=g), torch.rand(H * W, C, generator=g)
    if kind == "ramp":
        y, x = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        base = torch.stack([(0.2 + 0.6 * (x + y) / 2) * (1 - 0.1 * c) for c in range(C)], -1)
        tgt = base.reshape(H * W, C).contiguous()
        pred = (tgt + 0.05 * (torch.rand(H * W, C, generator=g) - 0.5)).clamp(0, 1)
        return pred.contiguous(), tgt
    if kind == "flat":
        tgt = torch.full((H * W, C), 0.7)
        pred = tgt.clone()
        pred[(H // 2) * W + W // 2] = 0.1
        return pred, tgt
    raise ValueError(kind)
