"""The inputs of a training step from a device-resident training set
(datasets/base.py:23-31: the batch's image / pixel picks and the target
gather; train_ml.py:84-96,180: the rays, the march jitter, the random
background), one HIP launch per step (rn_sample_batch, csrc/sample.hip):

    ti = TrainImages(images)                    # (N, H*W, 3) uint8 or fp32, on the device
    b = sample_batch(ti, directions, poses, n_rays, n_models, seed, step)
    b["img_idxs"], b["pix_idxs"], b["target"], b["rays_o"], b["rays_d"],
    b["imgs_d"], b["noise"], b["bg"]
    b = sample_batch(..., step + 1, out=b)      # the same buffers, no allocation

Everything random is a counter-based hash of (seed, rank, step), stated in
include/radnerf.h: no generator state, so a batch depends on its key alone,
data-parallel ranks draw different pixels, and a run resumed with its saved
global_step (Trainer.load_state) continues the stream.  cosine_lr is the schedule of train_ml.py:148-151.
"""
import math

import torch

from ._lib import lib

_DTYPES = {torch.uint8: 0, torch.float32: 1}
KEYS = ("img_idxs", "pix_idxs", "target", "rays_o", "rays_d", "imgs_d", "noise", "bg")


class TrainImages:
    """The training images as the sampler reads them: (N, H*W, 3) uint8 or
    float32, contiguous, on the device.  Nothing is converted or copied: a
    uint8 set stays uint8 (a quarter of fp32's bytes), and the targets are
    formed per pick as v / 255."""

    def __init__(self, images):
        fn = "TrainImages"
        if not torch.is_tensor(images):
            raise ValueError(f"{fn}: images must be a tensor, got {type(images).__name__}")
        if images.ndim != 3 or images.shape[2] != 3 or images.shape[0] < 1 or images.shape[1] < 1:
            raise ValueError(f"{fn}: images must be (N, H*W, 3), got {tuple(images.shape)}")
        if images.dtype not in _DTYPES:
            raise ValueError(f"{fn}: images must be uint8 or float32, got {images.dtype}")
        if not images.is_contiguous():
            raise ValueError(f"{fn}: images must be contiguous")
        if images.shape[0] >= 1 << 32 or images.shape[1] >= 1 << 32:
            raise ValueError(f"{fn}: at most 2^32 - 1 images and pixels per image, got "
                             f"{tuple(images.shape)}")
        # last of the checks: the kernel takes device pointers only
        if not images.is_cuda:
            raise ValueError(f"{fn}: images must be on the GPU, got {images.device}")
        self.images = images.detach()
        self.n_images, self.n_pix = int(images.shape[0]), int(images.shape[1])
        self.dtype_code = _DTYPES[images.dtype]
        self.device = images.device


def _f32(fn, name, t, shape):
    if not torch.is_tensor(t) or tuple(t.shape) != shape:
        raise ValueError(f"{fn}: {name} must be {shape}, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be contiguous float32")


def _buffers(n, K, with_imgs_d, dev):
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    i = lambda: torch.empty(n, device=dev, dtype=torch.int64)
    return {"img_idxs": i(), "pix_idxs": i(), "target": f(n, 3), "rays_o": f(n, 3),
            "rays_d": f(n, 3), "imgs_d": f(n, 3) if with_imgs_d else None,
            "noise": f(K, n), "bg": f(3)}


def _check_out(out, n, K, with_imgs_d, dev):
    fn = "sample_batch"
    if not isinstance(out, dict) or set(out) != set(KEYS):
        raise ValueError(f"{fn}: out must be a dict a previous call returned")
    want = {"img_idxs": ((n,), torch.int64), "pix_idxs": ((n,), torch.int64),
            "target": ((n, 3), torch.float32), "rays_o": ((n, 3), torch.float32),
            "rays_d": ((n, 3), torch.float32), "noise": ((K, n), torch.float32),
            "bg": ((3,), torch.float32)}
    if with_imgs_d:
        want["imgs_d"] = ((n, 3), torch.float32)
    elif out["imgs_d"] is not None:
        raise ValueError(f"{fn}: out['imgs_d'] is given but mean_dir is not")
    for k, (shape, dtype) in want.items():
        t = out[k]
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype \
                or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{fn}: out[{k!r}] must be a contiguous {dtype} {shape} on {dev}")


def sample_batch(train_images, directions, poses, n_rays, n_models, seed, step, rank=0,
                 dR=None, dT=None, mean_dir=None, out=None):
    """One training batch for the key (seed, step, rank): a dict of img_idxs,
    pix_idxs (n_rays) int64, target, rays_o, rays_d (n_rays, 3), imgs_d
    ((n_rays, 3) when mean_dir is given, else None), noise (n_models, n_rays)
    and bg (3).  directions (H*W, 3) and poses (N, 3, 4) are contiguous fp32
    on the images' device; dR / dT (N, 3) refine the poses as rays.pose_rays
    does (the rays are rays.batch_rays' bits on the same picks without them,
    pose_rays' with them).  out: a dict a previous call with the same sizes
    returned; its buffers are overwritten and returned."""
    fn = "sample_batch"
    if not isinstance(train_images, TrainImages):
        raise ValueError(f"{fn}: train_images must be a TrainImages")
    ti = train_images
    n, K = int(n_rays), int(n_models)
    if n < 0 or K < 1:
        raise ValueError(f"{fn}: n_rays must be >= 0 and n_models >= 1, got {n_rays}, {n_models}")
    if not 0 <= int(step) < 1 << 40:
        raise ValueError(f"{fn}: step must be in [0, 2^40), got {step}")
    if not 0 <= int(rank) < 1 << 24:
        raise ValueError(f"{fn}: rank must be in [0, 2^24), got {rank}")
    _f32(fn, "directions", directions, (ti.n_pix, 3))
    _f32(fn, "poses", poses, (ti.n_images, 3, 4))
    tensors = [directions, poses]
    for name, t in (("dR", dR), ("dT", dT)):
        if t is not None:
            _f32(fn, name, t, (ti.n_images, 3))
            tensors.append(t)
    if mean_dir is not None:
        _f32(fn, "mean_dir", mean_dir, (3,))
        tensors.append(mean_dir)
    for t in tensors:
        if t.device != ti.device:
            raise ValueError(f"{fn}: every tensor must be on the images' device {ti.device}, "
                             f"got {t.device}")
    if out is None:
        out = _buffers(n, K, mean_dir is not None, ti.device)
    else:
        _check_out(out, n, K, mean_dir is not None, ti.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    lib().sample_batch(ti.images.data_ptr(), ti.dtype_code, ti.n_images, ti.n_pix,
                       directions.data_ptr(), poses.data_ptr(), ptr(dR), ptr(dT), ptr(mean_dir),
                       int(seed) & 0xffffffffffffffff, int(step), int(rank), n, K,
                       out["img_idxs"].data_ptr(), out["pix_idxs"].data_ptr(),
                       out["target"].data_ptr(), out["rays_o"].data_ptr(),
                       out["rays_d"].data_ptr(), ptr(out["imgs_d"]), out["noise"].data_ptr(),
                       out["bg"].data_ptr(), torch.cuda.current_stream(ti.device).cuda_stream)
    return out


def cosine_lr(lr0, epoch, num_epochs, eta_min=None):
    """CosineAnnealingLR(T_max=num_epochs, eta_min) in closed form, in double:
    eta_min + (lr0 - eta_min) (1 + cos(pi epoch / num_epochs)) / 2; eta_min
    defaults to lr0 / 30 (train_ml.py:148-151)."""
    lr0 = float(lr0)
    eta_min = lr0 / 30 if eta_min is None else float(eta_min)
    if int(num_epochs) < 1:
        raise ValueError(f"cosine_lr: num_epochs must be at least 1, got {num_epochs}")
    return eta_min + (lr0 - eta_min) * (1.0 + math.cos(math.pi * epoch / int(num_epochs))) / 2.0
