"""The inputs of a training step from a device-resident training set
(datasets/base.py:23-31: the batch's image / pixel picks and the target
gather; train_ml.py:84-96,180: the rays, the march jitter, the random
background), one HIP launch per step (rn_sample_batch, csrc/sample.hip):

    ti = TrainImages(images)                    # (N, H*W, 3) uint8 or fp32, on the device
    b = sample_batch(ti, directions, poses, n_rays, n_models, seed, step)
    b["img_idxs"], b["pix_idxs"], b["target"], b["rays_o"], b["rays_d"],
    b["imgs_d"], b["noise"], b["bg"]
    b = sample_batch(..., step + 1, out=b)      # the same buffers, no allocation

GuidedSampler draws the same batch from the mixture of the uniform density
and a tiled map of the recent rgb error, with per-ray importance weights
(rn_sample_batch_guided and its three companions, csrc/guided.hip):

    gs = GuidedSampler(ti, (W, H), tile=16, uniform_frac=0.5, alpha=0.5)
    b = gs.sample(directions, poses, n_rays, n_models, seed, step)   # + cell_idx, ray_weight

Everything random is a counter-based hash of (seed, rank, step), stated in
include/radnerf.h: no generator state, so a batch depends on its key alone,
data-parallel ranks draw different pixels, and a run resumed with its saved
global_step (Trainer.load_state) continues the stream.  cosine_lr is the schedule of train_ml.py:148-151.
"""
import math

import torch

from . import _lib as _lib_mod
from ._lib import lib

_DTYPES = {torch.uint8: 0, torch.float32: 1}
KEYS = ("img_idxs", "pix_idxs", "target", "rays_o", "rays_d", "imgs_d", "noise", "bg")
GUIDED_KEYS = KEYS + ("cell_idx", "ray_weight")


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


DEPTH_KINDS = {"t": 0, "euclidean": 1}


class TrainDepths:
    """The training set's depth maps as rn_gather_depth reads them: (N, H*W)
    uint16 (torch.uint16, or int16 storage of the same words) or float32,
    contiguous, on the device; nothing is converted or copied.  A raw value v
    becomes the target ray parameter of its pixel's ray: kind "t", t = v *
    scale -- the z-depth for directions whose z is 1 and which are not
    normalised (ray_utils.get_ray_directions), so e.g. scale = 1 / 1000 for
    millimetre maps of a scene in metres, times the dataset's own scene scale;
    kind "euclidean", the range along the ray, t = (v * scale) / |direction|.
    A raw 0, a negative value or a NaN means "no measurement" (t = 0).
    images: the TrainImages the maps belong to; their (N, H*W) must agree."""

    def __init__(self, depths, scale=1.0, kind="t", images=None):
        fn = "TrainDepths"
        if not torch.is_tensor(depths):
            raise ValueError(f"{fn}: depths must be a tensor, got {type(depths).__name__}")
        if depths.ndim != 2 or depths.shape[0] < 1 or depths.shape[1] < 1:
            raise ValueError(f"{fn}: depths must be (N, H*W), got {tuple(depths.shape)}")
        codes = {torch.float32: 1, torch.int16: 0}
        if hasattr(torch, "uint16"):
            codes[torch.uint16] = 0
        if depths.dtype not in codes:
            raise ValueError(f"{fn}: depths must be uint16 or float32, got {depths.dtype}")
        if not depths.is_contiguous():
            raise ValueError(f"{fn}: depths must be contiguous")
        if kind not in DEPTH_KINDS:
            raise ValueError(f"{fn}: kind must be 't' or 'euclidean', got {kind!r}")
        scale = float(scale)
        if not (scale > 0.0 and scale < float("inf")):
            raise ValueError(f"{fn}: scale must be a positive finite number, got {scale!r}")
        if images is not None:
            if not isinstance(images, TrainImages):
                raise ValueError(f"{fn}: images must be a TrainImages")
            if (images.n_images, images.n_pix) != tuple(depths.shape):
                raise ValueError(f"{fn}: depths {tuple(depths.shape)} do not match the images' "
                                 f"{(images.n_images, images.n_pix)}")
        if depths.shape[0] >= 1 << 32 or depths.shape[1] >= 1 << 32:
            raise ValueError(f"{fn}: at most 2^32 - 1 maps and pixels per map, got "
                             f"{tuple(depths.shape)}")
        if not depths.is_cuda:
            raise ValueError(f"{fn}: depths must be on the GPU, got {depths.device}")
        if images is not None and images.device != depths.device:
            raise ValueError(f"{fn}: depths must be on the images' device {images.device}")
        self.depths = depths.detach()
        self.n_images, self.n_pix = int(depths.shape[0]), int(depths.shape[1])
        self.dtype_code = codes[depths.dtype]
        self.scale, self.kind, self.kind_code = scale, kind, DEPTH_KINDS[kind]
        self.device = depths.device

    def check_images(self, fn, images):
        """ValueError unless these maps have the shape and device of `images`"""
        if (images.n_images, images.n_pix) != (self.n_images, self.n_pix):
            raise ValueError(f"{fn}: depths {(self.n_images, self.n_pix)} do not match the "
                             f"images' {(images.n_images, images.n_pix)}")
        if images.device != self.device:
            raise ValueError(f"{fn}: depths must be on the images' device {images.device}")


def gather_depth(train_depths, directions, img_idxs, pix_idxs, out=None):
    """The target ray parameter of each pick, (n,) fp32 (rn_gather_depth):
    0 where the map holds no measurement.  directions (H*W, 3) as the sampler's
    (read for kind "euclidean" only); img_idxs / pix_idxs (n,) int64, e.g. a
    batch's; out: a (n,) fp32 buffer to overwrite."""
    fn = "gather_depth"
    td = train_depths
    if not isinstance(td, TrainDepths):
        raise ValueError(f"{fn}: train_depths must be a TrainDepths")
    n = int(img_idxs.shape[0])
    for name, t in (("img_idxs", img_idxs), ("pix_idxs", pix_idxs)):
        if tuple(t.shape) != (n,) or t.dtype != torch.int64 or not t.is_contiguous() \
                or t.device != td.device:
            raise ValueError(f"{fn}: {name} must be ({n},) contiguous int64 on {td.device}")
    if td.kind_code == 1:
        _f32(fn, "directions", directions, (td.n_pix, 3))
        if directions.device != td.device:
            raise ValueError(f"{fn}: directions must be on {td.device}")
    if out is None:
        out = torch.empty(n, device=td.device, dtype=torch.float32)
    else:
        _f32(fn, "out", out, (n,))
    lib().gather_depth(td.depths.data_ptr(), td.dtype_code, td.n_images, td.n_pix, td.scale,
                       td.kind_code, directions.data_ptr() if td.kind_code == 1 else None,
                       img_idxs.data_ptr(), pix_idxs.data_ptr(), n, out.data_ptr(),
                       torch.cuda.current_stream(td.device).cuda_stream)
    return out


def _f32(fn, name, t, shape):
    if not torch.is_tensor(t) or tuple(t.shape) != shape:
        raise ValueError(f"{fn}: {name} must be {shape}, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be contiguous float32")


def _buffers(n, K, with_imgs_d, dev, guided=False):
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    i = lambda: torch.empty(n, device=dev, dtype=torch.int64)
    out = {"img_idxs": i(), "pix_idxs": i(), "target": f(n, 3), "rays_o": f(n, 3),
           "rays_d": f(n, 3), "imgs_d": f(n, 3) if with_imgs_d else None,
           "noise": f(K, n), "bg": f(3)}
    if guided:
        out["cell_idx"] = torch.empty(n, device=dev, dtype=torch.int32)
        out["ray_weight"] = f(n)
    return out


def _check_out(out, n, K, with_imgs_d, dev, guided=False):
    fn = "GuidedSampler.sample" if guided else "sample_batch"
    if not isinstance(out, dict) or set(out) != set(GUIDED_KEYS if guided else KEYS):
        raise ValueError(f"{fn}: out must be a dict a previous call returned")
    want = {"img_idxs": ((n,), torch.int64), "pix_idxs": ((n,), torch.int64),
            "target": ((n, 3), torch.float32), "rays_o": ((n, 3), torch.float32),
            "rays_d": ((n, 3), torch.float32), "noise": ((K, n), torch.float32),
            "bg": ((3,), torch.float32)}
    if guided:
        want["cell_idx"] = ((n,), torch.int32)
        want["ray_weight"] = ((n,), torch.float32)
    if with_imgs_d:
        want["imgs_d"] = ((n, 3), torch.float32)
    elif out["imgs_d"] is not None:
        raise ValueError(f"{fn}: out['imgs_d'] is given but mean_dir is not")
    for k, (shape, dtype) in want.items():
        t = out[k]
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype \
                or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{fn}: out[{k!r}] must be a contiguous {dtype} {shape} on {dev}")


def _batch_args(fn, train_images, directions, poses, n_rays, n_models, step, rank, dR, dT,
                mean_dir, out, guided=False):
    """sample_batch's argument checks and its output buffers: (n, K, out)"""
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
        out = _buffers(n, K, mean_dir is not None, ti.device, guided)
    else:
        _check_out(out, n, K, mean_dir is not None, ti.device, guided)
    return n, K, out


def _ptr(t):
    return None if t is None else t.data_ptr()


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
    ti = train_images
    n, K, out = _batch_args("sample_batch", ti, directions, poses, n_rays, n_models, step, rank,
                            dR, dT, mean_dir, out)
    ptr = _ptr
    lib().sample_batch(ti.images.data_ptr(), ti.dtype_code, ti.n_images, ti.n_pix,
                       directions.data_ptr(), poses.data_ptr(), ptr(dR), ptr(dT), ptr(mean_dir),
                       int(seed) & 0xffffffffffffffff, int(step), int(rank), n, K,
                       out["img_idxs"].data_ptr(), out["pix_idxs"].data_ptr(),
                       out["target"].data_ptr(), out["rays_o"].data_ptr(),
                       out["rays_d"].data_ptr(), ptr(out["imgs_d"]), out["noise"].data_ptr(),
                       out["bg"].data_ptr(), torch.cuda.current_stream(ti.device).cuda_stream)
    return out


# ---- error-guided sampling ------------------------------------------------------
MAX_CELLS = 1 << 24


def guided_geometry(fn, n_images, n_pix, img_wh, tile):
    """(W, H, tile, tw, th, n_cells) of the tiled error map (include/radnerf.h
    "error-guided pixel sampling"); ValueError for a tile outside 1..256, W H
    != n_pix or 2^24 cells and more."""
    if isinstance(tile, bool) or int(tile) != tile or not 1 <= int(tile) <= 256:
        raise ValueError(f"{fn}: tile must be an int in 1..256, got {tile!r}")
    if img_wh is None or len(img_wh) != 2:
        raise ValueError(f"{fn}: img_wh must be (W, H), got {img_wh!r}")
    W, H, tile = int(img_wh[0]), int(img_wh[1]), int(tile)
    if W < 1 or H < 1 or W * H != int(n_pix):
        raise ValueError(f"{fn}: img_wh {(W, H)} does not match the images' {n_pix} pixels")
    tw, th = -(-W // tile), -(-H // tile)
    n_cells = int(n_images) * th * tw
    if n_cells >= MAX_CELLS:
        raise ValueError(f"{fn}: {n_images} images of {th} x {tw} tiles are {n_cells} cells, "
                         f"the map holds fewer than 2^24 (use a larger tile)")
    return W, H, tile, tw, th, n_cells


def _unit_range(fn, name, v, open_low):
    v = float(v)
    if not ((0.0 < v if open_low else 0.0 <= v) and v <= 1.0):
        raise ValueError(f"{fn}: {name} must be in {'(' if open_low else '['}0, 1], got {v!r}")
    return v


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def guided_weights(emap, n_images, img_wh, tile, w, cdf, work):
    """rn_guided_weights: w (int32 storage of the uint32 weights) and cdf
    (int64 storage of the uint64 sums) of the (n_cells,) fp32 map."""
    W, H, tile, _, _, n_cells = guided_geometry("guided_weights", n_images, img_wh[0] * img_wh[1],
                                                img_wh, tile)
    for name, t, dt in (("emap", emap, torch.float32), ("w", w, torch.int32),
                        ("cdf", cdf, torch.int64)):
        if t.numel() != n_cells or t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"guided_weights: {name} must be {n_cells} contiguous {dt} on the GPU")
    if work.numel() * work.element_size() < _lib_mod.GUIDED_WORK_BYTES or not work.is_cuda:
        raise ValueError("guided_weights: work must hold GUIDED_WORK_BYTES on the GPU")
    lib().guided_weights(emap.data_ptr(), int(n_images), W, H, tile, w.data_ptr(), cdf.data_ptr(),
                         work.data_ptr(), _stream(emap.device))


def guided_epilogue(rgb, target, cell_idx, ray_weight, n_models, acc_sum, acc_cnt, dL_drgb,
                    dL_dopacity, dL_ddepth):
    """rn_guided_epilogue: records each ray's squared rgb error in its cell's
    integer accumulators (acc_sum int64 / acc_cnt int32 storage; both None:
    nothing is recorded) and multiplies the seeds in place by ray_weight."""
    fn = "guided_epilogue"
    B, K = int(ray_weight.shape[0]), int(n_models)
    _f32(fn, "ray_weight", ray_weight, (B,))
    _f32(fn, "dL_drgb", dL_drgb, (B, 3))
    _f32(fn, "dL_dopacity", dL_dopacity, (B,))
    if dL_ddepth is not None:
        _f32(fn, "dL_ddepth", dL_ddepth, (B, K))
    n_cells = 0
    if (acc_sum is None) != (acc_cnt is None):
        raise ValueError(f"{fn}: give acc_sum and acc_cnt together")
    if acc_sum is not None:
        _f32(fn, "rgb", rgb, (B, 3))
        _f32(fn, "target", target, (B, 3))
        n_cells = acc_sum.numel()
        if acc_sum.dtype != torch.int64 or acc_cnt.dtype != torch.int32 \
                or acc_cnt.numel() != n_cells or not acc_sum.is_contiguous() \
                or not acc_cnt.is_contiguous():
            raise ValueError(f"{fn}: acc_sum must be int64 and acc_cnt int32, contiguous, of one "
                             f"length")
        if tuple(cell_idx.shape) != (B,) or cell_idx.dtype != torch.int32 \
                or not cell_idx.is_contiguous():
            raise ValueError(f"{fn}: cell_idx must be ({B},) contiguous int32")
    dev = ray_weight.device
    for t in (rgb, target, cell_idx, acc_sum, acc_cnt, dL_drgb, dL_dopacity, dL_ddepth):
        if t is not None and t.device != dev:
            raise ValueError(f"{fn}: every tensor must be on {dev}, got {t.device}")
    lib().guided_epilogue(_ptr(rgb), _ptr(target), _ptr(cell_idx), ray_weight.data_ptr(), B, K,
                          n_cells, _ptr(acc_sum), _ptr(acc_cnt), dL_drgb.data_ptr(),
                          dL_dopacity.data_ptr(), _ptr(dL_ddepth), _stream(dev))


def guided_refresh(emap, acc_sum, acc_cnt, alpha):
    """rn_guided_refresh: the visited cells move by alpha towards their mean
    recorded error; the accumulators are zeroed."""
    fn = "guided_refresh"
    alpha = _unit_range(fn, "alpha", alpha, True)
    n = emap.numel()
    if emap.dtype != torch.float32 or acc_sum.dtype != torch.int64 or acc_cnt.dtype != torch.int32 \
            or acc_sum.numel() != n or acc_cnt.numel() != n or not 1 <= n < MAX_CELLS \
            or not (emap.is_contiguous() and acc_sum.is_contiguous() and acc_cnt.is_contiguous()) \
            or not (emap.is_cuda and acc_sum.device == emap.device
                    and acc_cnt.device == emap.device):
        raise ValueError(f"{fn}: emap fp32, acc_sum int64 and acc_cnt int32 must be contiguous, "
                         f"of one length below 2^24, on one GPU")
    lib().guided_refresh(emap.data_ptr(), acc_sum.data_ptr(), acc_cnt.data_ptr(), n, alpha,
                         _stream(emap.device))


class GuidedSampler:
    """Error-guided batches (DESIGN.md §4 "Error-guided sampling"): a tiled
    map of the recent squared rgb error over the training set; a batch draws
    each ray uniformly with probability uniform_frac and in proportion to the
    map otherwise, and carries per ray the weight (1 / N) / p(pixel) that
    keeps the weighted gradient an unbiased estimate of the uniform batch's.

        gs = GuidedSampler(ti, (W, H))
        b = gs.sample(directions, poses, n_rays, n_models, seed, step)   # + cell_idx, ray_weight
        ... loss -> seeds ...
        gs.accumulate(rgb, b["target"], b["cell_idx"], b["ray_weight"], n_models,
                      dL_drgb, dL_dopacity, dL_ddepth)
        gs.refresh()                 # every few steps: the map, then w and cdf

    The map (emap, fp32, all ones when fresh) and the integer accumulators
    are the state; w and cdf are derived (integer sums: the same bits from
    any scan).  Everything is a function of the key and this state, so a run
    that saves and restores state_dict() continues bit for bit."""

    def __init__(self, train_images, img_wh, tile=16, uniform_frac=0.5, alpha=0.5):
        fn = "GuidedSampler"
        if not isinstance(train_images, TrainImages):
            raise ValueError(f"{fn}: train_images must be a TrainImages")
        ti = train_images
        self.W, self.H, self.tile, self.tw, self.th, self.n_cells = guided_geometry(
            fn, ti.n_images, ti.n_pix, img_wh, tile)
        self.uniform_frac = _unit_range(fn, "uniform_frac", uniform_frac, False)
        self.alpha = _unit_range(fn, "alpha", alpha, True)
        self.images = ti
        dev, n = ti.device, self.n_cells
        self.emap = torch.ones(n, device=dev, dtype=torch.float32)
        # int64 / int32 storage of the kernels' uint64 / uint32 words
        self.acc_sum = torch.zeros(n, device=dev, dtype=torch.int64)
        self.acc_cnt = torch.zeros(n, device=dev, dtype=torch.int32)
        self.w = torch.empty(n, device=dev, dtype=torch.int32)
        self.cdf = torch.empty(n, device=dev, dtype=torch.int64)
        self._work = torch.empty(_lib_mod.GUIDED_WORK_BYTES // 8, device=dev, dtype=torch.int64)
        self.update_weights()

    def update_weights(self):
        """w and cdf from the map as it stands (rn_guided_weights)"""
        guided_weights(self.emap, self.images.n_images, (self.W, self.H), self.tile, self.w,
                       self.cdf, self._work)

    def sample(self, directions, poses, n_rays, n_models, seed, step, rank=0, dR=None, dT=None,
               mean_dir=None, out=None):
        """sample_batch's arguments and dict, plus cell_idx (n_rays) int32 and
        ray_weight (n_rays) fp32 (rn_sample_batch_guided)."""
        ti = self.images
        n, K, out = _batch_args("GuidedSampler.sample", ti, directions, poses, n_rays, n_models,
                                step, rank, dR, dT, mean_dir, out, guided=True)
        ptr = _ptr
        lib().sample_batch_guided(
            ti.images.data_ptr(), ti.dtype_code, ti.n_images, ti.n_pix, directions.data_ptr(),
            poses.data_ptr(), ptr(dR), ptr(dT), ptr(mean_dir), int(seed) & 0xffffffffffffffff,
            int(step), int(rank), n, K, out["img_idxs"].data_ptr(), out["pix_idxs"].data_ptr(),
            out["target"].data_ptr(), out["rays_o"].data_ptr(), out["rays_d"].data_ptr(),
            ptr(out["imgs_d"]), out["noise"].data_ptr(), out["bg"].data_ptr(), self.W, self.H,
            self.tile, self.uniform_frac, self.w.data_ptr(), self.cdf.data_ptr(),
            out["cell_idx"].data_ptr(), out["ray_weight"].data_ptr(), _stream(ti.device))
        return out

    def accumulate(self, rgb, target, cell_idx, ray_weight, n_models, dL_drgb, dL_dopacity,
                   dL_ddepth=None):
        """The loss epilogue of a guided step: the rays' errors into the
        accumulators, the seeds times ray_weight in place."""
        guided_epilogue(rgb, target, cell_idx, ray_weight, n_models, self.acc_sum, self.acc_cnt,
                        dL_drgb, dL_dopacity, dL_ddepth)

    def refresh(self):
        """Fold the accumulators into the map, then recompute w and cdf."""
        guided_refresh(self.emap, self.acc_sum, self.acc_cnt, self.alpha)
        self.update_weights()

    def error_map(self):
        """the map as an (n_images, th, tw) view"""
        return self.emap.view(self.images.n_images, self.th, self.tw)

    def reset(self):
        """a fresh map: all ones, nothing accumulated"""
        self.emap.fill_(1.0)
        self.acc_sum.zero_()
        self.acc_cnt.zero_()
        self.update_weights()

    def state_dict(self):
        """emap, acc_sum, acc_cnt as CPU tensors (w and cdf are derived)"""
        return {k: getattr(self, k).detach().to("cpu", copy=True)
                for k in ("emap", "acc_sum", "acc_cnt")}

    def load_state_dict(self, state):
        want = {"emap": torch.float32, "acc_sum": torch.int64, "acc_cnt": torch.int32}
        for k, dt in want.items():
            t = state.get(k) if isinstance(state, dict) else None
            if not torch.is_tensor(t) or t.numel() != self.n_cells or t.dtype != dt:
                raise ValueError(f"GuidedSampler.load_state_dict: {k} must be {self.n_cells} "
                                 f"values of {dt}")
        with torch.no_grad():
            for k in want:
                getattr(self, k).copy_(state[k].reshape(-1).to(self.emap.device))
        self.update_weights()


def cosine_lr(lr0, epoch, num_epochs, eta_min=None):
    """CosineAnnealingLR(T_max=num_epochs, eta_min) in closed form, in double:
    eta_min + (lr0 - eta_min) (1 + cos(pi epoch / num_epochs)) / 2; eta_min
    defaults to lr0 / 30 (train_ml.py:148-151)."""
    lr0 = float(lr0)
    eta_min = lr0 / 30 if eta_min is None else float(eta_min)
    if int(num_epochs) < 1:
        raise ValueError(f"cosine_lr: num_epochs must be at least 1, got {num_epochs}")
    return eta_min + (lr0 - eta_min) * (1.0 + math.cos(math.pi * epoch / int(num_epochs))) / 2.0
