"""Whole-image validation on the test-time chain (validation_step,
train_ml.py:214-250): one camera pose in, the rendered image and its PSNR /
SSIM against the ground truth out.

    ev = ImageEvaluator(model, gating_net, directions, img_wh)
    res = ev.render_image(pose)          # rgb (H*W,3), opacity, depth, depth_k,
                                         # gating_code (H*W,K), total_samples
    m = ev.evaluate(pose, rgb_gt)        # {"psnr", "ssim"} device scalars
    im = ev.images8()                    # uint8 (H, W, 3): rgb, depth, gate (K > 1)

Per chunk of rays: rn_get_rays (one pose, the chunk's directions by pointer
offset) -> the gate (rn_gate_fwd on rays_o / rays_d in place, written into
the image-sized gating_code) -> the AABB interval with the NEAR_DISTANCE clamp
-> rn_render_test (all sub-NeRFs in one launch) -> rn_ml_combine_test, which
writes background, gate-weighted rgb / opacity / depth and the per-sub-NeRF
depths at the chunk's rows of the image-sized outputs.  The results are those
of rendering.ml_render(test_time=True) on the same rays; everything runs on
the current stream with no host synchronisation and no per-chunk allocation.

Gate-sparse render (sparse_gate.py; include/radnerf.h rn_gate_select):
render_image / evaluate take gate_min, gate_topk and renormalize.  With
gate_min > 0 or gate_topk < K the chain is gate -> rn_gate_select ->
rn_render_test_list (only the live (ray, sub-NeRF) pairs are rendered; the dead
slots hold exact zeros) -> rn_ml_combine_test with gate_used for the gate.  The
result gains gating_live (N, K) uint8, gating_used (N, K) fp32 and pairs (the
number of live pairs, a device int64); depth_k is 0 at dead pairs,
total_samples counts live pairs, gating_code stays the full softmax.  Without
renormalize the image differs from the dense one by at most the dead gate mass
per ray.  The defaults, K = 1 and gating_net=None run the dense launches above
and return the dense dict.
"""
import torch

from . import imageout, metrics, sparse_gate
from ._lib import GATE_SELECT_WORK_BYTES, lib
from .rendering import MAX_SAMPLES, NEAR_DISTANCE

DEFAULT_CHUNK = 1 << 18


def _check_camera(fn, directions, img_wh, chunk):
    try:
        W, H = (int(v) for v in img_wh)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: img_wh must be (W, H), got {img_wh!r}") from None
    if W < 1 or H < 1:
        raise ValueError(f"{fn}: img_wh must be positive, got {W} x {H}")
    if not torch.is_tensor(directions) or directions.ndim != 2 or directions.shape[1] != 3:
        raise ValueError(f"{fn}: directions must be a (H*W, 3) tensor, got "
                         f"{tuple(getattr(directions, 'shape', ()))}")
    if directions.shape[0] != H * W:
        raise ValueError(f"{fn}: img_wh {W} x {H} = {H * W} pixels, directions has "
                         f"{directions.shape[0]} rows")
    if directions.dtype != torch.float32:
        raise ValueError(f"{fn}: directions must be float32, got {directions.dtype}")
    if not directions.is_contiguous():
        raise ValueError(f"{fn}: directions must be contiguous")
    if int(chunk) < 1:
        raise ValueError(f"{fn}: chunk must be at least 1, got {chunk}")
    return W, H


def _check_pose(fn, pose):
    if not torch.is_tensor(pose) or tuple(pose.shape) != (3, 4):
        raise ValueError(f"{fn}: pose must be a (3, 4) camera-to-world tensor, got "
                         f"{tuple(getattr(pose, 'shape', ()))}")


class ImageEvaluator:
    """Renders whole images of one camera (directions (H*W, 3), img_wh = (W,
    H)) from `model` (MNGP + gating_net, or a single NGP with gating_net=None:
    K = 1 and a gate of exactly 1).  Workspaces are sized once for `chunk`
    rays; the image-sized outputs are reused by the next render_image (clone
    what must outlive it).  exp_step_factor=None follows train_ml.py:101-102
    (1/256 beyond scale 0.5)."""

    def __init__(self, model, gating_net, directions, img_wh, chunk=DEFAULT_CHUNK,
                 exp_step_factor=None):
        W, H = _check_camera("ImageEvaluator", directions, img_wh, chunk)
        if gating_net is None and getattr(model, "size", None) != 1:
            raise ValueError("ImageEvaluator: gating_net=None needs a single-model NGP "
                             f"(model.size == 1), got size {getattr(model, 'size', None)}")
        if gating_net is not None and gating_net.out_dim != model.size:
            raise ValueError(f"ImageEvaluator: gating_net has {gating_net.out_dim} outputs for "
                             f"{model.size} sub-NeRFs")
        self.model, self.gate = model, gating_net
        self.img_wh, self.n_pix = (W, H), H * W
        dev = self.device = model.mlp_params.device
        self.directions = directions.detach().to(dev)
        self.esf = (1 / 256 if model.scale > 0.5 else 0.0) if exp_step_factor is None \
            else float(exp_step_factor)
        K, N = model.size, self.n_pix
        B = self.chunk = min(int(chunk), N)
        image_gate = gating_net is not None and gating_net.type == "image"
        self.mean_dir = self.directions.mean(0).contiguous() if image_gate else None
        f32 = dict(device=dev, dtype=torch.float32)
        # per chunk
        self.rays_o, self.rays_d = torch.empty(B, 3, **f32), torch.empty(B, 3, **f32)
        self.imgs_d = torch.empty(B, 3, **f32) if image_gate else None
        self.hits_t = torch.empty(B, 1, 2, **f32)
        self.hit_cnt = torch.empty(B, device=dev, dtype=torch.int32)
        self.hit_idx = torch.empty(B, 1, device=dev, dtype=torch.int64)
        self.op_k, self.depth_k = torch.empty(K * B, **f32), torch.empty(K * B, **f32)
        self.rgb_k = torch.empty(K * B * 3, **f32)
        self.n_smp = torch.empty(K * B, device=dev, dtype=torch.int32)
        self.importance = torch.zeros(K, **f32)          # rn_gate_fwd's by-product, unused
        self.bits = None
        # per image
        self.out = {"rgb": torch.empty(N, 3, **f32), "opacity": torch.empty(N, **f32),
                    "depth": torch.empty(N, **f32), "depth_k": torch.empty(N, K, **f32),
                    "gating_code": torch.ones(N, K, **f32)}
        # ml_rendering.py:149-153: white beyond the samples unless exp stepping
        self.bg = torch.ones(3, **f32) if self.esf == 0 else torch.zeros(3, **f32)
        self.out8 = None                                 # images8()'s buffers, on first use
        self.sparse = None                               # the sparse render's, on first use

    def _bitfields(self):
        """[K][bytes] contiguous, as rn_render_test reads them (refreshed per
        image: training updates the bitfields in place)."""
        bf = [getattr(self.model, f"density_bitfield_{i}").view(-1)
              for i in range(self.model.size)]
        if len(bf) == 1 and bf[0].is_contiguous():
            return bf[0], bf[0].numel()
        if self.bits is None or self.bits.shape[1] != bf[0].numel():
            self.bits = torch.empty(len(bf), bf[0].numel(), dtype=torch.uint8,
                                    device=self.device)
        for i, b in enumerate(bf):
            self.bits[i].copy_(b)
        return self.bits, bf[0].numel()

    def _sparse_params(self, fn, gate_min, gate_topk, renormalize):
        """None for the dense render (every pair live: the defaults, K = 1, no
        gate), else (gate_min, gate_topk, renormalize) checked.  No library."""
        K = self.model.size
        tau, k = sparse_gate.check_params(fn, K, gate_min, gate_topk)
        if self.gate is None or sparse_gate.is_dense(K, tau, k):
            return None
        return tau, k, int(bool(renormalize))

    def _sparse_buffers(self):
        if self.sparse is None:
            K, N, B, dev = self.model.size, self.n_pix, self.chunk, self.device
            self.sparse = {
                "live": torch.empty(N, K, dtype=torch.uint8, device=dev),
                "used": torch.empty(N, K, dtype=torch.float32, device=dev),
                "list": torch.empty(K * B, dtype=torch.int32, device=dev),
                "count": torch.empty(K, dtype=torch.int32, device=dev),
                "work": torch.empty(GATE_SELECT_WORK_BYTES, dtype=torch.uint8, device=dev)}
        return self.sparse

    @torch.no_grad()
    def render_image(self, pose, T_threshold=1e-4, max_samples=MAX_SAMPLES, gate_min=0.0,
                     gate_topk=None, renormalize=False):
        _check_pose("ImageEvaluator.render_image", pose)
        sp = self._sparse_params("ImageEvaluator.render_image", gate_min, gate_topk, renormalize)
        m, g, dev, L = self.model, self.gate, self.device, lib()
        K, N = m.size, self.n_pix
        pose = pose.detach().to(dev, torch.float32).contiguous()
        st = torch.cuda.current_stream(dev).cuda_stream
        bits, nb = self._bitfields()
        enc = m.xyz_encoder
        lo, lh, lr, ls = enc.level_ptrs()
        grid16, frags = enc.params_f16(), m.packed_frags()
        gfrags = None if g is None else g.packed_frags()
        out = self.out
        total = torch.zeros((), device=dev, dtype=torch.int64)
        if sp is not None:
            sb = self._sparse_buffers()
            pairs = torch.zeros((), device=dev, dtype=torch.int64)
        ptr = lambda t: None if t is None else t.data_ptr()
        for ray0 in range(0, N, self.chunk):
            n = min(self.chunk, N - ray0)
            L.get_rays(self.directions.data_ptr() + 12 * ray0, pose.data_ptr(), None, None, n,
                       ptr(self.mean_dir), self.rays_o.data_ptr(), self.rays_d.data_ptr(),
                       ptr(self.imgs_d), st)
            gate_ptr = None
            if g is not None:
                second = self.imgs_d if self.imgs_d is not None else self.rays_d
                gate_ptr = out["gating_code"].data_ptr() + 4 * K * ray0
                L.gate_fwd(self.rays_o.data_ptr(), second.data_ptr(), 3, n, K, gfrags.data_ptr(),
                           gate_ptr, self.importance.data_ptr(),
                           max(1, min(256, (n + 127) // 128)), st)
            # ml_rendering.py:48-50: the box interval, a near hit inside
            # NEAR_DISTANCE moved out to it
            L.ray_aabb_intersect(self.rays_o.data_ptr(), self.rays_d.data_ptr(),
                                 m.center.data_ptr(), m.half_size.data_ptr(), n, 1, 1,
                                 self.hit_cnt.data_ptr(), self.hits_t.data_ptr(),
                                 self.hit_idx.data_ptr(), st)
            near = self.hits_t[:n, 0, 0]
            near.masked_fill_((near >= 0) & (near < NEAR_DISTANCE), NEAR_DISTANCE)
            render = (self.rays_o.data_ptr(), self.rays_d.data_ptr(), self.hits_t.data_ptr(),
                      n, K, bits.data_ptr(), nb, m.cascades, float(m.scale), self.esf,
                      m.grid_size, int(max_samples), grid16.data_ptr(), lo, lh, lr, ls,
                      m._h_min.ctypes.data, m._h_ext.ctypes.data, frags.data_ptr(),
                      float(T_threshold), self.op_k.data_ptr(), self.depth_k.data_ptr(),
                      self.rgb_k.data_ptr(), self.n_smp.data_ptr())
            blocks = max(1, min((n + 3) // 4, 512 // K))
            if sp is None:
                L.render_test(*render, blocks, st)
            else:
                # the dead slots of the per-pair buffers become zeros, the live
                # ones are rendered: the combine then adds exact zeros
                used_ptr = sb["used"].data_ptr() + 4 * K * ray0
                L.gate_select(gate_ptr, n, K, sp[0], sp[1], sp[2],
                              sb["live"].data_ptr() + K * ray0, used_ptr, sb["list"].data_ptr(),
                              sb["count"].data_ptr(), self.op_k.data_ptr(),
                              self.depth_k.data_ptr(), self.rgb_k.data_ptr(),
                              self.n_smp.data_ptr(), sb["work"].data_ptr(), st)
                L.render_test_list(*render, sb["list"].data_ptr(), sb["count"].data_ptr(),
                                   blocks, st)
                pairs += sb["count"].sum()
                gate_ptr = used_ptr
            L.ml_combine_test(gate_ptr, self.op_k.data_ptr(), self.depth_k.data_ptr(),
                              self.rgb_k.data_ptr(), self.bg.data_ptr(), n, K, ray0,
                              out["rgb"].data_ptr(), out["opacity"].data_ptr(),
                              out["depth"].data_ptr(), out["depth_k"].data_ptr(), st)
            total += self.n_smp[:K * n].sum()
        res = dict(out)
        res["total_samples"] = total
        if sp is not None:
            res["gating_live"], res["gating_used"], res["pairs"] = sb["live"], sb["used"], pairs
        return res

    def evaluate(self, pose, rgb_gt, T_threshold=1e-4, max_samples=MAX_SAMPLES, gate_min=0.0,
                 gate_topk=None, renormalize=False, lpips=None):
        """validation_step's two numbers for one image: rgb_gt (H*W, 3) fp32
        on the device -> {"psnr", "ssim"} (device fp64 scalars).  gate_min /
        gate_topk / renormalize: the gate-sparse render, as render_image.
        lpips: a radnerf_amd.lpips.LPIPS of this camera's size adds "lpips"
        (--eval_lpips); None launches and returns nothing more."""
        fn = "ImageEvaluator.evaluate"
        if lpips is not None:
            from .lpips import check_metric
            check_metric(fn, lpips, self.img_wh)
        if not torch.is_tensor(rgb_gt) or tuple(rgb_gt.shape) != (self.n_pix, 3):
            raise ValueError(f"{fn}: rgb_gt must be a ({self.n_pix}, 3) tensor, got "
                             f"{tuple(getattr(rgb_gt, 'shape', ()))}")
        # dtype, contiguity and the 11 x 11 window, before anything is rendered
        metrics._check_image(fn, rgb_gt, rgb_gt, self.img_wh)
        _check_pose("ImageEvaluator.evaluate", pose)
        rgb = self.render_image(pose, T_threshold, max_samples, gate_min, gate_topk,
                                renormalize)["rgb"]
        out = {"psnr": metrics.psnr(rgb, rgb_gt), "ssim": metrics.ssim(rgb, rgb_gt, self.img_wh)}
        if lpips is not None:
            out["lpips"] = lpips(rgb, rgb_gt)
        return out

    def images8(self, swap_rb=False, hard_gate=False):
        """The pictures validation_step saves (train_ml.py:238-248), from the
        buffers the last render_image filled: device uint8 (H, W, 3) tensors
        "rgb" ((rgb * 255).astype(uint8)), "depth" (depth2img of the
        gate-weighted depth, train_ml.py:243; swap_rb: red and blue exchanged,
        as the reference's files) and, for K > 1, "gate" (imageout.gate2img of
        the gating code, default palette; hard_gate: the first maximal gate's
        colour).  The buffers are the evaluator's own, reused by the next call;
        nothing synchronises with the host."""
        W, H = self.img_wh
        K = self.model.size
        if self.out8 is None:
            self.out8 = {k: torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)
                         for k in (("rgb", "depth", "gate") if K > 1 else ("rgb", "depth"))}
        out, out8 = self.out, self.out8
        imageout.to_uint8(out["rgb"], out=out8["rgb"])
        imageout.depth2img(out["depth"], swap_rb=swap_rb, out=out8["depth"])
        if K > 1:
            imageout.gate2img(out["gating_code"], hard=hard_gate, out=out8["gate"])
        return dict(out8)
