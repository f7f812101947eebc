"""NeRFLoss of the reference (losses.py:39-76) in two forms.

`NeRFLoss`         the reference module: a dict of loss tensors built from torch
                   ops (autograd), for callers that keep the reference training
                   loop (`loss = sum(l.mean() for l in loss_d.values())`).
`fused_nerf_loss`  one HIP pass (rn_nerf_loss) that returns the per-term means
                   AND the seeds dL/drgb, dL/dopacity, dL/ddepth, dL/dgate of
                   `sum(term.mean())`; FusedMLRenderer.train_step feeds them
                   straight into the fused backward (no autograd graph).

`DistortionLoss`    the reference autograd Function (losses.py:6-36) on the HIP
                   distortion kernels (vren.distortion_loss_fw / _bw).
"""
import torch
from torch import nn

from . import vren
from ._lib import lib


class DistortionLoss(torch.autograd.Function):
    """losses.py:6-36: Mip-NeRF 360 distortion loss (DVGO-v2 form) per ray.
    Inputs ws, deltas, ts (N) and rays_a (N_rays, 3); output loss (N_rays)."""

    @staticmethod
    def forward(ctx, ws, deltas, ts, rays_a):
        loss, ws_incl, wts_incl = vren.distortion_loss_fw(
            ws.float().contiguous(), deltas.float().contiguous(), ts.float().contiguous(),
            rays_a.contiguous())
        ctx.save_for_backward(ws_incl, wts_incl, ws, deltas, ts, rays_a)
        return loss

    @staticmethod
    def backward(ctx, dL_dloss):
        ws_incl, wts_incl, ws, deltas, ts, rays_a = ctx.saved_tensors
        dL_dws = vren.distortion_loss_bw(dL_dloss.float().contiguous(), ws_incl, wts_incl,
                                         ws.float().contiguous(), deltas.float().contiguous(),
                                         ts.float().contiguous(), rays_a.contiguous())
        return dL_dws, None, None, None


class NeRFLoss(nn.Module):
    """losses.py:39-76."""

    def __init__(self, lambda_opacity=1e-3):
        super().__init__()

    def forward(self, results, target, lambda_opacity=1e-3, lambda_distortion=0, lambda_disp=0,
                lambda_cv_importance=0, lambda_depth_mutual=0, lambda_depth=0,
                lambda_depth_var=0, depth_clip=float("inf")):
        """lambda_depth / lambda_depth_var > 0: depth supervision against
        target["depth"] ((B,) ray parameters, <= 0 where there is no
        measurement), both divided by B (not the valid count):
        "depth" = lambda_depth sum_r m_r (sum_k g D - z)^2 / B and "depth_var" =
        lambda_depth_var sum_r m_r sum_k g V / B, g the gate the render was
        combined with (results["gating_used"] on a routed render) and V
        results["depth_var"] (ml_render(depth_target=...) on the fused chain)
        or, without that key, composed_depth_var on the per-sub-NeRF keys."""
        from .fused import check_depth_args
        depth_on = check_depth_args("NeRFLoss", results["rgb"].shape[0], target.get("depth"),
                                    lambda_depth, lambda_depth_var, depth_clip,
                                    device=results["rgb"].device)
        loss = {}
        loss["rgb"] = (results["rgb"] - target["rgb"]) ** 2
        o = results["opacity"] + 1e-10
        loss["opacity"] = lambda_opacity * (-o * torch.log(o))
        if lambda_disp > 0:
            loss["disp"] = lambda_disp * results["disp"] ** 2
        K = results["gating_code"].shape[-1]
        if lambda_distortion > 0 and "distortion" in results:
            # the render's own per-ray loss of every sub-NeRF, (B, K) (or (B,)
            # from render()): ml_render(..., distortion=True) on either chain
            dist = results["distortion"]
            dist = dist[:, None] if dist.dim() == 1 else dist
            loss["distortion"] = lambda_distortion * sum(
                dist[:, i].mean() for i in range(dist.shape[1]))
        elif lambda_distortion > 0:
            # per sub-NeRF keys ws_i / deltas_i / ts_i / rays_a_i (losses.py:63-67)
            loss["distortion"] = 0
            for i in range(K):
                loss["distortion"] += lambda_distortion * DistortionLoss.apply(
                    results[f"ws_{i}"], results[f"deltas_{i}"], results[f"ts_{i}"],
                    results[f"rays_a_{i}"]).mean()
        if lambda_cv_importance > 0 and K > 1:
            imp = results["gating_importance"].float()
            loss["cv_importance"] = lambda_cv_importance * imp.var() / (imp.mean() ** 2 + 1e-10)
        if lambda_depth_mutual > 0 and K > 1:
            d = results["depth"]
            loss["depth_mutual"] = lambda_depth_mutual * (
                (d - torch.sum(d * results["gating_code"], 1, keepdim=True).detach()) ** 2)
        if depth_on:
            z = target["depth"].float()
            m = (z > 0).float()
            B = z.shape[0]
            g = results.get("gating_used", results["gating_code"]).float()
            if lambda_depth > 0:
                e = torch.sum(g * results["depth"].float(), 1) - z
                loss["depth"] = lambda_depth * torch.sum(m * e * e) / B
            if lambda_depth_var > 0:
                V = results["depth_var"] if "depth_var" in results else composed_depth_var(
                    results, z, depth_clip)
                loss["depth_var"] = lambda_depth_var * torch.sum(m[:, None] * g * V.float()) / B
        return loss


def composed_depth_var(results, target_t, depth_clip=float("inf")):
    """The ray-termination second moment of every sub-NeRF about the per-ray
    target, (B, K), from torch ops on the reference's per-sub-NeRF keys ws_i /
    ts_i / rays_a_i (ml_render(fused=False, distortion=True) returns them):
    V[r, i] = sum over the samples of ray r's segment of ws min((ts - z_r)^2,
    clip^2), 0 for z_r <= 0.  Differentiable in ws_i; the op-by-op form the
    in-chain term (results["depth_var"]) is compared against."""
    K = results["gating_code"].shape[-1]
    z = target_t.float()
    cols = []
    for i in range(K):
        ws, ts, rays_a = results[f"ws_{i}"], results[f"ts_{i}"], results[f"rays_a_{i}"].long()
        ray, inside = _ray_of(rays_a, ws.shape[0])
        zs = z[ray]
        phi = ((ts.float() - zs) ** 2).clamp(max=float(depth_clip) ** 2)
        term = torch.where(inside & (zs > 0), ws.float() * phi, torch.zeros_like(phi))
        cols.append(torch.zeros_like(z).index_add(0, ray, term))
    return torch.stack(cols, 1)


def _ray_of(rays_a, n):
    """(ray index, inside a segment) of each of n sample slots from rays_a rows
    (ray, start, count) whose segments lie back to back in row order."""
    if rays_a.shape[0] == 0 or n == 0:
        z = torch.zeros(n, dtype=torch.long, device=rays_a.device)
        return z, z.bool()
    order = torch.argsort(rays_a[:, 1], stable=True)
    starts = rays_a[order, 1].contiguous()
    idx = torch.arange(n, device=rays_a.device)
    seg = order[(torch.searchsorted(starts, idx, right=True) - 1).clamp_min(0)]
    inside = (idx >= rays_a[seg, 1]) & (idx < rays_a[seg, 1] + rays_a[seg, 2])
    return rays_a[seg, 0], inside


def fused_depth_loss(depth, gate, dvar_k, target_t, ray_weight, lambda_depth, lambda_depth_var,
                     d_depth, d_gate):
    """rn_depth_loss after the loss kernel (and the guided epilogue): the
    expected-depth term lambda_depth / B sum_r m_r (sum_k g D - z)^2 and the
    ray-termination term lambda_depth_var / B sum_r m_r sum_k g V (m_r = z_r >
    0; dvar_k [K][B] from FusedMLRenderer.forward(depth_target=...), or None
    for the mean term alone), their seeds added into d_depth and d_gate
    ((B, K), gate being the one the render was combined with) and the seed on
    dvar_k returned ([K][B], or None).  ray_weight multiplies every seed; the
    returned terms stay unweighted.  The terms are ordered sums: the same bits
    from call to call."""
    B, K = gate.shape
    dev = gate.device
    c = lambda t: None if t is None else t.float().contiguous()
    depth, gate, dvar_k, target_t, ray_weight = map(c, (depth, gate, dvar_k, target_t, ray_weight))
    assert depth.shape == (B, K) and target_t.shape == (B,)
    assert dvar_k is None or dvar_k.shape == (K, B)
    assert ray_weight is None or ray_weight.shape == (B,)
    for t in (depth, dvar_k, target_t, ray_weight, d_depth, d_gate):
        assert t is None or t.device == dev, "fused_depth_loss: every tensor on the gate's device"
    for t in (d_depth, d_gate):         # added to in place
        assert t.shape == (B, K) and t.dtype == torch.float32 and t.is_contiguous()
    out = torch.empty(2, device=dev)
    part = torch.empty((B + 255) // 256, 2, device=dev)
    d_dvar = None if dvar_k is None else torch.empty(K, B, device=dev)
    lib().depth_loss(depth.data_ptr(), gate.data_ptr(),
                     None if dvar_k is None else dvar_k.data_ptr(), target_t.data_ptr(),
                     None if ray_weight is None else ray_weight.data_ptr(), B, K,
                     float(lambda_depth), float(lambda_depth_var), out.data_ptr(),
                     part.data_ptr(), d_depth.data_ptr(), d_gate.data_ptr(),
                     None if d_dvar is None else d_dvar.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
    terms = {}
    if lambda_depth > 0:
        terms["depth"] = out[0] / B
    if lambda_depth_var > 0:
        terms["depth_var"] = out[1] / B
    return terms, d_dvar


def fused_nerf_loss(rgb, target_rgb, opacity, depth, gate, importance, lambda_opacity=1e-3,
                    lambda_cv_importance=0.0, lambda_depth_mutual=0.0, lambda_distortion=0.0,
                    dist_k=None, deterministic=False, live=None):
    """Returns ({term: mean (0-d tensor)}, (dL_drgb, dL_dopacity, dL_ddepth, dL_dgate))
    for loss = sum of the term means.  All inputs fp32 CUDA, contiguous.
    lambda_distortion > 0 with dist_k (the [K][B] per-segment distortion loss
    of FusedMLRenderer.forward(distortion=True)) reports terms["distortion"] =
    lambda * sum_k mean_rays; its seed, the constant lambda / B per segment,
    goes to FusedMLRenderer.backward(dL_ddist=...).
    deterministic=True sums the per-ray terms as per-block partials added in
    block order (rn_nerf_loss_det) instead of one fp32 atomic per block: the
    same seeds bit for bit, and terms that do not vary from run to run.
    live ((B, K) uint8, a routed step): `gate` is then gate_used, a dead
    pair adds nothing to the depth-mutual term and gets dL_ddepth = 0 (the
    divisor stays B K); `importance` is still the softmax gate's column sums
    and dL_dgate the seed on that gate (rn_nerf_loss_routed / _det)."""
    B, K = gate.shape
    dev = rgb.device
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    out = f(4)
    d_rgb, d_op, d_depth, d_gate = f(B, 3), f(B), f(B, K), f(B, K)
    c = lambda t: t.float().contiguous()
    rgb, target_rgb, opacity, depth, gate, importance = map(
        c, (rgb, target_rgb, opacity, depth, gate, importance))
    if live is not None:
        assert live.shape == (B, K) and live.dtype == torch.uint8 and live.is_contiguous()
    head = (rgb.data_ptr(), target_rgb.data_ptr(), opacity.data_ptr(), depth.data_ptr(),
            gate.data_ptr(), *(() if live is None else (live.data_ptr(),)),
            importance.data_ptr(), B, K, float(lambda_opacity),
            float(lambda_cv_importance), float(lambda_depth_mutual), out.data_ptr())
    seeds = (d_rgb.data_ptr(), d_op.data_ptr(), d_depth.data_ptr(), d_gate.data_ptr(),
             torch.cuda.current_stream(dev).cuda_stream)
    L = lib()
    if deterministic:
        part = f((B + 255) // 256, 4)
        (L.nerf_loss_det if live is None else L.nerf_loss_routed_det)(
            *head, part.data_ptr(), *seeds)
    else:
        (L.nerf_loss if live is None else L.nerf_loss_routed)(*head, *seeds)
    terms = {"rgb": out[0] / (3 * B), "opacity": out[1] / B}
    if lambda_distortion > 0 and dist_k is not None:
        terms["distortion"] = lambda_distortion * dist_k.sum() / B
    if lambda_cv_importance > 0 and K > 1:
        terms["cv_importance"] = out[2]
    if lambda_depth_mutual > 0 and K > 1:
        terms["depth_mutual"] = out[3] / (B * K)
    return terms, (d_rgb, d_op, d_depth, d_gate)
