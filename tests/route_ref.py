"""Routed training restated (test infrastructure, CPU only).

routed_train_step    one routed step built from the oracle's building blocks
                     (oracle.ml_march, field_oracle.field_forward /
                     gate_forward, oracle.composite_train_fw / _bw) the way
                     ml_oracle.ml_train_step builds the dense one: given a
                     `live` mask (B, K), a dead pair's sample count is zeroed
                     and its samples dropped, the render is combined with
                     gate_used, and the gradient flows back through the masked
                     (optionally renormalised) gate -- that step in fp64, the
                     selection held constant.
select_bw_ref        rn_gate_select_bw in numpy fp32, operation for operation.
depth_mutual_ref     the routed depth-mutual term and its seed in numpy fp32,
                     operation for operation (rn_nerf_loss_routed).
"""
import numpy as np
import torch

import oracle
from oracle import field_oracle as fo
from oracle.ml_oracle import MAX_SAMPLES, NEAR_DISTANCE, _split_field, _split_gate


def routed_train_step(rays_o, rays_d, bitfields, noise, grid_master, mlp_master, gate_master,
                      scale, live, renormalize=False, seeds=None, bg=None, T_threshold=1e-4,
                      log2_T=19, grid_size=128, input_grads=False, dgate_ext=None,
                      dist_seed=None):
    """ml_oracle.ml_train_step's arguments and result keys, plus live (B, K)
    (non-zero: the pair is marched).  Adds "gate_used", and with seeds "dgate"
    (B, K): dL/d softmax gate through gate_used (dead pairs exactly 0), before
    dgate_ext (a seed on the softmax gate itself, e.g. the cv^2 term's) is
    added.  Samples are per sub-NeRF: "ts" / "deltas" / "xyzs" are lists of K
    arrays (live rays in ray order), "starts" (K, B) indexes into them.
    "distortion" (B, K) is each segment's Mip-NeRF 360 distortion loss
    (oracle.distortion_loss_fw on its ws / deltas / ts; 0 for a dead pair);
    dist_seed (a number, or (B, K)) is dL/d of it, back-propagated through
    oracle.distortion_loss_bw into the composite backward's dL_dws."""
    K, B = bitfields.shape[0], len(rays_o)
    live = np.asarray(live).astype(bool)
    assert live.shape == (B, K)
    cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)
    esf = 1.0 / 256 if scale > 0.5 else 0.0
    if bg is None:
        bg = np.ones(3, np.float32) if esf == 0 else np.zeros(3, np.float32)
    lv = fo.grid_levels(scale, log2_T)
    xyz_min = torch.full((1, 3), -float(scale))
    xyz_max = torch.full((1, 3), float(scale))
    center, half = np.zeros(3, np.float32), np.full(3, scale, np.float32)

    o_t = torch.from_numpy(np.asarray(rays_o, np.float32).copy()).requires_grad_(input_grads)
    d_t = torch.from_numpy(np.asarray(rays_d, np.float32).copy()).requires_grad_(input_grads)
    grid_p = torch.tensor(np.asarray(grid_master, np.float32)).half().float().requires_grad_(True)
    mlp_p = torch.tensor(np.asarray(mlp_master, np.float32)).requires_grad_(True)
    gate_p = torch.tensor(np.asarray(gate_master, np.float32)).requires_grad_(True)
    gate = fo.gate_forward(torch.cat([o_t, d_t], 1), _split_gate(gate_p, K))

    # the dense march, then the dead pairs' counts zeroed and their samples dropped
    c0, s0, x0, t0, dl0, _ = oracle.ml_march(rays_o, rays_d, center, half, noise, bitfields,
                                             cascades, scale, esf, grid_size, MAX_SAMPLES,
                                             NEAR_DISTANCE)
    counts = np.where(live.T, c0, 0).astype(c0.dtype)
    starts = np.zeros_like(counts)
    xs, tss, dls, rays_of = [], [], [], []
    for k in range(K):
        starts[k] = np.concatenate([[0], np.cumsum(counts[k])[:-1]])
        keep = np.concatenate([np.arange(s0[k, r], s0[k, r] + counts[k, r]) for r in range(B)]
                              + [np.zeros(0, np.int64)]).astype(np.int64)
        xs.append(x0[keep]); tss.append(t0[keep]); dls.append(dl0[keep])
        rays_of.append(np.repeat(np.arange(B), counts[k]))
    res = {"counts": counts, "starts": starts, "xyzs": xs, "ts": tss, "deltas": dls,
           "total": int(counts.sum()), "gate": gate.detach().numpy(), "ray_of": rays_of}

    sig_l, rgb_l, Ok, Dk, RGBk, ws_l, used_l, ra_l, x_l = [], [], [], [], [], [], [], [], []
    for k in range(K):
        x = torch.from_numpy(xs[k].copy()).requires_grad_(input_grads)
        d = d_t[torch.from_numpy(rays_of[k])]
        sigma, rgb = fo.field_forward(x, d, grid_p, _split_field(mlp_p[k]), lv, xyz_min, xyz_max)
        rays_a = np.stack([np.arange(B), starts[k], counts[k]], 1).astype(np.int64)
        total_k, O, D, RGB, ws = oracle.composite_train_fw(
            sigma.detach().numpy(), rgb.detach().numpy(), dls[k], tss[k], rays_a, T_threshold)
        sig_l.append(sigma); rgb_l.append(rgb); ra_l.append(rays_a); x_l.append(x)
        Ok.append(O); Dk.append(D); RGBk.append(RGB); ws_l.append(ws); used_l.append(total_k)
    dist_l = [oracle.distortion_loss_fw(ws_l[k], dls[k], tss[k], ra_l[k]) for k in range(K)]
    res["distortion"] = np.stack([d[0] for d in dist_l], 1)

    # gate_used in fp64 with the selection constant: mask . g (/ its row sum)
    mask = torch.from_numpy(live.astype(np.float64))
    used = mask * gate.double()
    if renormalize:
        used = used / used.sum(1, keepdim=True)
    O_t = torch.tensor(np.stack(Ok), requires_grad=True)        # (K, B)
    D_t = torch.tensor(np.stack(Dk), requires_grad=True)
    C_t = torch.tensor(np.stack(RGBk), requires_grad=True)      # (K, B, 3)
    bg_t = torch.from_numpy(np.asarray(bg, np.float32))
    rgb_out, op_out = torch.zeros(B, 3, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    depth_out = torch.zeros(B, K)
    for k in range(K):
        rgb_k = C_t[k] + bg_t * (1 - O_t[k])[:, None]
        rgb_out = rgb_out + rgb_k.double() * used[:, k][:, None]
        op_out = op_out + O_t[k].double() * used[:, k]
        depth_out[:, k] = D_t[k]
    res.update({"rgb": rgb_out.detach().numpy().astype(np.float32),
                "opacity": op_out.detach().numpy().astype(np.float32),
                "depth": depth_out.detach().numpy(), "gate_used": used.detach().numpy(),
                "sigmas": [s.detach().numpy() for s in sig_l],
                "rgbs": [c.detach().numpy() for c in rgb_l], "opacity_k": np.stack(Ok),
                "depth_k": np.stack(Dk), "rgb_k": np.stack(RGBk), "ws": ws_l, "used": used_l})
    if seeds is None:
        return res

    g_rgb, g_op, g_depth = (torch.from_numpy(np.asarray(s, np.float32)) for s in seeds)
    gate.retain_grad()
    outs, gs = [rgb_out, op_out, depth_out], [g_rgb.double(), g_op.double(), g_depth]
    torch.autograd.backward(outs, gs, retain_graph=dgate_ext is not None)
    res["dgate"] = gate.grad.numpy().copy()
    if dgate_ext is not None:
        torch.autograd.backward([gate], [torch.from_numpy(np.asarray(dgate_ext, np.float32))])
    dsig_l, drgb_l = [], []
    g_dist = None if dist_seed is None else np.broadcast_to(
        np.asarray(dist_seed, np.float32), (B, K))
    for k in range(K):
        n_k = int(counts[k].sum())
        dws = np.zeros(n_k, np.float32)
        if g_dist is not None:
            _, wi, wti = dist_l[k]
            dws = oracle.distortion_loss_bw(np.ascontiguousarray(g_dist[:, k]), wi, wti, ws_l[k],
                                            dls[k], tss[k], ra_l[k])
        dsig, drgb = oracle.composite_train_bw(
            O_t.grad[k].numpy(), D_t.grad[k].numpy(), C_t.grad[k].numpy(),
            dws, sig_l[k].detach().numpy(), rgb_l[k].detach().numpy(),
            ws_l[k], dls[k], tss[k], ra_l[k], Ok[k], Dk[k], RGBk[k], T_threshold)
        dsig_l.append(dsig); drgb_l.append(drgb)
        if n_k:
            torch.autograd.backward([sig_l[k], rgb_l[k]],
                                    [torch.from_numpy(dsig), torch.from_numpy(drgb)])
    if input_grads:
        go = np.zeros((B, 3)) if o_t.grad is None else o_t.grad.numpy().astype(np.float64)
        gd = np.zeros((B, 3)) if d_t.grad is None else d_t.grad.numpy().astype(np.float64)
        dx_l = []
        for k in range(K):
            n_k = int(counts[k].sum())
            gx = (np.zeros((n_k, 3)) if x_l[k].grad is None
                  else x_l[k].grad.numpy().astype(np.float64))
            np.add.at(go, rays_of[k], gx)
            np.add.at(gd, rays_of[k], gx * tss[k][:, None].astype(np.float64))
            dx_l.append(gx)
        res.update({"drays_o": go, "drays_d": gd, "dxyzs": dx_l})
    zero = lambda p: p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    res.update({"dsigmas": dsig_l, "drgbs": drgb_l, "grid_grad": zero(grid_p),
                "mlp_grad": zero(mlp_p), "gate_grad": zero(gate_p)})
    return res


def select_bw_ref(gate, live, d_used, renormalize=False):
    """rn_gate_select_bw (include/radnerf.h) in fp32: dead 0; live d_i, or with
    renormalize (d_i - D) / S, S the live gates and D the rounded products
    d_j * (g_j / S) summed in index order from 0; a row with S == 0 gives 0."""
    f = np.float32
    g, d = np.ascontiguousarray(gate, f), np.ascontiguousarray(d_used, f)
    lv = np.asarray(live).astype(bool)
    n, K = g.shape
    if not renormalize:
        return np.where(lv, d, f(0)).astype(f)
    S, D = np.zeros(n, f), np.zeros(n, f)
    for i in range(K):
        S = np.where(lv[:, i], (S + g[:, i]).astype(f), S)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(K):
            u = (g[:, i] / S).astype(f)
            D = np.where(lv[:, i], (D + (d[:, i] * u).astype(f)).astype(f), D)
        out = ((d - D[:, None]).astype(f) / S[:, None]).astype(f)
    return np.where(lv & (S != 0)[:, None], out, f(0)).astype(f)


def depth_mutual_ref(depth, gate_used, live, lambda_dm):
    """The routed depth-mutual term (rn_nerf_loss_routed) in fp32, its
    operation order: per row mean_d = sum_k depth * gate_used (index order, from
    0); per live pair e = depth - mean_d, term lambda e e, seed (2 lambda /
    (B K)) e; dead pairs 0 and 0.  Returns (terms (B, K), d_depth (B, K))."""
    f = np.float32
    dep, gu = np.ascontiguousarray(depth, f), np.ascontiguousarray(gate_used, f)
    lv = np.asarray(live).astype(bool)
    B, K = dep.shape
    mean_d = np.zeros(B, f)
    for k in range(K):
        mean_d = (mean_d + (dep[:, k] * gu[:, k]).astype(f)).astype(f)
    lam = f(lambda_dm)
    s = (f(2.0) * lam / (f(B) * f(K))).astype(f)
    e = (dep - mean_d[:, None]).astype(f)
    terms = np.where(lv, ((lam * e).astype(f) * e).astype(f), f(0)).astype(f)
    return terms, np.where(lv, (s * e).astype(f), f(0)).astype(f)
