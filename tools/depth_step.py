"""Whole-step cost of depth supervision's ray-termination term on the fused
chain (dev tool, GPU; DESIGN.md §4 "Depth supervision"): fwd+bwd steps with no
per-launch events, three forms interleaved round by round in one process
(tools/steptime.py), a device synchronise around the timed steps; one JSON
line per shape appended to profiles/depth/depth_step.jsonl.

  default   the default step (no depth term);
  inchain   forward(depth_target=) + backward(dL_ddvar=): the second moment and
            its gradient inside the composite kernels
            (rn_ml_composite_depth_fw / _bw);
  composed  the default step's forward, then V and dL_dws from torch ops on the
            workspace's ws / ts (a gather of the ray's target per sample slot,
            the clipped square, a segment sum; three sample-sized arrays) and
            rn_composite_train_bw with that dL_dws in place of the fused
            composite backward.

Shapes: C3 (K = 2, 8192 rays, scale 0.5) and C5's per-GPU shape (K = 8, 8192
rays, scale 16, exp step 1/256).  Targets: the scene's own expected depth,
a third of the rays without one.

usage: python tools/depth_step.py [c3] [c5] [--out DIR]
       python tools/depth_step.py --ab PARENT_TREE [--ab-out FILE] [--ab-rounds N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from steptime import ab_main, append_jsonl, interleaved_ms  # noqa: E402

SHAPES = {"c3": (2, 8192, 0.5), "c5": (8, 8192, 16.0)}
LAMBDA = 0.1
CLIP = {0.5: 0.5, 16.0: 4.0}


class Composed:
    """The composed form on the renderer's workspace: per sample slot the
    ray's target, phi and dL_dws = seed phi from torch ops, V as a segment
    sum, and the drop-in backward over rays_a rows built from counts / offsets.
    The torch ops run over the slots up to the last sub-NeRF's last sample
    (n_slots, read back once before the timing: the timed steps repeat one
    batch), not over the workspace's worst-case capacity."""

    def __init__(self, r, z, clip, n_slots):
        w = r.ws
        self.r, self.z, self.clip2, self.n_slots = r, z, clip * clip, n_slots
        self.rows = torch.empty(w.K * w.B, 3, device=w.device, dtype=torch.int64)
        self.rows[:, 0] = torch.arange(w.K * w.B, device=w.device)
        self.idx = torch.arange(n_slots, device=w.device)
        self.dL_dws = torch.zeros(w.capacity, device=w.device)
        self.V = None

    def composite_bw(self, gate, bg, d_rgb, d_op, d_depth, st):
        from radnerf_amd._lib import lib
        r, w, L = self.r, self.r.ws, lib()
        n, B, ns = w.K * w.B, w.B, self.n_slots
        self.rows[:, 1] = w.offsets.view(-1)
        self.rows[:, 2] = w.counts.view(-1)
        # sub-NeRF k's samples lie in [seg_base[k], seg_base[k] + seg_count[k]);
        # the alignment gaps between them are never written
        base = w.seg_base.long()
        k_of = torch.bucketize(self.idx, base, right=True) - 1
        inside = self.idx < (base + w.seg_count.long())[k_of]
        ray = w.ray_of[:ns].long().clamp_(0, B - 1)
        zs = self.z[ray]
        phi = ((w.ts[:ns] - zs) ** 2).clamp_(max=self.clip2)
        phi = torch.where(inside & (zs > 0), phi, torch.zeros_like(phi))
        seg = k_of * B + ray
        gt = gate.t().contiguous()                                 # [K][B]
        wphi = torch.where(inside, w.ws[:ns] * phi, torch.zeros_like(phi))
        self.V = torch.zeros(n, device=w.device).index_add_(0, seg, wphi)
        seed = (LAMBDA / B) * gt.view(-1)
        self.dL_dws[:ns] = seed[seg] * phi
        s_rgb = (gt[:, :, None] * d_rgb[None]).contiguous().view(-1, 3)
        s_op = (gt * (d_op - d_rgb @ bg)[None]).contiguous().view(-1)
        s_de = d_depth.t().contiguous().view(-1)
        L.composite_train_bw(s_op.data_ptr(), s_de.data_ptr(), s_rgb.data_ptr(),
                             self.dL_dws.data_ptr(), w.sigma.data_ptr(), w.rgb.data_ptr(),
                             w.ws.data_ptr(), w.deltas.data_ptr(), w.ts.data_ptr(),
                             self.rows.data_ptr(), n, w.opacity_k.data_ptr(),
                             w.depth_k.data_ptr(), w.rgb_k.data_ptr(), 1e-4,
                             w.dsigma.data_ptr(), w.drgb.data_ptr(), st)


def run(name, steps=10, rounds=6):
    from radnerf_amd import synthetic as S
    from radnerf_amd._lib import lib
    from radnerf_amd.fused import FusedMLRenderer
    K, B, scale = SHAPES[name]
    dev = torch.device("cuda")
    sc = S.bench_scene(K, B, scale, dev)
    m, g, o, d, nz, sd, bg, esf = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bg, sc.esf
    r = FusedMLRenderer(m, g, B)
    gg, mg, ag = sc.grid_grad, sc.mlp_grad, sc.gate_grad
    L = lib()
    plain_bw = L.ml_composite_bw
    _, _, depth, gate0, _ = r.forward(o, d, d, nz, bg, 1e-4, esf)
    z = (gate0 * depth).sum(1)
    z = torch.where(z > 0.02, z, torch.full_like(z, 0.5))
    z[::3] = 0.0
    z = z.contiguous()
    clip = CLIP[scale]
    n_slots = int(r.ws.seg_base[-1]) + int(r.ws.seg_count[-1])
    ex = Composed(r, z, clip, n_slots)

    def default():
        _, _, _, gt, _ = r.forward(o, d, d, nz, bg, 1e-4, esf)
        r.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag)

    def inchain():
        _, _, _, gt, _ = r.forward(o, d, d, nz, bg, 1e-4, esf, depth_target=z, depth_clip=clip)
        seed = ((LAMBDA / B) * (z > 0))[None] * gt.t()
        r.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag, dL_ddvar=seed.contiguous())

    def composed():
        # the renderer's own backward with its composite launch replaced
        _, _, _, gt, _ = r.forward(o, d, d, nz, bg, 1e-4, esf)
        st = torch.cuda.current_stream(dev).cuda_stream
        L.ml_composite_bw = lambda *a: ex.composite_bw(gt, bg, *sd, st)
        try:
            r.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag)
        finally:
            L.ml_composite_bw = plain_bw

    # the two forms compute the same thing: V and dsigma agree before they are timed
    inchain()
    v_in, ds_in = r.ws.dvar_k.clone().view(-1), r.ws.dsigma.clone()
    composed()
    n = r.ws.n_samples()
    inside = torch.zeros_like(ds_in, dtype=torch.bool)
    for b, c in zip(r.ws.seg_base.tolist(), r.ws.seg_count.tolist()):
        inside[b:b + c] = True
    v_err = float((v_in - ex.V).abs().max() / ex.V.abs().max().clamp_min(1e-30))
    ds_err = float((ds_in[inside] - r.ws.dsigma[inside]).abs().max()
                   / ds_in[inside].abs().max().clamp_min(1e-30))
    forms = {"default": default, "inchain": inchain, "composed": composed}
    times = interleaved_ms(forms, steps, rounds)
    out = {"shape": name, "K": K, "rays": B, "scale": scale, "samples": n, "steps": steps,
           "rounds": rounds - 1, "lambda": LAMBDA, "clip": clip,
           "valid_share": round(float((z > 0).float().mean()), 4),
           "inchain_vs_composed": {"dvar_rel": v_err, "dsigma_rel": ds_err},
           "slots": n_slots}
    for k, t in times.items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    dest = os.path.join(ROOT, "profiles", "depth")
    if "--ab" in args:
        ab_main(args, os.path.join(dest, "ab_default.txt"))
        sys.exit(0)
    if "--out" in args:
        i = args.index("--out")
        dest = args[i + 1]
        del args[i:i + 2]
    for name in args or ["c3", "c5"]:
        append_jsonl(os.path.join(dest, "depth_step.jsonl"), run(name))
        torch.cuda.empty_cache()
