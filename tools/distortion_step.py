"""Whole-step cost of the distortion loss on the fused chain (dev tool, GPU):
fwd+bwd steps with no per-launch events, three forms interleaved round by
round in one process (as tools/step_variants.py), a device synchronise around
the timed steps; one JSON line per shape with the median ms per step.

  default   the default step (no distortion loss);
  inchain   forward(distortion=True) + backward(dL_ddist): the loss and its
            gradient inside the composite kernels (rn_ml_composite_dist_fw/_bw);
  explicit  the default step's forward, then rn_distortion_loss_fw/_bw over the
            workspace's samples (ws_incl, wts_incl and dL_dws arrays of one
            float per sample slot) and rn_composite_train_bw with that dL_dws
            in place of the fused composite backward.

Shapes: C3 (K = 2, 8192 rays, scale 0.5) and C5's per-GPU shape (K = 8, 8192
rays, scale 16, exp step 1/256).

usage: python tools/distortion_step.py [c3] [c5]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd._lib import lib  # noqa: E402
from radnerf_amd.fused import FusedMLRenderer  # noqa: E402
from steptime import interleaved_ms  # noqa: E402

SHAPES = {"c3": (2, 8192, 0.5), "c5": (8, 8192, 16.0)}
LAMBDA = 1e-3       # --distortion_loss_w of the reference's 360 scripts


class Explicit:
    """The composed form on the renderer's workspace: the combine's seeds
    folded per segment with torch ops, the three sample-sized arrays, and the
    drop-in kernels over rays_a rows built from counts / offsets."""

    def __init__(self, r):
        w = r.ws
        f = dict(device=w.device, dtype=torch.float32)
        self.r = r
        self.ws_incl = torch.empty(w.capacity, **f)
        self.wts_incl = torch.empty(w.capacity, **f)
        self.dL_dws = torch.empty(w.capacity, **f)
        self.loss = torch.empty(w.K * w.B, **f)
        self.seed = torch.full((w.K * w.B,), LAMBDA / w.B, **f)
        self.rows = torch.empty(w.K * w.B, 3, device=w.device, dtype=torch.int64)
        self.rows[:, 0] = torch.arange(w.K * w.B, device=w.device)

    def composite_bw(self, gate, bg, d_rgb, d_op, d_depth, st):
        r, w, L = self.r, self.r.ws, lib()
        n = w.K * w.B
        self.rows[:, 1] = w.offsets.view(-1)
        self.rows[:, 2] = w.counts.view(-1)
        L.distortion_loss_fw(w.ws.data_ptr(), w.deltas.data_ptr(), w.ts.data_ptr(),
                             self.rows.data_ptr(), n, self.loss.data_ptr(),
                             self.ws_incl.data_ptr(), self.wts_incl.data_ptr(), st)
        L.distortion_loss_bw(self.seed.data_ptr(), self.ws_incl.data_ptr(),
                             self.wts_incl.data_ptr(), w.ws.data_ptr(), w.deltas.data_ptr(),
                             w.ts.data_ptr(), self.rows.data_ptr(), n, self.dL_dws.data_ptr(), st)
        gt = gate.t()                                               # [K][B]
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
    K, B, scale = SHAPES[name]
    dev = torch.device("cuda")
    sc = S.bench_scene(K, B, scale, dev)
    m, g, o, d, nz, sd, bg, esf = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bg, sc.esf
    r = FusedMLRenderer(m, g, B)
    ex = Explicit(r)
    gg, mg, ag = sc.grid_grad, sc.mlp_grad, sc.gate_grad
    L = lib()
    plain_bw = L.ml_composite_bw

    def default():
        _, _, _, gt, _ = r.forward(o, d, d, nz, bg, 1e-4, esf)
        r.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag)

    def inchain():
        _, _, _, gt, _ = r.forward(o, d, d, nz, bg, 1e-4, esf, distortion=True)
        r.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag, dL_ddist=LAMBDA / B)

    def explicit():
        # the renderer's own backward with its composite launch replaced
        _, _, _, gt, _ = r.forward(o, d, d, nz, bg, 1e-4, esf)
        st = torch.cuda.current_stream(dev).cuda_stream
        L.ml_composite_bw = lambda *a: ex.composite_bw(gt, bg, *sd, st)
        try:
            r.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag)
        finally:
            L.ml_composite_bw = plain_bw

    forms = {"default": default, "inchain": inchain, "explicit": explicit}
    times = interleaved_ms(forms, steps, rounds)
    out = {"shape": name, "K": K, "rays": B, "scale": scale, "samples": r.ws.n_samples(),
           "steps": steps, "rounds": rounds - 1, "lambda": LAMBDA,
           "extra_bytes_explicit": 3 * 4 * r.ws.capacity}
    for k, t in times.items():
        out[k + "_ms"], out[k + "_spread_ms"] = t["ms"], t["range_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    for name in sys.argv[1:] or ["c3", "c5"]:
        run(name)
        torch.cuda.empty_cache()
