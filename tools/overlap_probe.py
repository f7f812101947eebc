"""Can the field forward of one half-batch overlap the field backward of the
other?  (dev tool, GPU)  Two FusedMLRenderers of B/2 rays each; schedules:
  seq : fwd(A) fwd(B) bwd(A) bwd(B) on one stream
  ovl : fwd(A); [stream 2: fwd(B)] || [stream 1: bwd(A) with `blocks` merged
        blocks]; bwd(B) after both
prints median ms per full-batch step for each `blocks` value."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radnerf_amd import synthetic as S  # noqa: E402
from radnerf_amd.fused import FusedMLRenderer  # noqa: E402


def main():
    dev = torch.device("cuda")
    B, K = 8192, 2
    sc = S.bench_scene(K, B, 0.5, dev)
    m, g, o, d, nz, sd, bg = sc.m, sc.g, sc.o, sc.d, sc.noise, sc.seeds, sc.bg
    h = B // 2
    halves = [(o[:h].contiguous(), d[:h].contiguous(), nz[:, :h].contiguous(), [x[:h].contiguous() for x in sd]),
              (o[h:].contiguous(), d[h:].contiguous(), nz[:, h:].contiguous(), [x[h:].contiguous() for x in sd])]
    rs = [FusedMLRenderer(m, g, h), FusedMLRenderer(m, g, h)]
    full = FusedMLRenderer(m, g, B)
    gg, mg, ag = sc.grid_grad, sc.mlp_grad, sc.gate_grad
    s1 = torch.cuda.current_stream()
    s2 = torch.cuda.Stream()

    def fwd(i):
        oo, dd, n_, _ = halves[i]
        return rs[i].forward(oo, dd, dd, n_, bg)[3]

    def bwd(i, gt):
        oo, dd, _, ss = halves[i]
        rs[i].backward(oo, dd, dd, gt, bg, *ss, None, 1e-4, gg, mg, ag)

    def one():
        gt = full.forward(o, d, d, nz, bg)[3]
        full.backward(o, d, d, gt, bg, *sd, None, 1e-4, gg, mg, ag)

    def seq():
        ga = fwd(0); gb = fwd(1); bwd(0, ga); bwd(1, gb)

    def ovl():
        ga = fwd(0)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            gb = fwd(1)
        bwd(0, ga)
        s1.wait_stream(s2)
        bwd(1, gb)

    variants = {"full": one, "seq": seq}
    for blocks in (256, 224, 192, 160):
        def f(blocks=blocks):
            rs[0].merged_blocks = blocks
            ovl()
            rs[0].merged_blocks = 256
        variants[f"ovl{blocks}"] = f
    times = {k: [] for k in variants}
    for rnd in range(6):
        for k, fn in variants.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            if rnd:
                times[k].append((time.perf_counter() - t0) / 10 * 1e3)
    print(json.dumps({k: round(float(np.median(v)), 4) for k, v in times.items()}))


if __name__ == "__main__":
    main()
