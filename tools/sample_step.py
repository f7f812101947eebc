"""Cost of producing a training step's inputs (dev tool, GPU): whole Trainer
steps at C3 (K = 2, 8192 rays, scale 0.5) on 100 uint8 800 x 800 images
generated from a seed, three ways of feeding them, interleaved in one process
after a warm-up past the occupancy grid's own (256 steps), `steps` steps per
leg between two device events, the round of three repeated in rotating order;
one JSON line per mode (fixed poses, optimize_ext) with each repeat's and the
median ms per step, and the host's time to issue a step (`*_host_issue_ms`: a
leg whose issue time reaches its step time is bound by the host, not the GPU).

  sampled  Trainer.step_sampled: rn_sample_batch (picks, targets, rays,
           jitter, background in one launch) then the step;
  torch    Trainer.step_pixels fed by torch ops on the device: torch.randint
           twice, images[img, pix].float() / 255, torch.rand(K, B);
  host     Trainer.step_pixels fed as the reference's loader feeds it
           (datasets/base.py:23-31): np.random.choice twice on the host, a
           gather from the fp32 images in host memory, a pinned buffer and an
           asynchronous copy to the device.

The three legs feed one trainer in turn, so every leg steps the same model
in the same state (the step's cost follows the sample count, which drifts as
the model trains: it is reported before and after the timed rounds).  Then
the input producers alone (20 back-to-back calls between two events, us per
call).

usage: python tools/sample_step.py [--out FILE] [--steps N] [--images N] [--res N]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rad-nerf_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pose_step import kernel_us  # noqa: E402
from radnerf_amd.networks import MNGP, Ray_Gate  # noqa: E402
from radnerf_amd.sampler import TrainImages, sample_batch  # noqa: E402
from radnerf_amd.synthetic import ring_cameras  # noqa: E402
from radnerf_amd.trainer import Trainer  # noqa: E402

K, B, SCALE = 2, 8192, 0.5


def make_images(n_img, res, seed=0):
    """(n_img, res * res, 3) uint8: a smooth seeded pattern per image (low
    frequency sines with seeded phases) plus seeded byte noise"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.linspace(0, 1, res)
    y, x = torch.meshgrid(u, u, indexing="ij")
    out = torch.empty(n_img, res * res, 3, dtype=torch.uint8)
    for i in range(n_img):
        ph = torch.rand(3, 3, generator=gen) * 6.283
        im = torch.stack([0.5 + 0.4 * torch.sin(6.283 * (x * (c + 1) + y) + ph[c, 0])
                          * torch.cos(6.283 * y * (i % 3 + 1) + ph[c, 1]) for c in range(3)], -1)
        noise = torch.randint(0, 16, (res, res, 3), generator=gen)
        out[i] = (im * 255).long().add_(noise).clamp_(0, 255).to(torch.uint8).view(-1, 3)
    return out


def run(optimize_ext, u8_host, f32_host, dirs, poses, steps=200, repeats=3, warmup=300):
    dev = torch.device("cuda")
    n_img, n_pix = u8_host.shape[0], u8_host.shape[1]
    u8 = u8_host.to(dev)
    ti = TrainImages(u8)
    host_np = f32_host.numpy()
    pinned = torch.empty(B, 3).pin_memory()
    pin_i, pin_p = torch.empty(B, dtype=torch.int64).pin_memory(), \
        torch.empty(B, dtype=torch.int64).pin_memory()
    rng = np.random.RandomState(0)

    m, g = MNGP(SCALE, size=K, seed=3).to(dev), Ray_Gate(K, seed=4).to(dev)
    tr = Trainer(m, g, B, lr=1e-2, lambda_cv_importance=1e-2, directions=dirs, poses=poses,
                 images=ti, optimize_ext=optimize_ext, seed=1)

    def sampled():
        tr.step_sampled()

    def composed():
        img = torch.randint(n_img, (B,), device=dev)
        pix = torch.randint(n_pix, (B,), device=dev)
        tgt = u8[img, pix].float() / 255
        tr.step_pixels(img, pix, tgt, noise=torch.rand(K, B, device=dev))

    def host():
        img, pix = rng.choice(n_img, B), rng.choice(n_pix, B)
        pinned.copy_(torch.from_numpy(host_np[img, pix]))
        pin_i.copy_(torch.from_numpy(img))
        pin_p.copy_(torch.from_numpy(pix))
        tr.step_pixels(pin_i.to(dev, non_blocking=True), pin_p.to(dev, non_blocking=True),
                       pinned.to(dev, non_blocking=True))

    legs = {"sampled": sampled, "torch": composed, "host": host}
    for _ in range(warmup // 3):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    samples = [tr.renderer.ws.n_samples()]
    times, issue = {k: [] for k in legs}, {k: [] for k in legs}
    names = list(legs)
    for rep in range(repeats):
        # the order rotates from round to round, so no leg always follows the same one
        for k in names[rep % 3:] + names[:rep % 3]:
            fn = legs[k]
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            # the host's share: how long issuing the steps took, before waiting
            issue[k].append((time.perf_counter() - t0) / steps * 1e3)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    out = {"shape": "c3", "K": K, "rays": B, "scale": SCALE, "images": n_img,
           "pixels_per_image": n_pix, "image_bytes_uint8": u8.numel(),
           "image_bytes_fp32": 4 * u8.numel(), "optimize_ext": optimize_ext, "steps": steps,
           "repeats": repeats, "warmup": warmup,
           "samples_before_after": samples + [tr.renderer.ws.n_samples()]}
    for k, t in times.items():
        out[k + "_ms"] = round(float(np.median(t)), 4)
        out[k + "_repeats_ms"] = [round(float(v), 4) for v in t]
        out[k + "_host_issue_ms"] = round(float(np.median(issue[k])), 4)
    out["sampled_over_torch"] = round(out["sampled_ms"] / out["torch_ms"], 4)
    out["sampled_over_host"] = round(out["sampled_ms"] / out["host_ms"], 4)
    # the producers alone
    buf = tr.last_batch
    kw = dict(dR=tr.dR.detach(), dT=tr.dT.detach()) if optimize_ext else {}

    def torch_inputs():
        img = torch.randint(n_img, (B,), device=dev)
        pix = torch.randint(n_pix, (B,), device=dev)
        return u8[img, pix].float() / 255, torch.rand(K, B, device=dev)

    out["producers_us"] = {
        "sample_batch": kernel_us(lambda: sample_batch(ti, dirs, poses, B, K, 1, 7, out=buf, **kw)),
        "torch_inputs_without_rays": kernel_us(torch_inputs)}
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    path = argv[argv.index("--out") + 1] if "--out" in argv else \
        os.path.join(ROOT, "profiles", "sampler", "sample_step.jsonl")
    n_img, res, steps = opt("--images", 100), opt("--res", 800), opt("--steps", 200)
    u8 = make_images(n_img, res)
    f32 = u8.float() / 255
    dirs, poses = (t.to("cuda") for t in ring_cameras(n_img, res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for ext in (False, True):
        line = json.dumps(run(ext, u8, f32, dirs, poses, steps=steps))
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")
