"""GPU: the validation kernels of csrc/metrics.hip against fp64 / torch
restatements (tests/metrics_ref.py).

  rn_image_sse        PSNR within 1e-4 dB of fp64 (the fp32 block sums carry a
                      relative error of about 1e-6, i.e. 4e-6 dB); inf on equal
                      inputs; two calls give the same bits;
  rn_ssim             mean within 1e-4 and every pixel of ssim_map within 1e-3
                      of fp64 (about five times what a plain fp32 restatement
                      of the formula differs by); exactly 1.0 on pred is
                      target; H = 10 raises; bitwise repeatable; C = 1 and 3.
                      The kernel's tile is 32 x 32 valid outputs: 12 x 43 and
                      77 x 59 leave remainders in both directions over
                      several tiles;
  rn_ml_combine_test  against the torch composition of rendering.ml_render's
                      loop within 2e-6 (K fp32 multiply-adds on values in
                      [0, 1]), written at ray0 of a larger buffer whose other
                      rows stay untouched.
"""
import pytest
import torch

import metrics_ref as MR
from radnerf_amd import metrics
from radnerf_amd._lib import lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_rays", [1, 255, 256, 257, 33335])
def test_psnr_vs_fp64(cuda, n_rays):
    g = torch.Generator().manual_seed(n_rays)
    pred, tgt = torch.rand(n_rays, 3, generator=g), torch.rand(n_rays, 3, generator=g)
    got = metrics.psnr(pred.to(cuda), tgt.to(cuda))
    assert got.device.type == "cuda" and got.ndim == 0
    ref = MR.psnr_ref(pred, tgt)
    print(f"psnr n={n_rays}: {float(got):.7f} vs fp64 {ref:.7f} ({abs(float(got) - ref):.2e} dB)")
    assert abs(float(got) - ref) <= 1e-4
    # a close pair (a high PSNR, small differences)
    near = (tgt + 1e-3 * (pred - 0.5)).contiguous()
    got, ref = float(metrics.psnr(near.to(cuda), tgt.to(cuda))), MR.psnr_ref(near, tgt)
    print(f"psnr n={n_rays} near: {got:.7f} vs {ref:.7f}")
    assert abs(got - ref) <= 1e-4


def test_psnr_identical_and_repeatable(cuda):
    a = torch.rand(4097, 3, device=cuda)
    b = torch.rand(4097, 3, device=cuda)
    assert float(metrics.psnr(a, a)) == float("inf")
    assert float(metrics.psnr(a, a.clone())) == float("inf")
    s1, s2 = metrics.sse(a, b), metrics.sse(a, b)
    assert torch.equal(s1, s2) and s1.dtype == torch.float64
    assert torch.equal(metrics.psnr(a, b), metrics.psnr(a, b))
    # no elements: sse 0
    e = torch.empty(0, 3, device=cuda)
    assert float(metrics.sse(e, e)) == 0.0


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw", [(11, 11), (12, 43), (77, 59)])
@pytest.mark.parametrize("kind", ["noise", "ramp", "flat"])
def test_ssim_vs_fp64(cuda, kind, hw, C):
    H, W = hw
    pred, tgt = MR.images(kind, (W, H), C, seed=H * W + C)
    score, smap = metrics.ssim(pred.to(cuda), tgt.to(cuda), (W, H), return_map=True)
    ref, ref_map = MR.ssim_ref(pred, tgt, (W, H))
    assert smap.shape == (H - 10, W - 10, C) and smap.dtype == torch.float32
    e_mean = abs(float(score) - ref)
    e_pix = float((smap.double().cpu() - ref_map).abs().max())
    print(f"ssim {kind} {H}x{W} C={C}: {float(score):.6f} vs fp64 {ref:.6f}: mean {e_mean:.2e}, "
          f"per pixel {e_pix:.2e}")
    assert e_mean <= 1e-4 and e_pix <= 1e-3
    # the score is the mean of the map, and the map is optional
    assert abs(float(smap.double().mean()) - float(score)) <= 1e-6
    assert torch.equal(metrics.ssim(pred.to(cuda), tgt.to(cuda), (W, H)), score)


@pytest.mark.parametrize("C", [1, 3])
def test_ssim_identical_is_exactly_one(cuda, C):
    for kind in ("noise", "ramp", "flat"):
        a = MR.images(kind, (59, 77), C)[0].to(cuda)
        score, smap = metrics.ssim(a, a, (59, 77), return_map=True)
        assert float(score) == 1.0 and bool((smap == 1.0).all()), kind


def test_ssim_repeatable_and_small_image_raises(cuda):
    pred, tgt = (t.to(cuda) for t in MR.images("noise", (59, 77), 3))
    s1, m1 = metrics.ssim(pred, tgt, (59, 77), return_map=True)
    s2, m2 = metrics.ssim(pred, tgt, (59, 77), return_map=True)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    a = torch.rand(10 * 20, 3, device=cuda)
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim(a, a, (20, 10))                              # H = 10
    # the library's own check (a caller of the C ABI): a status and a message
    out = torch.zeros((), dtype=torch.float64, device=cuda)
    work = torch.empty(1024, dtype=torch.float64, device=cuda)
    with pytest.raises(RuntimeError, match="rn_ssim.*at least 11"):
        lib().ssim(a.data_ptr(), a.data_ptr(), 10, 20, 3, work.data_ptr(), out.data_ptr(), None,
                   None)


def _combine_ref(gate, op_k, depth_k, rgb_k, bg):
    """rendering.ml_render's loop (ml_rendering.py:65-68) and the gated depth
    of train_ml.py:243, in torch."""
    K, B = op_k.shape
    rgb = torch.zeros(B, 3, device=op_k.device)
    op = torch.zeros(B, device=op_k.device)
    depth_all = torch.zeros(B, K, device=op_k.device)
    for i in range(K):
        r = rgb_k[i] + bg * (1 - op_k[i])[:, None]
        rgb = rgb + r * gate[:, i][:, None]
        depth_all[:, i] = depth_k[i]
        op = op + op_k[i] * gate[:, i]
    return rgb, op, (gate * depth_all).sum(1), depth_all


@pytest.mark.parametrize("B", [1, 63, 257])
@pytest.mark.parametrize("K", [1, 2, 4, 9, 16])
def test_ml_combine_test_vs_torch(cuda, K, B):
    g = torch.Generator().manual_seed(100 * K + B)
    gate = torch.softmax(torch.randn(B, K, generator=g), 1).to(cuda).contiguous()
    op_k = torch.rand(K, B, generator=g).to(cuda)
    depth_k = torch.rand(K, B, generator=g).to(cuda)
    rgb_k = (torch.rand(K, B, 3, generator=g).to(cuda) * op_k[:, :, None]).contiguous()
    st = torch.cuda.current_stream(cuda).cuda_stream
    for ray0 in (0, 5):
        for bg in (torch.ones(3, device=cuda), torch.zeros(3, device=cuda)):
            N = B + 12
            bufs = [torch.full(s, -7.0, device=cuda) for s in ((N, 3), (N,), (N,), (N, K))]
            lib().ml_combine_test(gate.data_ptr(), op_k.data_ptr(), depth_k.data_ptr(),
                                  rgb_k.data_ptr(), bg.data_ptr(), B, K, ray0,
                                  *[b.data_ptr() for b in bufs], st)
            want = _combine_ref(gate, op_k, depth_k, rgb_k, bg)
            keep = torch.ones(N, dtype=torch.bool, device=cuda)
            keep[ray0:ray0 + B] = False
            for name, got, ref in zip(("rgb", "opacity", "depth", "depth_k"), bufs, want):
                err = float((got[ray0:ray0 + B] - ref).abs().max())
                assert err <= 2e-6, (name, ray0, err)
                assert bool((got[keep] == -7.0).all()), (name, ray0)
    # depth_k_out is optional, and a NULL gate is a gate of exactly 1 (K = 1)
    bufs = [torch.full(s, -7.0, device=cuda) for s in ((B, 3), (B,), (B,))]
    bg = torch.ones(3, device=cuda)
    lib().ml_combine_test(gate.data_ptr(), op_k.data_ptr(), depth_k.data_ptr(), rgb_k.data_ptr(),
                          bg.data_ptr(), B, K, 0, *[b.data_ptr() for b in bufs], None, st)
    assert float((bufs[0] - _combine_ref(gate, op_k, depth_k, rgb_k, bg)[0]).abs().max()) <= 2e-6
    if K == 1:
        lib().ml_combine_test(None, op_k.data_ptr(), depth_k.data_ptr(), rgb_k.data_ptr(),
                              bg.data_ptr(), B, K, 0, *[b.data_ptr() for b in bufs], None, st)
        ref = _combine_ref(torch.ones(B, 1, device=cuda), op_k, depth_k, rgb_k, bg)
        for got, want in zip(bufs, ref):
            assert float((got - want).abs().max()) <= 2e-6
    else:
        with pytest.raises(RuntimeError, match="rn_ml_combine_test.*gate"):
            lib().ml_combine_test(None, op_k.data_ptr(), depth_k.data_ptr(), rgb_k.data_ptr(),
                                  bg.data_ptr(), B, K, 0, *[b.data_ptr() for b in bufs], None, st)
