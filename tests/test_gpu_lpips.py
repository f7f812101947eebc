"""GPU: LPIPS (VGG) -- the kernels of csrc/lpips.hip one by one and the whole
distance (radnerf_amd/lpips.py) against the fp64 restatement
(tests/lpips_ref.py), then the wiring into validation.

Bounds (u = 2^-24, the unit roundoff of fp32; none of them is fitted):

  rn_lpips_prepare     bit-equal to the numpy fp32 restatement, op by op.

  rn_conv3x3_relu_f16  per output element, against the fp64 convolution of the
                       same f16 inputs and weights,
                         |out - ref| <= 2^-11 |ref| + 9 Cin u S + 2^-14,
                       S = sum |w x| over the element's 9 Cin products.  The
                       f16 products are exact in fp32 (11 x 11 significand
                       bits), so the accumulator differs from the exact sum by
                       the fp32 additions alone: at most (n - 1) u S for n =
                       9 Cin terms in any order (the bias addition's own u
                       (S + |b|) fits in the slack between n - 1 and n and in
                       the last term); ReLU does not increase a difference;
                       the one rounding to f16 adds 2^-11 |ref| for a normal
                       result, and a result below 2^-14 is a subnormal (or
                       flushed) within 2^-14 absolutely.

  rn_maxpool2_f16      torch.equal with torch's pool of the same values.

  rn_lpips_layer       per pixel, with e = (C / 2 + 4) u the relative error of
                       a normalised feature (C u for the sum of exact squares,
                       halved by the root plus its own u; two u for the
                       constant 1e-10 and its addition; one for the division):
                         e_c = e (|n0_c| + |n1_c|) + u |n0_c - n1_c|
                       bounds the error of the fp32 difference -- absolute in
                       |n0| + |n1|, since n0 - n1 may cancel -- and
                         B = sum_c w_c (2 |n0_c - n1_c| e_c + e_c^2)
                             + (C + 2) u sum_c w_c (|n0_c - n1_c| + e_c)^2
                       the error of d (the square, the product with w and the
                       C-term sum of non-negative terms).  The test allows
                       1.01 mean(B) (the second-order terms) on the mean.

  end to end           (a) against lpips_ref(round_f16=True): what is left is
                       isolated one-ulp f16 flips (the kernels round fp32
                       results where the restatement rounds doubles) and the
                       summation order.  Measured on an MI355X over the 27
                       cases below, the largest relative deviation is
                       MEASURED_REL (profiles/lpips/accuracy.json has every
                       value); the bar BOUND_F16_REL is 4 x that.
                       (b) against lpips_ref(round_f16=False): 2e-3 relative.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from radnerf_amd import lpips as LP
from radnerf_amd._lib import lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TILE_H, TILE_W = 8, 32                   # csrc/lpips.hip CV_TH, CV_TW
MEASURED_REL = 3.553e-5                  # profiles/lpips/accuracy.json max_rel_f16
BOUND_F16_REL = 4 * MEASURED_REL         # 1.42e-4
BOUND_FULL_REL = 2e-3


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 1. prepare -----------------------------------------------------------------
def test_prepare_bit_equal(cuda):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1001, 3, generator=g) * 2 - 0.5              # [-0.5, 1.5)
    x[:6] = torch.tensor([[0.0, 0.5, 1.0], [-3.0, 7.0, 0.25], [1.0, 1.0, 0.0],
                          [2.0 ** -25, 1 - 2.0 ** -24, 0.5 + 2.0 ** -24], [-0.0, 1e-30, 0.999],
                          [0.015, 0.044, 0.094]])
    out = torch.full((1001 * 3 + 16,), -7.0, dtype=torch.float16, device=cuda)
    lib().lpips_prepare(x.to(cuda).data_ptr(), 1001, out.data_ptr() + 16, _stream(cuda))
    f32 = np.float32
    v = f32(2) * x.numpy() - f32(1)
    v = np.minimum(np.maximum(v, f32(-1)), f32(1))
    want = ((v - np.array(R.SHIFT, dtype=f32)) / np.array(R.SCALE, dtype=f32)).astype(np.float16)
    assert v.dtype == f32
    got = out.cpu().numpy()
    assert (got[:8] == -7).all() and (got[-8:] == -7).all()
    assert np.array_equal(got[8:-8].reshape(1001, 3).view(np.uint16), want.view(np.uint16))


# ---- 2. convolution ---------------------------------------------------------------
PAIRS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]


def _conv_sizes(cin):
    last = (33, 35) if cin <= 128 else (9, 11)
    # one past the kernel's 8 x 32 tile in both dimensions
    return [(1, 1), (2, 3), (5, 7) if cin <= 128 else None, last, (TILE_H + 1, TILE_W + 1)]


CONV_CASES = [(ci, co, hw) for ci, co in PAIRS for hw in _conv_sizes(ci) if hw is not None]


@pytest.mark.parametrize("cin,cout,hw", CONV_CASES,
                         ids=[f"{ci}-{co}-{h}x{w}" for ci, co, (h, w) in CONV_CASES])
def test_conv_vs_fp64(cuda, cin, cout, hw):
    """The bound is derived in the module docstring."""
    H, W = hw
    g = torch.Generator().manual_seed(cin * 1000 + cout + H)
    x = torch.randn(2, H, W, cin, generator=g).to(torch.float16)          # two different images
    # the border rows and columns are where a wrong halo shows: no value is zero
    x = torch.where(x == 0, torch.ones_like(x), x)
    assert not torch.equal(x[0], x[1])
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(torch.float16)
    b = (torch.rand(cout, generator=g) - 0.5)
    guard = 2 * W * cout                                                   # two rows of sentinel
    n_out = 2 * H * W * cout
    out = torch.full((n_out + 2 * guard,), -7.0, dtype=torch.float16, device=cuda)
    frags = LP.pack_conv(w.float()).to(cuda)
    xd, bd = x.to(cuda), b.to(cuda)
    lib().conv3x3_relu_f16(xd.data_ptr(), frags.data_ptr(), bd.data_ptr(), 2, H, W, cin, cout,
                           out.data_ptr() + 2 * guard, _stream(cuda))
    got = out.cpu()
    assert bool((got[:guard] == -7).all()) and bool((got[-guard:] == -7).all())
    got = got[guard:-guard].double().reshape(2, H, W, cout)
    xn = x.double().permute(0, 3, 1, 2)
    ref = R.conv3x3_relu(xn, w.double(), b.double()).permute(0, 2, 3, 1)
    S = F.conv2d(xn.abs(), w.double().abs(), padding=1).permute(0, 2, 3, 1)
    bound = 2.0 ** -11 * ref.abs() + 9 * cin * U * S + 2.0 ** -14
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"conv {cin}->{cout} {H}x{W}: max err {float(err.max()):.3e}, max err/bound {worst:.3f}, "
          f"ref max {float(ref.max()):.2f}, positive {float((ref > 0).double().mean()):.2f}")
    assert float(ref.max()) > 0.1 and bool((got >= 0).all())
    assert worst <= 1.0


def test_conv_refuses_bad_arguments(cuda):
    L, st = lib(), _stream(cuda)
    t = torch.zeros(4096, dtype=torch.float16, device=cuda)
    bias = torch.zeros(64, device=cuda)
    out = torch.full((4096,), -7.0, dtype=torch.float16, device=cuda)
    p = t.data_ptr()
    for args, msg in (((p, p, bias.data_ptr(), 1, 2, 2, 32, 64, out.data_ptr(), st), "Cin must be"),
                      ((p, p, bias.data_ptr(), 1, 2, 2, 64, 32, out.data_ptr(), st), "Cout must be"),
                      ((p, p, bias.data_ptr(), 0, 2, 2, 64, 64, out.data_ptr(), st), "bad sizes"),
                      ((p, None, bias.data_ptr(), 1, 2, 2, 64, 64, out.data_ptr(), st), "null"),
                      ((p + 2, p, bias.data_ptr(), 1, 2, 2, 64, 64, out.data_ptr(), st), "aligned")):
        with pytest.raises(RuntimeError, match=msg):
            L.conv3x3_relu_f16(*args)
    with pytest.raises(RuntimeError, match="at least 2"):
        L.maxpool2_f16(p, 1, 1, 2, 64, out.data_ptr(), st)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        L.lpips_layer(p, p, bias.data_ptr(), 4, 12, out.data_ptr(), out.data_ptr(), st)
    torch.cuda.synchronize()
    assert bool((out == -7).all())                   # status 1: nothing written


# ---- 3. pool ----------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (33, 35), (2, 2)])
@pytest.mark.parametrize("C", [8, 64])
def test_pool_equals_torch(cuda, hw, C):
    H, W = hw
    x = torch.randn(2, H, W, C, generator=torch.Generator().manual_seed(H + C)).to(torch.float16)
    n_out = 2 * (H // 2) * (W // 2) * C
    out = torch.full((n_out + 128,), -7.0, dtype=torch.float16, device=cuda)
    lib().maxpool2_f16(x.to(cuda).data_ptr(), 2, H, W, C, out.data_ptr() + 128, _stream(cuda))
    got = out.cpu()
    want = R.pool2(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).to(torch.float16)
    assert want.shape == (2, H // 2, W // 2, C)
    assert bool((got[:64] == -7).all()) and bool((got[-64:] == -7).all())
    assert torch.equal(got[64:-64].reshape(want.shape), want)


# ---- 4. the per-tap distance ---------------------------------------------------------
def _layer(cuda, f0, f1, w):
    work = torch.empty(1024, dtype=torch.float64, device=cuda)
    out = torch.full((3,), -7.0, dtype=torch.float64, device=cuda)
    a, b, wd = f0.to(cuda), f1.to(cuda), w.to(cuda)
    lib().lpips_layer(a.data_ptr(), b.data_ptr(), wd.data_ptr(), f0.shape[0], f0.shape[1],
                      work.data_ptr(), out.data_ptr() + 8, _stream(cuda))
    out = out.cpu()
    assert out[0] == -7 and out[2] == -7
    return float(out[1])


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("n_pix", [1, 37, 4099])
def test_layer_vs_fp64(cuda, C, n_pix):
    """The bound is derived in the module docstring."""
    g = torch.Generator().manual_seed(C + n_pix)
    f0 = torch.randn(n_pix, C, generator=g).clamp_min(0).mul(3).to(torch.float16)
    f1 = (f0.float() + 0.5 * torch.randn(n_pix, C, generator=g)).clamp_min(0).to(torch.float16)
    if n_pix > 4:
        f0[1] = 0                           # an all-zero pixel (one image only)
        f0[2] = 0
        f1[2] = 0                           # ... and in both
        f1[3] = f0[3]                       # an equal pixel
    w = torch.rand(C, generator=g)
    w = w / w.sum()
    got = _layer(cuda, f0, f1, w) / n_pix
    a, b = f0.double(), f1.double()
    n0 = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    diff, wd = (n0 - n1).abs(), w.double()[None]
    d = (wd * diff.pow(2)).sum(1)
    same = R.tap_distance(a.t().reshape(1, C, n_pix, 1), b.t().reshape(1, C, n_pix, 1), w)
    assert torch.allclose(same[:, 0], d, rtol=1e-12, atol=0)          # the restatement's formula
    e = (C / 2 + 4) * U
    ec = e * (n0.abs() + n1.abs()) + U * diff
    B = (wd * (2 * diff * ec + ec.pow(2))).sum(1) + (C + 2) * U * (wd * (diff + ec).pow(2)).sum(1)
    ref, bound = float(d.mean()), 1.01 * float(B.mean())
    print(f"layer C={C} n={n_pix}: {got:.9e} vs fp64 {ref:.9e}: |diff| {abs(got - ref):.2e}, "
          f"bound {bound:.2e}")
    if n_pix > 4:
        assert float(d[3]) == 0.0 and float(d[2]) == 0.0 and float(d[1]) > 0
    assert ref > 0 and abs(got - ref) <= bound
    # identical inputs: exactly 0; two calls: the same bits
    assert _layer(cuda, f0, f0.clone(), w) == 0.0
    assert _layer(cuda, f0, f1, w) / n_pix == got


# ---- 5. end to end -------------------------------------------------------------------
SIZES = [(16, 16), (37, 50), (48, 64)]                  # (H, W)


@functools.lru_cache(maxsize=None)
def _weights(seed):
    return LP.synthetic_weights(seed)


def e2e_pairs(H, W, seed):
    """target uniform; pred = clip(target + sigma noise), sigma 0.05 and 0.3;
    and an unrelated image"""
    g = torch.Generator().manual_seed(100 * seed + H)
    t = torch.rand(H * W, 3, generator=g)
    out = []
    for sigma in (0.05, 0.3):
        out.append((f"sigma{sigma}", (t + sigma * torch.randn(H * W, 3, generator=g))
                    .clamp(0, 1).contiguous(), t))
    out.append(("unrelated", torch.rand(H * W, 3, generator=g), t))
    return out


def e2e_measure(cuda, seed, hw):
    """One row per image pair of a (weights, size) case: the score, both
    restatements and the relative deviations (profiles/lpips/accuracy.json
    holds these rows as measured on an MI355X)."""
    H, W = hw
    wts = _weights(seed)
    lp = LP.LPIPS(wts, (W, H), device=cuda)
    rows = []
    for name, p, t in e2e_pairs(H, W, seed):
        got = lp(p.to(cuda), t.to(cuda))
        assert got.dtype == torch.float64 and got.ndim == 0 and got.device.type == "cuda"
        terms = lp.layers(p.to(cuda), t.to(cuda))
        assert terms.shape == (5,) and float(terms.sum()) == pytest.approx(float(got), rel=1e-15)
        r16, t16 = R.lpips_ref(p, t, wts, (W, H), round_f16=True)
        r64, _ = R.lpips_ref(p, t, wts, (W, H), round_f16=False)
        rows.append({"seed": seed, "H": H, "W": W, "pair": name, "got": float(got),
                     "ref_f16": r16, "ref_full": r64, "rel_f16": abs(float(got) - r16) / r16,
                     "rel_full": abs(float(got) - r64) / r64,
                     "rel_terms_f16": [abs(float(a) - b) / b for a, b in zip(terms, t16)]})
    return lp, rows


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_to_end(cuda, seed, hw):
    lp, rows = e2e_measure(cuda, seed, hw)
    for r in rows:
        print(f"lpips seed {seed} {hw[0]}x{hw[1]} {r['pair']}: {r['got']:.9e} vs f16-storage fp64 "
              f"{r['ref_f16']:.9e} (rel {r['rel_f16']:.2e}), vs full fp64 {r['ref_full']:.9e} "
              f"(rel {r['rel_full']:.2e})")
    for r in rows:
        assert r["rel_f16"] <= BOUND_F16_REL, r
        assert r["rel_full"] <= BOUND_FULL_REL, r
    # pred is target: exactly 0; two calls give equal bits, also after an
    # unrelated call in between
    H, W = hw
    (_, p, t), (_, q, _), _ = e2e_pairs(H, W, seed)
    p, q, t = p.to(cuda), q.to(cuda), t.to(cuda)
    assert float(lp(t, t)) == 0.0 and bool((lp.layers(t, t) == 0).all())
    a = lp(p, t)
    b = lp(p, t)
    lp(q, t)
    c = lp(p, t)
    assert torch.equal(a, b) and torch.equal(a, c) and float(a) > 0
    assert torch.equal(lp.layers(p, t), lp.layers(p, t))
    # the buffers are the constructor's: a call allocates its result only
    assert lp.buf[0].numel() == 2 * H * W * 64 and lp.x.shape == (2, H, W, 3)


def test_from_files_gives_the_same_score(cuda, tmp_path):
    wts = _weights(0)
    backbone = {}
    for k, (cw, cb) in zip(LP.FEATURE_KEYS, wts["conv"]):
        backbone[f"features.{k}.weight"], backbone[f"features.{k}.bias"] = cw, cb
    lin = {f"lin{i}.model.1.weight": v.view(1, -1, 1, 1) for i, v in enumerate(wts["lin"])}
    torch.save(backbone, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    a = LP.LPIPS.from_files(tmp_path / "vgg16.pth", tmp_path / "lin.pth", (16, 16), device=cuda)
    b = LP.LPIPS(wts, (16, 16), device=cuda)
    _, p, t = e2e_pairs(16, 16, 0)[1]
    assert torch.equal(a(p.to(cuda), t.to(cuda)), b(p.to(cuda), t.to(cuda)))


# ---- 6. wiring -----------------------------------------------------------------------
def test_validate_and_fit_report_lpips(cuda):
    from radnerf_amd.evaluate import ImageEvaluator
    from radnerf_amd.trainer import Trainer
    from test_gpu_evaluate import WH, _setup
    assert WH == (24, 20)
    m, g, dirs, poses = _setup(cuda, 2, "ray", 0.5)
    gen = torch.Generator().manual_seed(4)
    u8 = torch.randint(0, 256, (2, dirs.shape[0], 3), generator=gen, dtype=torch.uint8).to(cuda)
    gt = (u8.float() / torch.full((), 255.0, device=cuda)).contiguous()
    tr = Trainer(m, g, 256, directions=dirs, poses=poses, img_wh=WH, images=u8, seed=1)
    lp = LP.LPIPS(_weights(0), WH, device=cuda)

    plain = tr.validate(poses, gt)
    assert set(plain) == {"psnr", "ssim", "per_image"}
    assert all(set(p) == {"psnr", "ssim"} for p in plain["per_image"])
    val = tr.validate(poses, gt, lpips=lp)
    assert set(val) == {"psnr", "ssim", "lpips", "per_image"}
    ev = ImageEvaluator(m, g, dirs, WH, exp_step_factor=tr.esf)
    per = []
    for i in range(2):
        rgb = ev.render_image(poses[i])["rgb"]
        want = lp(rgb, gt[i])
        per.append(want)
        one = val["per_image"][i]
        assert set(one) == {"psnr", "ssim", "lpips"}
        assert torch.equal(one["lpips"], want) and float(want) > 0
        for k in ("psnr", "ssim"):
            assert torch.equal(one[k], plain["per_image"][i][k])
        full = ev.evaluate(poses[i], gt[i], lpips=lp)
        assert torch.equal(full["lpips"], want)
        assert set(ev.evaluate(poses[i], gt[i])) == {"psnr", "ssim"}
    assert torch.equal(val["lpips"], torch.stack(per).mean())
    assert float(per[0]) != float(per[1])
    for k in ("psnr", "ssim"):
        assert torch.equal(val[k], plain[k])

    # fit: off by default, on through the class attribute's instance override
    log = tr.fit(num_epochs=1, steps_per_epoch=2, val_poses=poses, val_images=gt)
    assert set(log[0]["val"]) == {"psnr", "ssim"}
    tr.val_lpips = lp
    log = tr.fit(num_epochs=2, steps_per_epoch=2, val_poses=poses, val_images=gt, val_every=1)
    assert len(log) == 2
    for e in log:
        assert set(e["val"]) == {"psnr", "ssim", "lpips"}
        assert isinstance(e["val"]["lpips"], float) and e["val"]["lpips"] > 0
    assert log[-1]["val"]["lpips"] == float(tr.validate(poses, gt, lpips=lp)["lpips"])
    assert Trainer.val_lpips is None
