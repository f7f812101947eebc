"""CPU: the fp64 restatement of LPIPS-VGG (tests/lpips_ref.py) is what it
says, and the weight loader of radnerf_amd/lpips.py maps the published key
names.

  * identical images give exactly 0, the distance is symmetric;
  * the convolution against a second opinion (scipy.signal.correlate2d);
  * the pool's floor sizes on odd inputs;
  * a one-tap example worked by hand;
  * f16 storage alone (round_f16) stays within 3e-4 of full precision on the
    recipe of the GPU tests;
  * synthetic state dicts of the published shapes map through
    weights_from_state_dicts, survive torch.save / LPIPS-style loading with
    weights_only=True, and every refusal names its key;
  * pack_conv puts every weight where include/radnerf.h says.
"""
import numpy as np
import pytest
import torch

import lpips_ref as R
from radnerf_amd import lpips as LP


def _pair(H, W, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(H * W, 3, generator=g)
    p = (t + sigma * torch.randn(H * W, 3, generator=g)).clamp(0, 1).contiguous()
    return p, t


@pytest.fixture(scope="module")
def weights():
    return LP.synthetic_weights(0)


def test_identical_is_zero_and_symmetric(weights):
    p, t = _pair(16, 19, 0.3, 1)
    for rnd in (False, True):
        s, terms = R.lpips_ref(t, t.clone(), weights, (19, 16), rnd)
        assert s == 0.0 and terms == [0.0] * 5
        a, ta = R.lpips_ref(p, t, weights, (19, 16), rnd)
        b, tb = R.lpips_ref(t, p, weights, (19, 16), rnd)
        assert a > 0 and len(ta) == 5 and min(ta) >= 0
        assert a == b and ta == tb


def test_f16_storage_stays_close(weights):
    for (H, W), sigma in (((16, 16), 0.05), ((37, 50), 0.3)):
        p, t = _pair(H, W, sigma, H)
        full, _ = R.lpips_ref(p, t, weights, (W, H))
        half, _ = R.lpips_ref(p, t, weights, (W, H), round_f16=True)
        assert abs(half - full) <= 3e-4 * full


def test_conv_against_scipy():
    from scipy.signal import correlate2d
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 3, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    got = R.conv3x3_relu(x, w, b)[0].numpy()
    for co in range(4):
        acc = sum(correlate2d(x[0, c].numpy(), w[co, c].numpy(), mode="same", boundary="fill")
                  for c in range(3)) + float(b[co])
        assert np.allclose(got[co], np.maximum(acc, 0.0), rtol=0, atol=1e-12)
    assert (got == 0).any() and (got > 0).any()           # the ReLU does something


def test_pool_floor_sizes():
    x = torch.arange(2 * 5 * 7, dtype=torch.float64).reshape(1, 2, 5, 7)
    y = R.pool2(x)
    assert y.shape == (1, 2, 2, 3)
    # ascending values: the maximum of a block is its bottom-right element,
    # and the last row and column (index 4 and 6) are never read
    assert torch.equal(y[0, 0], torch.tensor([[8., 10., 12.], [22., 24., 26.]], dtype=torch.float64))
    assert R.pool2(torch.zeros(1, 1, 33, 35)).shape == (1, 1, 16, 17)
    assert R.pool2(torch.zeros(1, 1, 2, 2)).shape == (1, 1, 1, 1)


def test_tap_distance_by_hand():
    # one pixel, two channels: f0 = (3, 4) -> n0 = (.6, .8); f1 = (0, 5) -> n1 = (0, 1);
    # w = (.25, .75): d = .25 * .36 + .75 * .04 = .12
    f0 = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    f1 = torch.tensor([0.0, 5.0], dtype=torch.float64).view(1, 2, 1, 1)
    d = R.tap_distance(f0, f1, torch.tensor([0.25, 0.75]))
    assert d.shape == (1, 1) and abs(float(d) - 0.12) <= 1e-9     # (the 1e-10 in the norm)
    # an all-zero feature vector: 0 / (0 + 1e-10) = 0, so d = sum w n1^2 = .75
    z = torch.zeros_like(f0)
    assert abs(float(R.tap_distance(z, f1, torch.tensor([0.25, 0.75]))) - 0.75) <= 1e-9
    assert float(R.tap_distance(z, z, torch.tensor([0.25, 0.75]))) == 0.0


def test_prepare_by_hand():
    x = torch.tensor([[0.0, 0.5, 1.0], [-1.0, 2.0, 0.25]])
    y = R.prepare(x, (2, 1))
    assert y.shape == (1, 3, 1, 2)
    sh = [float(np.float32(v)) for v in R.SHIFT]
    sc = [float(np.float32(v)) for v in R.SCALE]
    want = [[(-1 - sh[0]) / sc[0], (0 - sh[1]) / sc[1], (1 - sh[2]) / sc[2]],
            [(-1 - sh[0]) / sc[0], (1 - sh[1]) / sc[1], (-0.5 - sh[2]) / sc[2]]]
    assert np.allclose(y[0].permute(1, 2, 0)[0].numpy(), np.array(want), rtol=0, atol=1e-15)


# ---- the loader ---------------------------------------------------------------
def _state_dicts(w):
    backbone = {}
    for k, (cw, cb) in zip(LP.FEATURE_KEYS, w["conv"]):
        backbone[f"features.{k}.weight"] = cw.clone()
        backbone[f"features.{k}.bias"] = cb.clone()
    backbone["classifier.0.weight"] = torch.zeros(2, 2)          # the rest of VGG16 is ignored
    lin = {f"lin{i}.model.1.weight": v.clone().view(1, -1, 1, 1) for i, v in enumerate(w["lin"])}
    return backbone, lin


def test_loader_key_mapping(weights, tmp_path):
    assert LP.FEATURE_KEYS == (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
    assert [tuple(w.shape) for w, _ in weights["conv"]] == \
        [(co, ci, 3, 3) for ci, co in LP.CONVS]
    assert LP.TAP_CHANNELS == (64, 128, 256, 512, 512)
    backbone, lin = _state_dicts(weights)
    got = LP.weights_from_state_dicts(backbone, lin)
    for (a, b), (c, d) in zip(got["conv"], weights["conv"]):
        assert torch.equal(a, c) and torch.equal(b, d)
    for a, c in zip(got["lin"], weights["lin"]):
        assert a.shape == c.shape and torch.equal(a, c)
    # a round trip through files, read with weights_only=True
    torch.save(backbone, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    b2 = torch.load(tmp_path / "vgg16.pth", weights_only=True)
    l2 = torch.load(tmp_path / "lin.pth", weights_only=True)
    again = LP.weights_from_state_dicts(b2, l2)
    assert all(torch.equal(a, c) for (a, _), (c, _) in zip(again["conv"], weights["conv"]))
    # the same score through the restatement
    p, t = _pair(16, 16, 0.3, 5)
    assert R.lpips_ref(p, t, again, (16, 16)) == R.lpips_ref(p, t, weights, (16, 16))


def test_loader_refusals(weights):
    backbone, lin = _state_dicts(weights)
    bad = dict(backbone)
    del bad["features.17.bias"]
    with pytest.raises(ValueError, match=r"no features\.17\.bias"):
        LP.weights_from_state_dicts(bad, lin)
    bad = dict(backbone)
    bad["features.5.weight"] = torch.zeros(128, 64, 3, 2)
    with pytest.raises(ValueError, match=r"features\.5\.weight must be \(128, 64, 3, 3\)"):
        LP.weights_from_state_dicts(bad, lin)
    bad = dict(lin)
    del bad["lin3.model.1.weight"]
    with pytest.raises(ValueError, match=r"no lin3\.model\.1\.weight"):
        LP.weights_from_state_dicts(backbone, bad)
    bad = dict(lin)
    bad["lin0.model.1.weight"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight must be \(1, 64, 1, 1\)"):
        LP.weights_from_state_dicts(backbone, bad)
    bad = dict(lin)
    neg = lin["lin4.model.1.weight"].clone()
    neg[0, 7, 0, 0] = -1e-3
    bad["lin4.model.1.weight"] = neg
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight has a negative"):
        LP.weights_from_state_dicts(backbone, bad)


def test_pack_conv_layout():
    """Every weight lands where the header's index formula says."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(64, 128, 3, 3, generator=g)
    f = LP.pack_conv(w).view(-1, 64, 8)                   # [fragment][lane][j]
    assert f.dtype == torch.float16 and f.numel() == 9 * 128 * 64
    h16 = w.to(torch.float16)
    for ct, chunk, tap, ks, lane, j in ((0, 0, 0, 0, 0, 0), (1, 1, 8, 3, 63, 7), (1, 0, 4, 2, 37, 5),
                                        (0, 1, 5, 1, 31, 3)):
        r, h = lane & 31, lane >> 5
        frag = ((ct * 2 + chunk) * 9 + tap) * 4 + ks
        assert f[frag, lane, j] == h16[32 * ct + r, 64 * chunk + 16 * ks + 8 * h + j, tap // 3, tap % 3]
    w = torch.randn(64, 3, 3, 3, generator=g)
    f = LP.pack_conv(w).view(-1, 64, 8)
    assert f.numel() == 32 * 64
    h16 = w.to(torch.float16)
    for ct, ks, lane, j in ((0, 0, 0, 0), (1, 1, 40, 2), (1, 0, 63, 7), (0, 1, 5, 4)):
        r, h = lane & 31, lane >> 5
        k = 16 * ks + 8 * h + j
        want = h16[32 * ct + r, k % 3, (k // 3) // 3, (k // 3) % 3] if k < 27 else 0
        assert f[2 * ct + ks, lane, j] == want
    assert (f.view(2, 2, 64, 8)[:, 1, 32:, 3:] == 0).all()        # k = 27 .. 31
