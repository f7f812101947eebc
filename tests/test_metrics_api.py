"""CPU: the surface of whole-image validation (tests/test_gpu_metrics.py and
tests/test_gpu_evaluate.py hold the GPU side).

  * rn_image_sse / rn_ssim / rn_ml_combine_test are declared in the header and
    bound in _lib with the codes csrc/gen_sig.py derives from the header; the
    ABI version stays (the entries are additive);
  * the argument checks of metrics.psnr / ssim, evaluate.ImageEvaluator and
    Trainer.validate run before the library is loaded;
  * the tests' own fp64 SSIM (tests/metrics_ref.py) is what it says: 1 on equal
    images, and an fp32 run of the same formula stays within the GPU tests'
    bars.
"""
import importlib.util
import os
import re

import pytest
import torch

import metrics_ref as MR
from radnerf_amd import _lib, evaluate, metrics
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_ml_combine_test": "ppppplilppppp", "rn_image_sse": "pplppp", "rn_ssim": "ppiiipppp"}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (metrics, evaluate, _lib):
        monkeypatch.setattr(mod, "lib", boom)


def _header_table():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    return hdr, _lib.parse_signature_table(gs.table(hdr))


def test_entries_declared_and_bound():
    hdr, table = _header_table()
    sig = _lib.binding_signatures()
    for name, codes in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert sig[name] == table[name] == codes, name
    for name, codes in sig.items():
        assert table[name] == codes, name
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    m = re.search(r"#define\s+RN_METRICS_WORK_BYTES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.METRICS_WORK_BYTES
    assert "metrics.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()


def test_psnr_argument_checks(no_library):
    a = torch.rand(30, 3)
    with pytest.raises(ValueError, match="target shape"):
        metrics.psnr(a, torch.rand(29, 3))
    with pytest.raises(ValueError, match="pred must be float32"):
        metrics.psnr(a.double(), a.double())
    with pytest.raises(ValueError, match="target must be float32"):
        metrics.psnr(a, a.half())
    with pytest.raises(ValueError, match="pred must be contiguous"):
        metrics.psnr(torch.rand(3, 30).t(), a)
    with pytest.raises(ValueError, match="target must be contiguous"):
        metrics.psnr(a, torch.rand(3, 30).t())
    with pytest.raises(ValueError, match="pred must be a tensor"):
        metrics.psnr(a.numpy(), a)
    # host tensors are refused by name too, never handed to a kernel
    with pytest.raises(ValueError, match="must be on the GPU"):
        metrics.psnr(a, a.clone())


def test_ssim_argument_checks(no_library):
    a = torch.rand(12 * 13, 3)
    with pytest.raises(ValueError, match="target shape"):
        metrics.ssim(a, torch.rand(12 * 13, 1), (13, 12))
    with pytest.raises(ValueError, match=r"img_wh 13 x 11 = 143 pixels, pred has 156 rows"):
        metrics.ssim(a, a, (13, 11))
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim(torch.rand(200, 3), torch.rand(200, 3), (20, 10))       # H = 10
    with pytest.raises(ValueError, match="at least 11"):
        metrics.ssim(torch.rand(200, 3), torch.rand(200, 3), (10, 20))       # W = 10
    with pytest.raises(ValueError, match="pred must be float32"):
        metrics.ssim(a.double(), a.double(), (13, 12))
    with pytest.raises(ValueError, match="target must be contiguous"):
        metrics.ssim(a, torch.rand(3, 12 * 13).t(), (13, 12))
    with pytest.raises(ValueError, match=r"pred must be \(H\*W, C\)"):
        metrics.ssim(torch.rand(12, 13, 3), torch.rand(12, 13, 3), (13, 12))
    with pytest.raises(ValueError, match="C <= 4"):
        metrics.ssim(torch.rand(156, 5), torch.rand(156, 5), (13, 12))
    with pytest.raises(ValueError, match="img_wh must be"):
        metrics.ssim(a, a, 13)
    with pytest.raises(ValueError, match="must be on the GPU"):
        metrics.ssim(a, a.clone(), (13, 12))
    acc = metrics.ImageMetrics()
    with pytest.raises(ValueError, match="ImageMetrics.update.*rows"):
        acc.update(a, a, (12, 12))
    with pytest.raises(ValueError, match="no image"):
        acc.compute()


def test_image_evaluator_argument_checks(no_library):
    d = torch.rand(24 * 20, 3)
    mk = lambda dirs, wh, **kw: evaluate.ImageEvaluator(None, None, dirs, wh, **kw)
    with pytest.raises(ValueError, match=r"img_wh 24 x 21 = 504 pixels, directions has 480"):
        mk(d, (24, 21))
    with pytest.raises(ValueError, match="directions must be float32"):
        mk(d.double(), (24, 20))
    with pytest.raises(ValueError, match="directions must be contiguous"):
        mk(torch.rand(3, 480).t(), (24, 20))
    with pytest.raises(ValueError, match=r"directions must be a \(H\*W, 3\)"):
        mk(torch.rand(480, 2), (24, 20))
    with pytest.raises(ValueError, match="img_wh must be"):
        mk(d, 480)
    with pytest.raises(ValueError, match="chunk must be"):
        mk(d, (24, 20), chunk=0)
    # a model without a gate must be a single NGP
    with pytest.raises(ValueError, match="gating_net=None"):
        mk(d, (24, 20))
    import inspect
    p = inspect.signature(evaluate.ImageEvaluator.__init__).parameters
    assert list(p)[1:5] == ["model", "gating_net", "directions", "img_wh"]
    assert p["exp_step_factor"].default is None and p["chunk"].default >= 1
    r = inspect.signature(evaluate.ImageEvaluator.render_image).parameters
    assert r["T_threshold"].default == 1e-4 and r["max_samples"].default == 1024


def test_trainer_validate_argument_checks(no_library):
    d, poses = torch.rand(480, 3), torch.rand(2, 3, 4)
    import inspect
    p = inspect.signature(Trainer.__init__).parameters
    assert p["img_wh"].default is None
    # raised before the model is looked at
    with pytest.raises(ValueError, match="img_wh"):
        Trainer(None, None, 64, img_wh=(24, 20))
    with pytest.raises(ValueError, match="does not match"):
        Trainer(None, None, 64, directions=d, poses=poses, img_wh=(24, 21))
    tr = Trainer.__new__(Trainer)           # validate()'s own checks, no device
    ims = torch.rand(2, 480, 3)
    for dirs, wh in ((None, None), (d, None), (None, (24, 20))):
        tr.directions, tr.img_wh = dirs, wh
        with pytest.raises(ValueError, match="Trainer.validate needs"):
            tr.validate(poses, ims)
    tr.directions, tr.img_wh = d, (24, 20)
    with pytest.raises(ValueError, match=r"poses must be \(N, 3, 4\)"):
        tr.validate(poses[0], ims)
    with pytest.raises(ValueError, match="1 images for 2 poses"):
        tr.validate(poses, ims[:1])
    with pytest.raises(ValueError, match=r"images\[0\] must be \(480, 3\)"):
        tr.validate(poses, torch.rand(2, 479, 3))
    with pytest.raises(ValueError, match=r"images\[0\] must be contiguous float32"):
        tr.validate(poses, ims.double())
    tr.directions, tr.img_wh = torch.rand(200, 3), (20, 10)
    with pytest.raises(ValueError, match="at least 11"):
        tr.validate(poses, torch.rand(2, 200, 3))


@pytest.mark.parametrize("kind", ["noise", "ramp", "flat"])
def test_reference_ssim_and_fp32_spread(kind):
    """The yardstick of the GPU tests: the fp64 restatement gives 1 on equal
    images, and the GPU tests' bars (1e-4 in the mean, 1e-3 per pixel) are
    within reach of fp32 at all: the same formula run in plain fp32 on the same
    images stays inside them (the flat and low-variance regions, where
    E[x^2] - mu^2 cancels against c2 = 9e-4, come closest)."""
    wh = (59, 77)
    pred, tgt = MR.images(kind, wh, 3)
    one, m1 = MR.ssim_ref(tgt, tgt, wh)
    assert abs(one - 1) <= 1e-12 and float((m1 - 1).abs().max()) <= 1e-9
    mean64, map64 = MR.ssim_ref(pred, tgt, wh)
    mean32, map32 = MR.ssim_ref(pred, tgt, wh, dtype=torch.float32)
    assert map64.shape == (67, 49, 3) and -1 < mean64 < 1
    assert abs(mean32 - mean64) <= 1e-4
    assert float((map32.double() - map64).abs().max()) <= 1e-3
    assert MR.psnr_ref(tgt, tgt) == float("inf")
    assert abs(MR.psnr_ref(torch.zeros(4, 3), torch.full((4, 3), 0.1)) - 20.0) <= 1e-5
