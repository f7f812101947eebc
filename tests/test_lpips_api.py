"""CPU: the surface of LPIPS (tests/test_gpu_lpips.py holds the GPU side).

  * the four entries are declared in the header and bound in _lib with the
    codes csrc/gen_sig.py derives; lpips.hip is built; the ABI version stays;
  * the argument checks of lpips.LPIPS and of the lpips= wiring run before the
    library is loaded;
  * every new default is None, and fit / fit_resumable keep their arguments.
"""
import importlib.util
import inspect
import os
import re

import pytest
import torch

from radnerf_amd import _lib, evaluate, lpips, metrics
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_lpips_prepare": "plpp", "rn_conv3x3_relu_f16": "pppiiiiipp",
       "rn_maxpool2_f16": "piiiipp", "rn_lpips_layer": "ppplippp"}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (metrics, evaluate, lpips, _lib):
        monkeypatch.setattr(mod, "lib", boom)


def test_entries_declared_and_bound():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    table = _lib.parse_signature_table(gs.table(hdr))
    sig = _lib.binding_signatures()
    for name, codes in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert sig[name] == table[name] == codes, name
    # appended: the last four entries of the header's table and of the binding
    assert list(table)[-4:] == list(NEW) == list(_lib.SIGNATURES)[-4:]
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    mk = open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()
    assert "lpips.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()


def test_new_defaults_are_none():
    assert inspect.signature(metrics.ImageMetrics.__init__).parameters["lpips"].default is None
    ev = inspect.signature(evaluate.ImageEvaluator.evaluate).parameters
    assert ev["lpips"].default is None and list(ev)[-1] == "lpips"
    v = inspect.signature(Trainer.validate).parameters
    assert v["lpips"].default is None
    assert list(v)[-2:] == ["renormalize", "lpips"]           # appended after renormalize
    assert Trainer.val_lpips is None
    # fit and fit_resumable keep their argument lists
    assert list(inspect.signature(Trainer.fit).parameters) == [
        "self", "num_epochs", "steps_per_epoch", "val_poses", "val_images", "val_every",
        "eta_min", "callback"]
    assert "lpips" not in inspect.signature(Trainer.fit_resumable).parameters
    assert inspect.signature(lpips.LPIPS.__init__).parameters["device"].default is None


def test_constructor_argument_checks(no_library):
    w = lpips.synthetic_weights(0)
    with pytest.raises(ValueError, match="img_wh must be"):
        lpips.LPIPS(w, 32)
    with pytest.raises(ValueError, match="at least 16"):
        lpips.LPIPS(w, (15, 32))
    with pytest.raises(ValueError, match="at least 16"):
        lpips.LPIPS(w, (32, 15))
    with pytest.raises(ValueError, match="weights must be a dict"):
        lpips.LPIPS([1, 2], (32, 32))
    with pytest.raises(ValueError, match=r'weights\["conv"\] must hold 13'):
        lpips.LPIPS({"conv": w["conv"][:12], "lin": w["lin"]}, (32, 32))
    with pytest.raises(ValueError, match=r'weights\["lin"\] must hold 5'):
        lpips.LPIPS({"conv": w["conv"], "lin": w["lin"][:4]}, (32, 32))
    bad = list(w["conv"])
    bad[2] = (torch.zeros(128, 64, 3, 2), bad[2][1])
    with pytest.raises(ValueError, match=r'weights\["conv"\]\[2\] weight must be \(128, 64, 3, 3\)'):
        lpips.LPIPS({"conv": bad, "lin": w["lin"]}, (32, 32))
    bad = list(w["conv"])
    bad[0] = (bad[0][0], torch.zeros(63))
    with pytest.raises(ValueError, match=r'weights\["conv"\]\[0\] bias must be \(64,\)'):
        lpips.LPIPS({"conv": bad, "lin": w["lin"]}, (32, 32))
    bad = list(w["lin"])
    bad[1] = torch.zeros(127)
    with pytest.raises(ValueError, match=r'weights\["lin"\]\[1\] must be \(128,\)'):
        lpips.LPIPS({"conv": w["conv"], "lin": bad}, (32, 32))
    bad = list(w["lin"])
    bad[4] = -bad[4]
    with pytest.raises(ValueError, match=r'weights\["lin"\]\[4\] has a negative'):
        lpips.LPIPS({"conv": w["conv"], "lin": bad}, (32, 32))
    with pytest.raises(ValueError, match="device must be a GPU"):
        lpips.LPIPS(w, (32, 32), device="cpu")


def test_call_argument_checks(no_library):
    lp = lpips.LPIPS.__new__(lpips.LPIPS)           # the call's own checks, no device
    lp.img_wh, lp.device = (20, 16), torch.device("cuda", 0)
    a = torch.rand(320, 3)
    for call in (lp, lp.layers):
        with pytest.raises(ValueError, match="target shape"):
            call(a, torch.rand(319, 3))
        with pytest.raises(ValueError, match="pred must be float32"):
            call(a.double(), a.double())
        with pytest.raises(ValueError, match="target must be contiguous"):
            call(a, torch.rand(3, 320).t())
        with pytest.raises(ValueError, match=r"img_wh 20 x 16 = 320 pixels, pred has 300 rows"):
            call(torch.rand(300, 3), torch.rand(300, 3))
        with pytest.raises(ValueError, match=r"pred must be \(H\*W, 3\)"):
            call(torch.rand(320, 1), torch.rand(320, 1))
        with pytest.raises(ValueError, match="must be on the GPU"):
            call(a, a.clone())


def test_wiring_argument_checks(no_library):
    lp = lpips.LPIPS.__new__(lpips.LPIPS)
    lp.img_wh, lp.device = (24, 20), torch.device("cuda", 0)
    with pytest.raises(ValueError, match="ImageMetrics: lpips must be None or a"):
        metrics.ImageMetrics(lpips=lambda a, b: 0)
    acc = metrics.ImageMetrics(lpips=lp)
    a = torch.rand(16 * 16, 3)
    with pytest.raises(ValueError, match=r"lpips was built for img_wh \(24, 20\)"):
        acc.update(a, a, (16, 16))
    assert metrics.ImageMetrics().lpips is None
    # Trainer.validate: after its own checks, before anything is rendered
    tr = Trainer.__new__(Trainer)
    tr.directions, tr.img_wh = torch.rand(16 * 16, 3), (16, 16)
    poses, ims = torch.rand(2, 3, 4), torch.rand(2, 256, 3)
    with pytest.raises(ValueError, match=r"poses must be \(N, 3, 4\)"):
        tr.validate(poses[0], ims, lpips=lp)
    with pytest.raises(ValueError, match=r"Trainer.validate: lpips was built for img_wh \(24, 20\)"):
        tr.validate(poses, ims, lpips=lp)
    with pytest.raises(ValueError, match="Trainer.validate: lpips must be None or a"):
        tr.validate(poses, ims, lpips="vgg")
    ev = evaluate.ImageEvaluator.__new__(evaluate.ImageEvaluator)
    ev.img_wh, ev.n_pix = (16, 16), 256
    with pytest.raises(ValueError, match=r"ImageEvaluator.evaluate: lpips was built for"):
        ev.evaluate(torch.rand(3, 4), ims[0], lpips=lp)


def test_synthetic_weights_recipe():
    a, b = lpips.synthetic_weights(1), lpips.synthetic_weights(1)
    c = lpips.synthetic_weights(2)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
               for x, y in zip(a["conv"], b["conv"]))
    assert not torch.equal(a["conv"][0][0], c["conv"][0][0])
    for (cin, cout), (w, bias) in zip(lpips.CONVS, a["conv"]):
        assert tuple(w.shape) == (cout, cin, 3, 3) and tuple(bias.shape) == (cout,)
        assert float(bias.abs().max()) <= 0.1
        if cin >= 64:       # enough samples: the He-normal standard deviation
            assert abs(float(w.std()) / (2.0 / (9 * cin)) ** 0.5 - 1) <= 0.05
    for ch, v in zip(lpips.TAP_CHANNELS, a["lin"]):
        assert tuple(v.shape) == (ch,) and float(v.min()) >= 0
        assert abs(float(v.sum()) - 1) <= 1e-5
