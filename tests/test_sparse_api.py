"""CPU: the surface of the gate-sparse test-time render
(tests/test_gpu_sparse_render.py holds the GPU side).

  * rn_gate_select / rn_render_test_list are declared in the header, exported
    and bound with the codes csrc/gen_sig.py derives; the ABI version stays
    (additive entries); gate_select.hip is in the Makefile's source list;
  * the argument checks of sparse_gate.select, ImageEvaluator.render_image /
    evaluate and Trainer.validate raise ValueError naming the argument and its
    value before the library is loaded;
  * arguments that keep every pair never reach the selection.
"""
import importlib.util
import inspect
import os
import re
import types

import pytest
import torch

from radnerf_amd import _lib, evaluate, metrics, sparse_gate
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_gate_select": "plifiipppppppppp",
       "rn_render_test_list": "ppplipliffiippppppppfppppppip"}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (metrics, evaluate, sparse_gate, _lib):
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
    # rn_render_test's arguments, then list and count, then blocks and the stream
    dense, sparse = NEW["rn_render_test_list"], sig["rn_render_test"]
    assert dense == sparse[:-2] + "pp" + sparse[-2:]
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    m = re.search(r"#define\s+RN_GATE_SELECT_WORK_BYTES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.GATE_SELECT_WORK_BYTES
    # the scratch holds one int32 per (sub-NeRF <= 16, block <= 1024)
    assert _lib.GATE_SELECT_WORK_BYTES == 16 * 1024 * 4
    mk = open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "gate_select.hip" in srcs and "render.hip" in srcs
    # both sources cite the reference lines the feature answers
    for f in ("gate_select.hip", "render.hip"):
        text = open(os.path.join(ROOT, "rad-nerf_amd", "csrc", f)).read()
        assert "ml_rendering.py:33-36,65-68" in text and "networks.py:1087-1093" in text, f
    assert "ml_rendering.py:33-36,65-68" in hdr and "networks.py:1087-1093" in hdr


def test_select_argument_checks(no_library):
    g = torch.rand(10, 4)
    sel = sparse_gate.select
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match=r"gate_min must be a number in \[0, 1\), got " +
                           re.escape(repr(bad))):
            sel(g, gate_min=bad)
    for bad in (0, 5, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match=r"gate_topk must be None or an int in \[1, 4\].*got "
                           + re.escape(repr(bad))):
            sel(g, gate_topk=bad)
    with pytest.raises(ValueError, match="gate must be float32, got torch.float64"):
        sel(g.double())
    with pytest.raises(ValueError, match="gate must be contiguous"):
        sel(torch.rand(4, 10).t())
    with pytest.raises(ValueError, match=r"gate must be a \(n, K\) tensor"):
        sel(torch.rand(10))
    with pytest.raises(ValueError, match=r"gate must be a \(n, K\) tensor"):
        sel(g.numpy())
    with pytest.raises(ValueError, match="17 columns"):
        sel(torch.rand(3, 17))
    # a host gate is refused by name, never handed to a kernel
    with pytest.raises(ValueError, match="gate must be on the GPU, got a cpu tensor"):
        sel(g, gate_min=0.5, gate_topk=2, renormalize=True)
    p = inspect.signature(sel).parameters
    assert list(p) == ["gate", "gate_min", "gate_topk", "renormalize", "out"]
    assert (p["gate_min"].default, p["gate_topk"].default, p["renormalize"].default,
            p["out"].default) == (0.0, None, False, None)


def _evaluator(K, gate=True):
    ev = evaluate.ImageEvaluator.__new__(evaluate.ImageEvaluator)
    ev.model = types.SimpleNamespace(size=K)
    ev.gate = object() if gate else None
    return ev


def test_evaluator_argument_checks(no_library):
    ev = _evaluator(3)
    pose = torch.eye(4)[:3]
    for kw, pat in (({"gate_min": 1.0}, r"render_image: gate_min must be .* got 1.0"),
                    ({"gate_min": -1e-3}, r"gate_min must be .* got -0.001"),
                    ({"gate_topk": 4}, r"render_image: gate_topk must be .*\[1, 3\].* got 4"),
                    ({"gate_topk": 0}, r"gate_topk must be .* got 0"),
                    ({"gate_topk": 1.5}, r"gate_topk must be .* got 1.5")):
        with pytest.raises(ValueError, match=pat):
            ev.render_image(pose, **kw)
    # a single NGP has one sub-NeRF: only gate_topk 1 (or None) is in range
    with pytest.raises(ValueError, match=r"gate_topk must be .*\[1, 1\].* got 2"):
        _evaluator(1, gate=False).render_image(pose, gate_topk=2)
    for fn in (evaluate.ImageEvaluator.render_image, evaluate.ImageEvaluator.evaluate,
               Trainer.validate):
        p = inspect.signature(fn).parameters
        assert (p["gate_min"].default, p["gate_topk"].default,
                p["renormalize"].default) == (0.0, None, False), fn
    r = list(inspect.signature(evaluate.ImageEvaluator.render_image).parameters)
    assert r[:4] == ["self", "pose", "T_threshold", "max_samples"]


def test_dense_arguments_never_reach_select(no_library):
    """gate_min 0 with gate_topk None or K, one sub-NeRF, or no gate: the
    evaluator's decision is `dense` (None), whatever renormalize says."""
    fn = "t"
    for K in (2, 3, 16):
        ev = _evaluator(K)
        for renorm in (False, True):
            assert ev._sparse_params(fn, 0.0, None, renorm) is None
            assert ev._sparse_params(fn, 0, K, renorm) is None
            assert ev._sparse_params(fn, 0.0, K - 1, renorm) == (0.0, K - 1, int(renorm))
            assert ev._sparse_params(fn, 0.25, None, renorm) == (0.25, K, int(renorm))
        # no gate at all (a caller's own model): dense
        assert _evaluator(K, gate=False)._sparse_params(fn, 0.5, 1, True) is None
    assert _evaluator(1)._sparse_params(fn, 0.5, 1, True) is None
    assert _evaluator(1, gate=False)._sparse_params(fn, 0.0, None, False) is None
    assert sparse_gate.is_dense(1, 0.9, 1) and sparse_gate.is_dense(4, 0.0, 4)
    assert not sparse_gate.is_dense(4, 0.0, 3) and not sparse_gate.is_dense(4, 1e-7, 4)
