"""CPU: routed training's interface -- the argument checks (ValueError with
the offending value, before the library is touched), what is refused
(NotImplementedError: the pinned layout, ml_render(fused=False)),
Trainer.routing, and the routing fields of the training state (recorded when
set; a state without them is a dense one).  The GPU side is
tests/test_gpu_routed.py.
"""
import inspect
import re
import os

import pytest
import torch

from radnerf_amd import _lib, fused, sparse_gate
from radnerf_amd.fused import FusedMLRenderer, ml_render_fused, route_params
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.pinned import PinnedMLRenderer
from radnerf_amd.rendering import ml_render
from radnerf_amd.trainer import Trainer
from test_train_state_api import _trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (fused, sparse_gate, _lib):
        monkeypatch.setattr(mod, "lib", boom)


BAD = [(dict(gate_topk=0), "gate_topk.*got 0"), (dict(gate_topk=5), "gate_topk.*got 5"),
       (dict(gate_topk=1.0), "gate_topk.*got 1.0"), (dict(gate_topk=True), "gate_topk.*got True"),
       (dict(gate_min=1.0), "gate_min.*got 1.0"), (dict(gate_min=-0.1), "gate_min.*got -0.1"),
       (dict(gate_min="x"), "gate_min.*got 'x'")]


def test_route_params():
    assert route_params("f", 4) is None
    assert route_params("f", 4, 4, 0.0, False) is None
    assert route_params("f", 4, None, 0.0, False, always=True) == (4, 0.0, False)
    assert route_params("f", 4, 2) == (2, 0.0, False)
    assert route_params("f", 4, None, 0.25) == (4, 0.25, False)
    assert route_params("f", 4, None, 0.0, True) == (4, 0.0, True)
    # one sub-NeRF: accepted and ignored
    assert route_params("f", 1, 3, 0.5, True, always=True) is None
    for kw, msg in BAD:
        with pytest.raises(ValueError, match="f: " + msg):
            route_params("f", 4, **kw)


def test_signatures_and_header():
    for fn in (FusedMLRenderer.forward, FusedMLRenderer.train_step, PinnedMLRenderer.forward):
        p = inspect.signature(fn).parameters
        assert (p["gate_topk"].default, p["gate_min"].default, p["renormalize"].default) == \
            (None, 0.0, False), fn
    p = inspect.signature(Trainer.__init__).parameters
    assert [p[k].default for k in ("gate_topk", "gate_min", "renormalize", "route_from_step")] \
        == [None, 0.0, False, 0]
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    sig = _lib.binding_signatures()
    for name in ("rn_ml_march_count_list", "rn_gate_select_bw", "rn_nerf_loss_routed",
                 "rn_nerf_loss_routed_det"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in sig
    # rn_ml_march_count's arguments, then list and count; the dense entries as they were
    assert sig["rn_ml_march_count_list"] == sig["rn_ml_march_count"][:-1] + "ppp"
    assert sig["rn_nerf_loss_routed"] == sig["rn_nerf_loss"][:5] + "p" + sig["rn_nerf_loss"][5:]
    assert sig["rn_nerf_loss_routed_det"] == \
        sig["rn_nerf_loss_det"][:5] + "p" + sig["rn_nerf_loss_det"][5:]
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)


@pytest.mark.parametrize("kw,msg", BAD)
def test_ml_render_checks_before_any_launch(no_library, kw, msg):
    m, g = MNGP(0.5, size=4, t=8, seed=1), Ray_Gate(4, seed=2)
    o = torch.zeros(8, 3)
    with pytest.raises(ValueError, match="ml_render: " + msg):
        ml_render_fused(m, g, o, o, o, **kw)
    with pytest.raises(ValueError, match="ml_render: " + msg):
        ml_render(m, g, o, o, o, fused=False, **kw)


def test_unfused_and_pinned_refuse_routing(no_library):
    m, g = MNGP(0.5, size=2, t=8, seed=1), Ray_Gate(2, seed=2)
    o = torch.zeros(8, 3)
    for kw in (dict(gate_topk=1), dict(gate_min=0.1), dict(renormalize=True)):
        with pytest.raises(NotImplementedError, match="routed training"):
            ml_render(m, g, o, o, o, fused=False, **kw)
        with pytest.raises(NotImplementedError, match="routed training"):
            ml_render(m, g, o, o, o, test_time=True, **kw)
        r = PinnedMLRenderer.__new__(PinnedMLRenderer)      # the check comes before any state
        with pytest.raises(NotImplementedError, match="routed training"):
            r.forward(o, o, o, torch.zeros(2, 8), torch.ones(3), **kw)
    r = PinnedMLRenderer.__new__(PinnedMLRenderer)
    with pytest.raises(ValueError, match="gate_topk.*got 3"):
        r.forward(o, o, o, torch.zeros(2, 8), torch.ones(3), gate_topk=3)


@pytest.mark.parametrize("kw,msg", BAD + [(dict(route_from_step=-1), "route_from_step.*got -1"),
                                          (dict(route_from_step=1.5), "route_from_step.*got 1.5")])
def test_trainer_checks_before_anything_is_allocated(no_library, monkeypatch, kw, msg):
    def boom(*a, **k):
        raise AssertionError("the renderer was built before the argument check")
    monkeypatch.setattr("radnerf_amd.trainer.FusedMLRenderer", boom)
    m, g = MNGP(0.5, size=4, t=8, seed=1), Ray_Gate(4, seed=2)
    with pytest.raises(ValueError, match="Trainer: " + msg):
        Trainer(m, g, 64, **kw)


def test_trainer_routing_property():
    tr = _trainer()
    assert tr.routing == {"gate_topk": None, "gate_min": 0.0, "renormalize": False}
    tr = _trainer(gate_topk=1, gate_min=0.125, renormalize=True, route_from_step=3)
    assert tr.routing == {"gate_topk": 1, "gate_min": 0.125, "renormalize": True}
    # validate() and the image renderer take exactly these
    p = inspect.signature(Trainer.validate).parameters
    assert set(tr.routing) <= set(p)
    assert [p[k].default for k in ("gate_topk", "gate_min", "renormalize")] == [None, 0.0, False]
    # dense before route_from_step, routed from it on
    tr.global_step = 2
    assert tr._route_now() == {}
    tr.global_step = 3
    assert tr._route_now() == tr.routing


def test_state_records_the_routing():
    dense = _trainer()
    routed = _trainer(gate_topk=1, gate_min=0.125, renormalize=True, route_from_step=3)
    sd, sr = dense.state_dict(), routed.state_dict()
    new = {"gate_topk", "gate_min", "renormalize", "route_from_step"}
    # a dense trainer writes the fields it always wrote
    assert not new & set(sd["hyper"])
    assert {k: sr["hyper"][k] for k in new} == {"gate_topk": 1, "gate_min": 0.125,
                                                "renormalize": True, "route_from_step": 3}
    assert set(sr["hyper"]) - new == set(sd["hyper"])
    # gate_topk None is recorded as all K
    assert _trainer(gate_min=0.5).state_dict()["hyper"]["gate_topk"] == 2


def test_state_without_routing_loads_as_dense():
    old = _trainer().state_dict()               # the format before routing existed
    fresh = _trainer(seed=1, filled=False)
    fresh.load_state_dict(old)
    assert fresh.global_step == 37 and fresh.routing["gate_topk"] is None
    # ... and into a routed trainer it is a hyper-parameter difference, listed
    routed = _trainer(seed=1, filled=False, gate_topk=1, route_from_step=3)
    with pytest.raises(ValueError) as e:
        routed.load_state_dict(old)
    msg = str(e.value)
    assert "override=True" in msg
    assert "gate_topk: saved 2, this trainer 1" in msg
    assert "route_from_step: saved 0, this trainer 3" in msg
    assert routed.global_step == 0
    routed.load_state_dict(old, override=True)
    assert routed.global_step == 37 and routed.routing["gate_topk"] == 1
    # a routed state into a dense trainer likewise; into its like it loads
    sr = _trainer(gate_topk=1, route_from_step=3).state_dict()
    with pytest.raises(ValueError, match="gate_topk: saved 1, this trainer 2"):
        _trainer(seed=1, filled=False).load_state_dict(sr)
    twin = _trainer(seed=1, filled=False, gate_topk=1, route_from_step=3)
    twin.load_state_dict(sr)
    assert twin.global_step == 37
