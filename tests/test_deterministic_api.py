"""CPU: the surface of the deterministic training mode
(FusedMLRenderer(deterministic=True), Trainer(deterministic=True);
tests/test_gpu_deterministic.py holds the GPU side).

  * the five entries are declared in the header and bound in _lib with the
    codes csrc/gen_sig.py derives from the header; the ABI version stays 9;
  * the entries' argument checks return status 1 before any device is touched;
  * what the mode refuses (more than 8 sub-NeRFs, the sub-NeRF-per-GPU layout,
    the per-model backward) raises ValueError at construction;
  * Trainer passes the flag to its renderer, scatter_mode reports "int-grad".
"""
import ctypes
import importlib.util
import inspect
import os
import re

import pytest
import torch

from radnerf_amd import _lib
from radnerf_amd.fused import FusedMLRenderer, get_renderer
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.pinned import PinnedMLRenderer
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "rn_reduce_partials": "pilpp",
    "rn_colsum_ordered": "plipp",
    "rn_field_bwd_merged_det": "pppppppppp" "lii" "pppppppppppppp" "l" "p" "ii" "ppp" "p",
    "rn_gate_bwd_det": "ppilipppippip",
    "rn_nerf_loss_det": "pppppp" "li" "fff" "ppppppp",
}
CPU = torch.device("cpu")


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
    # every bound entry still equals the header's (nothing else moved)
    for name, codes in sig.items():
        assert table[name] == codes, name
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    # the gate's deterministic backward takes rn_gate_bwd's arguments, and
    # rn_field_bwd_merged keeps its signature
    assert sig["rn_gate_bwd_det"] == sig["rn_gate_bwd"]
    assert sig["rn_field_bwd_merged"] == "pppppppppplii" + "p" * 14 + "lpiipppppppipppip"
    # the contracts are stated where the entries are declared
    assert "ORDER\n * CONTRACT" in hdr or "ORDER CONTRACT" in hdr
    assert "SCHEDULE CONTRACT" in hdr


def test_library_table_lists_the_entries():
    L = _lib.lib()
    fn = L.handle.rn_abi_signatures
    have = _lib.parse_signature_table(fn().decode())
    for name, codes in NEW.items():
        assert have[name] == codes, name
        assert callable(getattr(L, name[3:]))


def _status(name, *args):
    """the raw status of an entry (the binding's wrapper raises on non-zero)"""
    L = _lib.lib()
    fn = getattr(L.handle, name)
    fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int
    st = fn(*args)
    return st, L.handle.rn_last_error().decode("utf-8", "replace")


def test_reduce_partials_argument_checks():
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    for args in ((p, 0, 4, p, None), (p, -1, 4, p, None), (p, 2, -1, p, None),
                 (None, 2, 4, p, None), (p, 2, 4, None, None)):
        st, msg = _status("rn_reduce_partials", *args)
        assert st == 1 and "rn_reduce_partials" in msg, (args, st, msg)
    with pytest.raises(RuntimeError, match="status 1"):
        _lib.lib().reduce_partials(p, 0, 4, p, None)


def test_colsum_ordered_argument_checks():
    buf = (ctypes.c_float * 32)()
    p = ctypes.addressof(buf)
    for cols in (0, -1, 17):
        st, msg = _status("rn_colsum_ordered", p, 2, cols, p, None)
        assert st == 1 and "rn_colsum_ordered" in msg, (cols, st, msg)
    assert _status("rn_colsum_ordered", p, -1, 4, p, None)[0] == 1
    assert _status("rn_colsum_ordered", None, 2, 4, p, None)[0] == 1
    assert _status("rn_colsum_ordered", p, 2, 4, None, None)[0] == 1


def test_field_bwd_merged_det_argument_checks():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    codes = NEW["rn_field_bwd_merged_det"]
    full = [p if c == "p" else 1 for c in codes]
    full[-1] = None                              # the stream
    # positions as in the header
    i_dw_part, i_lo, i_carry, i_scale = 24, 31, 32, 33
    assert codes[i_dw_part] == codes[i_lo] == codes[i_carry] == codes[i_scale] == "p"
    for i, what in ((i_lo, "igrad"), (i_carry, "igrad"), (i_scale, "igrad"),
                    (i_dw_part, "dw_part")):
        args = list(full)
        args[i] = None
        st, msg = _status("rn_field_bwd_merged_det", *args)
        assert st == 1 and what in msg, (i, st, msg)


def test_refusals_at_construction():
    with pytest.raises(ValueError, match="sub-NeRFs"):
        FusedMLRenderer(MNGP(0.5, size=9, seed=3), Ray_Gate(9, seed=4), 64, device=CPU,
                        capacity=4096, deterministic=True)
    m, g = MNGP(0.5, size=2, seed=3), Ray_Gate(2, seed=4)
    with pytest.raises(ValueError, match="PinnedMLRenderer"):
        PinnedMLRenderer(m, g, 64, device=CPU, capacity=4096, deterministic=True)
    # the per-model backward: not with the mode on, in either order
    r = FusedMLRenderer(m, g, 64, device=CPU, capacity=4096, deterministic=True)
    with pytest.raises(ValueError, match="merged backward"):
        r.merged_bwd = False
    assert r.merged_bwd and r.deterministic
    r = FusedMLRenderer(m, g, 64, device=CPU, capacity=4096)
    r.merged_bwd = False
    with pytest.raises(ValueError, match="merged backward"):
        r.deterministic = True
    assert not r.deterministic
    # the pinned layout still takes the flag's default
    assert PinnedMLRenderer(m, g, 64, device=CPU, capacity=4096).deterministic is False


@pytest.mark.parametrize("scale,K,B", [(0.5, 2, 1024), (16.0, 4, 512), (16.0, 8, 256),
                                       (0.5, 1, 256)])
def test_scatter_mode_and_default(scale, K, B):
    m, g = MNGP(scale, size=K, seed=3), Ray_Gate(K, seed=4)
    r0 = FusedMLRenderer(m, g, B, device=CPU, capacity=4096)
    r1 = FusedMLRenderer(m, g, B, device=CPU, capacity=4096, deterministic=True)
    assert r0.deterministic is False and r1.deterministic is True
    assert r1.scatter_mode == "int-grad"
    assert r0.scatter_mode in ("fixed-point", "binned", "fp32-atomics")
    # the flag moves none of the default switches
    for k in ("merged_bwd", "merged_fwd", "level_fwd", "merged_blocks", "max_chunk", "min_chunk",
              "head_chunk", "balance_chunks", "grid_fx", "grid_bin", "bin_f32_levels", "int_grad",
              "gate_bwd_at", "feat_cache"):
        assert getattr(r0, k) == getattr(r1, k), k
    assert inspect.signature(FusedMLRenderer.__init__).parameters["deterministic"].default is False
    assert inspect.signature(get_renderer).parameters["deterministic"].default is False


def test_trainer_passes_the_flag():
    m, g = MNGP(0.5, size=2, seed=3), Ray_Gate(2, seed=4)
    tr = Trainer(m, g, 64, deterministic=True)
    assert tr.renderer.deterministic is True and tr.deterministic is True
    assert tr.renderer.scatter_mode == "int-grad"
    assert inspect.signature(Trainer.__init__).parameters["deterministic"].default is False
    with pytest.raises(ValueError, match="sub-NeRFs"):
        Trainer(MNGP(0.5, size=9, seed=3), Ray_Gate(9, seed=4), 64, deterministic=True)
