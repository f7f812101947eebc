"""CPU: the surface of the mesh clean-up (tests/test_gpu_mesh_clean.py holds
the GPU side): the argument checks of mesh.components / filter_components /
density_lattice(occupancy=True) / extract_mesh, which run before the library
is loaded and need no GPU, and the new entries declared in the header and
bound in _lib under ABI 9.
"""
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch

from radnerf_amd import _lib, mesh
from radnerf_amd.networks import MNGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_density_lattice_masked": "iiipppipppppppppiifpp", "rn_mesh_work_bytes": "llp",
       "rn_mesh_label": "pllppiip", "rn_mesh_components": "pllpplpppp",
       "rn_mesh_compact_count": "pllpplpp", "rn_mesh_compact_emit": "pllppppllppppp"}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (mesh, _lib):
        monkeypatch.setattr(mod, "lib", boom)


@pytest.fixture(scope="module")
def model():
    return MNGP(0.5, size=2, t=12, seed=1)


def _tri(faces=None, **kw):
    v = torch.zeros(4, 3)
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32) if faces is None else faces
    return mesh.Mesh(v, f, **kw)


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
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    assert "mesh_clean.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()


def test_no_criterion(no_library, model):
    with pytest.raises(ValueError, match="keep_largest, min_vertices or min_fraction"):
        mesh.filter_components(_tri())


@pytest.mark.parametrize("kw", [dict(keep_largest=0), dict(keep_largest=-2),
                                dict(keep_largest=1.5), dict(keep_largest=True),
                                dict(min_vertices=-1), dict(min_vertices=2.0),
                                dict(min_fraction=-0.01), dict(min_fraction=1.01),
                                dict(min_fraction=float("nan")), dict(min_fraction="half"),
                                dict(keep_largest=1, min_fraction=2.0)])
def test_bad_criteria(no_library, model, kw):
    name = "min_fraction" if "min_fraction" in kw else next(iter(kw))
    with pytest.raises(ValueError, match=name):
        mesh.filter_components(_tri(), **kw)
    # extract_mesh refuses them before it evaluates a lattice
    with pytest.raises(ValueError, match=name):
        mesh.extract_mesh(model, resolution=4, **kw)


@pytest.mark.parametrize("faces", [torch.zeros(2, 3, dtype=torch.int64),
                                   torch.zeros(2, 4, dtype=torch.int32),
                                   torch.zeros(6, dtype=torch.int32),
                                   torch.zeros(2, 3), np.zeros((2, 3), np.int32), None])
def test_bad_faces(no_library, faces):
    m = _tri()
    m.faces = faces
    for call in (mesh.components, lambda x: mesh.filter_components(x, keep_largest=1)):
        with pytest.raises(ValueError, match=r"\(F, 3\) int32"):
            call(m)


def test_bad_mesh(no_library):
    with pytest.raises(ValueError, match="contiguous"):
        mesh.components(_tri(torch.zeros(3, 2, dtype=torch.int32).t()))
    with pytest.raises(ValueError, match="vertices"):
        mesh.components(mesh.Mesh(torch.zeros(4, 3, dtype=torch.float64), _tri().faces))
    with pytest.raises(ValueError, match="normals"):
        mesh.components(_tri(normals=torch.zeros(3, 3)))
    with pytest.raises(ValueError, match="colors"):
        mesh.filter_components(_tri(colors=torch.zeros(4, 3)), keep_largest=1)
    with pytest.raises(ValueError, match="GPU"):
        mesh.components(_tri())
    with pytest.raises(ValueError, match="GPU"):
        mesh.filter_components(_tri(), min_vertices=1)


def test_occupancy_needs_bitfields(no_library, model):
    bare = types.SimpleNamespace(size=1, _h_min=np.full(3, -0.5, np.float32),
                                 _h_ext=np.ones(3, np.float32))
    with pytest.raises(ValueError, match="density_bitfield"):
        mesh.density_lattice(bare, 4, occupancy=True)
    with pytest.raises(ValueError, match="density_bitfield"):
        mesh.extract_mesh(bare, resolution=4, occupancy=True)
    # a bitfield of another size than cascades * grid_size^3 / 8
    odd = MNGP(0.5, size=2, t=12, seed=1)
    odd.density_bitfield_1 = odd.density_bitfield_1[:-1]
    with pytest.raises(ValueError, match="density_bitfield_1"):
        mesh.density_lattice(odd, 4, occupancy=True)
    # with bitfields the next check is the device's
    with pytest.raises(ValueError, match="GPU"):
        mesh.density_lattice(model, 4, occupancy=True)


def test_label_bounds_are_stated():
    assert mesh.LABEL_ROUNDS == 12 and mesh.LABEL_BATCHES == 16
