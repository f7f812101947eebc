"""CPU: the surface of the mesh export (tests/test_gpu_mesh.py holds the GPU
side): the argument checks of mesh.density_lattice / surface_nets, which run
before the library is loaded; PLY and OBJ round trips of a hand-made mesh; the
new entries declared in the header and bound in _lib under ABI 9.
"""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from radnerf_amd import _lib, mesh
from radnerf_amd.networks import MNGP, NGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_density_lattice": "iiipppipppppppppp", "rn_surface_work_bytes": "iiip",
       "rn_surface_count": "piiifpp", "rn_surface_emit": "piiifpppllpppp"}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (mesh, _lib):
        monkeypatch.setattr(mod, "lib", boom)


@pytest.fixture(scope="module")
def model():
    return MNGP(0.5, size=3, t=12, seed=1)


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
    assert "mesh.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("res", [0, -3, (4, 4), (4, 0, 4), 2.5, (4, 4, 4.0), "8"])
def test_bad_resolution(no_library, model, res):
    with pytest.raises(ValueError, match="resolution"):
        mesh.density_lattice(model, res)


def test_too_many_points(no_library, model):
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.density_lattice(model, 1290)                  # 1291^3 > 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.density_lattice(model, (1 << 20, 1 << 10, 1))
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.extract_mesh(model, resolution=2048)


@pytest.mark.parametrize("aabb", [((-0.6, -0.5, -0.5), (0.5, 0.5, 0.5)),
                                  ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5001)),
                                  ((0.1, 0.1, 0.1), (0.1, 0.2, 0.2)),
                                  ((0.2, 0.1, 0.1), (0.1, 0.2, 0.2)),
                                  ((0.0, 0.0, float("nan")), (0.1, 0.2, 0.2)),
                                  ((0.0, 0.0), (0.1, 0.2)), "box", 0.5])
def test_bad_box(no_library, model, aabb):
    with pytest.raises(ValueError, match="aabb"):
        mesh.density_lattice(model, 4, aabb=aabb)


@pytest.mark.parametrize("w", [[1.0, 0.0], [0.25] * 4, [[1.0, 0.0, 0.0]],
                               torch.ones(2), [1.0, float("inf"), 0.0]])
def test_bad_weights(no_library, model, w):
    with pytest.raises(ValueError, match="weights"):
        mesh.density_lattice(model, 4, weights=w)


def test_ngp_takes_one_weight(no_library):
    with pytest.raises(ValueError, match=r"\(1,\)"):
        mesh.density_lattice(NGP(0.5, t=12, seed=1), 4, weights=[0.5, 0.5])


def test_cpu_model_and_lattice_are_refused(no_library, model):
    with pytest.raises(ValueError, match="GPU"):
        mesh.density_lattice(model, 4)
    with pytest.raises(ValueError, match="GPU"):
        mesh.surface_nets(torch.zeros(3, 4, 5), 0.5, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="float32"):
        mesh.surface_nets(torch.zeros(3, 4, 5, dtype=torch.float64), 0.5, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="resolution"):
        mesh.surface_nets(torch.zeros(1, 4, 5), 0.5, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="contiguous"):
        mesh.surface_nets(torch.zeros(5, 4, 3).permute(2, 1, 0), 0.5, ((0, 0, 0), (1, 1, 1)))


def test_default_iso_is_the_training_threshold():
    from radnerf_amd import trainer
    assert mesh.DEFAULT_ISO == 0.01 * trainer.MAX_SAMPLES / 3 ** 0.5


def _hand_made(normals, colors):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1 / 3, -2.5e-7, 3e8]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    n = np.array([[-1, -1, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], np.float32)
    n[0] /= np.float32(np.sqrt(3))
    c = np.array([[0, 1, 2], [255, 254, 253], [17, 128, 200], [9, 9, 9], [1, 0, 255]], np.uint8)
    t = torch.from_numpy
    return mesh.Mesh(t(v), t(f), t(n) if normals else None, t(c) if colors else None)


def _same(a, b):
    assert torch.equal(a.vertices, b.vertices) and a.vertices.dtype == torch.float32
    assert torch.equal(a.faces, b.faces) and a.faces.dtype == torch.int32
    for x, y in ((a.normals, b.normals), (a.colors, b.colors)):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y) and x.dtype == y.dtype


@pytest.mark.parametrize("normals,colors", [(False, False), (True, False), (False, True),
                                            (True, True)])
def test_ply_and_obj_round_trip(tmp_path, normals, colors):
    m = _hand_made(normals, colors)
    p = str(tmp_path / "m.ply")
    assert m.save(p) == p
    head = open(p, "rb").read(4096).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
    assert ("property float nx" in head) == normals and ("property uchar red" in head) == colors
    assert "property list uchar int vertex_indices" in head and "element face 4" in head
    size = 3 * 4 + (12 if normals else 0) + (3 if colors else 0)
    assert head[-1] == ""                                  # the header's lines end in "\n"
    assert os.path.getsize(p) == len("\n".join(head)) + len("end_header\n") + 5 * size + 4 * 13
    _same(mesh.load_ply(p), m)
    o = str(tmp_path / "m.obj")
    m.save(o)
    _same(mesh.load_obj(o), m)


def test_empty_mesh_round_trip(tmp_path):
    m = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3))
    _same(mesh.load_ply(m.save(str(tmp_path / "e.ply"))), m)


def test_save_refuses_other_names_and_load_refuses_other_files(tmp_path):
    m = _hand_made(True, False)
    with pytest.raises(ValueError, match="ply or .obj"):
        m.save(str(tmp_path / "m.stl"))
    p = str(tmp_path / "m.ply")
    m.save(p)
    data = open(p, "rb").read()
    open(p, "wb").write(data[:-5])
    with pytest.raises(ValueError, match="truncated"):
        mesh.load_ply(p)
    open(p, "wb").write(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        mesh.load_ply(p)


def test_trainer_has_export_mesh():
    from radnerf_amd.trainer import Trainer
    assert callable(Trainer.export_mesh)
