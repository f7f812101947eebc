"""CPU: the argument checks of the TSDF export (radnerf_amd/tsdf.py,
Trainer.export_mesh(method="tsdf")) and the four C entries' declarations.
Every ValueError comes before the library is touched and before anything is
allocated on a device.
"""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from radnerf_amd import _lib, evaluate, mesh, tsdf
from radnerf_amd.trainer import Trainer

from test_train_state_api import _trainer as _cpu_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_tsdf_integrate": "iiipppiffffiippppfffippppp",
       "rn_surface_count_valid": "ppiiifpp",
       "rn_surface_emit_valid": "ppiiifpppllpppp",
       "rn_lattice_colors": "pliiipppppp"}
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
K3 = np.array([[30.0, 0, 19.37], [0, 30.0, 15.71], [0, 0, 1]])


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (tsdf, mesh, evaluate, _lib):
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
    # additive under the current ABI number
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    mk = open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()
    assert "tsdf.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()


def test_defaults_keep_the_density_export():
    p = inspect.signature(Trainer.export_mesh).parameters
    assert p["method"].default == "density" and p["poses"].default is None
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in p.values())
    f = inspect.signature(tsdf.fuse_mesh).parameters
    want = dict(resolution=256, aabb=None, trunc=None, colors=True, batch=8, keep_largest=None,
                min_vertices=None, min_fraction=None, gate_min=0.0, gate_topk=None,
                renormalize=False)
    assert {k: f[k].default for k in want} == want
    i = inspect.signature(tsdf.TSDFVolume.integrate).parameters
    assert i["opacity_min"].default == 0.5 and i["carve"].default is True
    assert i["rgb"].default is None and i["near"].default == 0.01


@pytest.mark.parametrize("kw,msg", [
    (dict(resolution=0), "resolution"),
    (dict(resolution=(4, 4)), "resolution"),
    (dict(resolution=(2047, 2047, 2047)), r"2\^31"),
    (dict(aabb=((0, 0, 0), (1, 1, 0))), "aabb"),
    (dict(aabb=(0, 1)), "aabb"),
    (dict(trunc=0.1), "sqrt"),                    # sqrt(3) / 16 = 0.108 is the floor
    (dict(trunc=float("nan")), "sqrt"),
    (dict(trunc="wide"), "trunc"),
    (dict(device="cpu"), "GPU"),
])
def test_volume_refuses(no_library, kw, msg):
    args = dict(resolution=(24, 20, 16), aabb=BOX)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        tsdf.TSDFVolume(**args)


def _bare_volume(colors=True):
    """a volume's host side without its device tensors: integrate's checks
    come before it reads them"""
    vol = tsdf.TSDFVolume.__new__(tsdf.TSDFVolume)
    vol.res = (24, 20, 16)
    vol.lo, vol.step = mesh._box("t", BOX, vol.res)
    vol.trunc, vol.device = 0.25, torch.device("cpu")
    vol.phi = vol.w = torch.zeros(1)
    vol.rgb = vol.wc = torch.zeros(1) if colors else None
    return vol


def _images(n=2, N=40 * 32):
    return dict(depth=torch.zeros(n, N), opacity=torch.zeros(n, N), poses=torch.zeros(n, 3, 4),
                intrinsics=K3, directions=torch.zeros(N, 3), img_wh=(40, 32))


@pytest.mark.parametrize("kw,msg", [
    (dict(img_wh=(40,)), "img_wh"),
    (dict(img_wh=(0, 32)), "img_wh"),
    (dict(intrinsics=np.eye(4)), "intrinsics"),
    (dict(intrinsics=np.diag([0.0, 30.0, 1.0])), "intrinsics"),
    (dict(near=-1.0), "near"),
    (dict(opacity_min=0.0), "opacity_min"),
    (dict(opacity_min=1.5), "opacity_min"),
    (dict(poses=torch.zeros(2, 4, 4)), "poses"),
    (dict(poses=torch.zeros(2, 3, 4, dtype=torch.float64)), "poses"),
    (dict(depth=torch.zeros(2, 40 * 32 + 1)), "depth"),
    (dict(opacity=torch.zeros(3, 40 * 32)), "opacity"),
    (dict(opacity=torch.zeros(2, 40 * 32, dtype=torch.float16)), "opacity"),
    (dict(directions=torch.zeros(40 * 32, 4)), "directions"),
    (dict(depth=torch.zeros(40 * 32, 2).t()), "depth"),
    (dict(rgb=torch.zeros(2, 40 * 32)), "rgb"),
    (dict(depth=np.zeros((2, 40 * 32), np.float32)), "depth"),
])
def test_integrate_refuses(no_library, kw, msg):
    args = _images()
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        _bare_volume().integrate(**args)


def test_integrate_refuses_colours_without_a_colour_lattice(no_library):
    with pytest.raises(ValueError, match="colors=False"):
        _bare_volume(colors=False).integrate(rgb=torch.zeros(2, 40 * 32, 3), **_images())


def test_integrate_refuses_another_device(no_library):
    vol = _bare_volume()
    vol.device = torch.device("meta")
    with pytest.raises(ValueError, match="is on cpu"):
        vol.integrate(**_images())


@pytest.mark.parametrize("kw,msg", [
    (dict(keep_largest=0), "keep_largest"),
    (dict(min_fraction=2.0), "min_fraction"),
    (dict(img_wh=(40, 32, 1)), "img_wh"),
    (dict(intrinsics=None), "intrinsics"),
    (dict(opacity_min=-0.1), "opacity_min"),
    (dict(poses=torch.zeros(3, 4)), "poses"),
    (dict(batch=0), "batch"),
    (dict(batch=2.5), "batch"),
    (dict(resolution=-3), "resolution"),
    (dict(aabb=((0, 0, 0), (0, 1, 1))), "aabb"),
    (dict(directions=torch.zeros(7, 3)), "directions"),
    (dict(aabb=BOX, trunc=1e-3), "sqrt"),
])
def test_fuse_mesh_refuses(no_library, kw, msg):
    tr = _cpu_trainer(ext=False, filled=False)
    args = dict(poses=torch.zeros(2, 3, 4), directions=torch.zeros(40 * 32, 3), img_wh=(40, 32),
                intrinsics=K3, resolution=16)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        tsdf.fuse_mesh(tr.model, tr.gate, **args)


def test_trainer_export_mesh_names_what_is_missing(no_library, tmp_path):
    p = str(tmp_path / "m.ply")
    full = dict(directions=torch.zeros(40 * 32, 3), poses=torch.zeros(2, 3, 4), img_wh=(40, 32),
                intrinsics=K3)
    for drop in ("intrinsics", "poses", "img_wh", "directions"):
        tr = _cpu_trainer(ext=False, filled=False, **dict(full, **{drop: None}))
        with pytest.raises(ValueError, match=drop):
            tr.export_mesh(p, method="tsdf")
    tr = _cpu_trainer(ext=False, filled=False, **dict(full, intrinsics=None, img_wh=None))
    with pytest.raises(ValueError, match=r"img_wh=\.\.\., intrinsics=\.\.\."):
        tr.export_mesh(p, method="tsdf")
    # poses given by the call stand in for the trainer's
    tr = _cpu_trainer(ext=False, filled=False, **dict(full, poses=None, intrinsics=None))
    with pytest.raises(ValueError) as e:
        tr.export_mesh(p, method="tsdf", poses=torch.zeros(1, 3, 4))
    assert "intrinsics" in str(e.value) and "poses" not in str(e.value)
    assert not os.path.exists(p)


def test_trainer_export_mesh_refuses_unknown_method(no_library, tmp_path):
    tr = _cpu_trainer(ext=False, filled=False, intrinsics=K3)
    with pytest.raises(ValueError, match="method"):
        tr.export_mesh(str(tmp_path / "m.ply"), method="marching_cubes")
    with pytest.raises(ValueError, match="poses"):
        tr.export_mesh(str(tmp_path / "m.ply"), poses=torch.zeros(1, 3, 4))
