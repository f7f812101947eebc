"""CPU: camera-visibility culling of the occupancy grids and the erode decay
(tests/test_gpu_visibility.py holds the GPU side).

  * the numpy restatement of rn_mark_invisible_cells (tests/visibility_ref.py,
    written from the header comment) gives, on the six-camera rig, the valid
    shares and too-near counts worked out when the rig was designed; its fp32
    and fp64 forms differ in at most 4 cells, all inside the edge band (cells
    with a comparison closer than 1e-5 of its terms), and the band holds at
    most 1e-3 of the cells;
  * a hand case: one camera at (0, 0, -2) looking along +z;
  * the argument checks of MNGP.mark_invisible_cells, update_density_grid(
    erode=True) and Trainer(cull_invisible=True) run before the library is
    loaded;
  * rn_mark_invisible_cells and rn_density_update_visible are declared, bound
    and generated with the same codes, the ABI version stays, and their own
    argument checks return status 1 without a device.
"""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import visibility_ref as V
from radnerf_amd import _lib, networks
from radnerf_amd import dist as rdist
from radnerf_amd.networks import MNGP, NGP
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK_CODES = "piffffiifppiiifppp"
UPD_CODES = "ppiiifffupppppppppppppi"     # rn_density_update_sampled less its stream


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (networks, _lib):
        monkeypatch.setattr(mod, "lib", boom)


# ---- the restatement on the rig ---------------------------------------------
@pytest.mark.parametrize("scale,shares,too_near,max_diff", [
    (0.5, [0.679], [146], 0),
    (4.0, [1.000, 1.000, 0.971, 0.692], [146, 21, 3, 0], 1),
])
def test_rig_shares_and_edge_band(scale, shares, too_near, max_diff):
    a = V.rig_mark(scale, 0.06, np.float32)
    b = V.rig_mark(scale, 0.06, np.float64, band_eps=1e-5)
    for r in (a, b):
        got = r["valid"].mean(1)
        print(f"scale {scale}: valid share per cascade {np.round(got, 4)}, too near "
              f"{r['too_near'].sum(1)}, culled {r['n_culled']}")
        assert np.all(np.abs(got - np.array(shares)) < 5e-4), got
        assert r["too_near"].sum(1).tolist() == too_near
        assert np.array_equal(r["n_culled"], V.G3 - r["valid"].sum(1))
    diff = (a["n_covered"] != b["n_covered"]) | (a["too_near"] != b["too_near"]) \
        | (a["valid"] != b["valid"])
    band = float(b["band"].mean())
    print(f"scale {scale}: fp32 vs fp64 differ in {int(diff.sum())} cells, "
          f"{int((diff & ~b['band']).sum())} outside the edge band; band share {band:.2e}")
    assert band <= 1e-3                         # the condition the cell bound rests on
    assert not (diff & ~b["band"]).any()
    assert diff.sum() <= 4 and diff.sum() == max_diff
    # the count is the covered share, rounded once
    assert a["count"].dtype == np.float32
    assert np.array_equal(a["count"], a["n_covered"].astype(np.float32) / np.float32(6))


@pytest.mark.parametrize("scale", [0.5, 4.0])
def test_rig_default_near_has_no_too_near_cell(scale):
    a = V.rig_mark(scale, 0.01, np.float32)
    assert a["too_near"].sum() == 0
    # nothing is valid at 0.06 that 0.01 culls, and the 0.06 cull is larger
    b = V.rig_mark(scale, 0.06, np.float32)
    assert not (b["valid"] & ~a["valid"]).any()
    assert int(b["n_culled"].sum()) > int(a["n_culled"].sum())


def test_hand_case_one_camera():
    # right / down / front = x / y / z, eye at (0, 0, -2)
    pose = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -2]]], np.float32)
    scale = 4.0
    cells = np.array([[64, 64, 64],      # next to the origin
                      [64, 64, 0],       # cascade 3: z = -3.97, behind the camera
                      [127, 64, 64]])    # cascade 3: x = 3.97 at depth 2, off the image
    for dtype in (np.float32, np.float64):
        for c, want in ((0, [1, 1, 1]), (3, [1, 0, 0])):
            X = V.cell_centres(cells, c, scale, dtype)
            n_cov, near = V.classify(X, pose, V.INTRINSICS, V.IMG_WH, 0.01, dtype)
            assert n_cov.tolist() == want and not near.any(), (c, dtype)
        # the centre cell of cascade 0: x = y = z = (64/127*2 - 1) * (0.5 - 0.5/128)
        X = V.cell_centres(cells[:1], 0, scale, dtype)
        assert abs(float(X[0, 0]) - (64 / 127 * 2 - 1) * (0.5 - 0.5 / 128)) < 1e-7
        # a near plane beyond it makes it too near instead of covered
        n_cov, near = V.classify(X, pose, V.INTRINSICS, V.IMG_WH, 2.5, dtype)
        assert n_cov.tolist() == [0] and near.tolist() == [True]
    # Morton order: cell m of the grid has the coordinates of its de-interleaved bits
    assert V.morton_coords([0, 1, 2, 4, 7, 8, V.G3 - 1]).tolist() == [
        [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 0, 0], [127, 127, 127]]
    # look_at: right / down / front are orthonormal, z up means down has z < 0
    P = V.look_at((3.0, 1.0, 0.5), (0.0, 0.0, 0.0))
    assert np.allclose(P[:, :3].T @ P[:, :3], np.eye(3), atol=1e-12) and P[2, 1] < 0
    assert np.allclose(np.cross(P[:, 0], P[:, 1]), P[:, 2], atol=1e-12)
    g, bits = V.apply_mark(np.array([[-2.0, 0.0, 3.0, -1.0, 5.0, 0.5, -0.5, 1.0]], np.float32),
                           np.array([0xff], np.uint8),
                           np.array([[1, 1, 1, 1, 0, 0, 0, 1]], bool))
    assert g.tolist() == [[0, 0, 3, 0, -1, -1, -1, 1]] and bits.tolist() == [0b10001111]


# ---- argument checks --------------------------------------------------------
def test_mark_argument_checks(no_library):
    m = MNGP(0.5, size=2, seed=1)
    poses = torch.from_numpy(V.rig_poses(0.5))
    K = torch.from_numpy(V.INTRINSICS)
    with pytest.raises(ValueError, match="K must be a 3x3"):
        m.mark_invisible_cells(np.eye(4), poses, V.IMG_WH)
    with pytest.raises(ValueError, match="poses must be a tensor"):
        m.mark_invisible_cells(K, poses.numpy(), V.IMG_WH)
    with pytest.raises(ValueError, match=r"poses must be \(N, 3, 4\)"):
        m.mark_invisible_cells(K, poses[:, :, :3], V.IMG_WH)
    with pytest.raises(ValueError, match="at least one camera"):
        m.mark_invisible_cells(K, poses[:0], V.IMG_WH)
    with pytest.raises(ValueError, match="poses must be float32"):
        m.mark_invisible_cells(K, poses.double(), V.IMG_WH)
    with pytest.raises(ValueError, match=r"img_wh must be \(W, H\)"):
        m.mark_invisible_cells(K, poses, 64)
    with pytest.raises(ValueError, match="img_wh must be positive"):
        m.mark_invisible_cells(K, poses, (64, 0))
    # host tensors are refused by name, never handed to a kernel
    with pytest.raises(ValueError, match="must be on the GPU"):
        m.mark_invisible_cells(V.INTRINSICS, poses, V.IMG_WH)
    with pytest.raises(ValueError, match="poses are on"):
        m.mark_invisible_cells(K, poses.to("meta"), V.IMG_WH)
    p = inspect.signature(MNGP.mark_invisible_cells).parameters
    assert list(p) == ["self", "K", "poses", "img_wh", "near_distance"]
    assert p["near_distance"].default == 0.01
    assert NGP.mark_invisible_cells is MNGP.mark_invisible_cells
    # count_grid is no buffer: the reference state_dict key set is unchanged
    assert getattr(m, "count_grid", None) is None
    assert not any("count" in k for k in m.state_dict())


def test_erode_needs_a_mark(no_library):
    for m in (MNGP(0.5, size=2, seed=1), NGP(0.5, seed=1)):
        with pytest.raises(ValueError, match="call mark_invisible_cells"):
            m.update_density_grid(1.0, erode=True, seed=3)
        with pytest.raises(ValueError, match="call mark_invisible_cells"):
            m.update_density_grid(1.0, warmup=True, erode=True, seed=3)
        with pytest.raises(ValueError, match="call mark_invisible_cells"):
            rdist.update_density_grid(m, 1.0, 16, erode=True)
    p = inspect.signature(rdist.update_density_grid).parameters
    assert p["erode"].default is False
    # register_bbox drops the cull of the old box
    m.count_grid = torch.ones(1, 8)
    m.register_bbox(np.array([[-1, -1, -1], [1, 1, 1]], np.float32))
    assert m.count_grid is None


def test_trainer_cull_argument_checks(no_library):
    p = inspect.signature(Trainer.__init__).parameters
    assert p["intrinsics"].default is None
    assert p["cull_invisible"].default is False and p["erode"].default is False
    d, poses = torch.rand(64 * 48, 3), torch.from_numpy(V.rig_poses(0.5))
    # raised before the model is looked at
    for kw in (dict(), dict(intrinsics=V.INTRINSICS), dict(directions=d, poses=poses),
               dict(directions=d, poses=poses, intrinsics=V.INTRINSICS),
               dict(directions=d, poses=poses, img_wh=V.IMG_WH)):
        with pytest.raises(ValueError, match=r"cull_invisible=True\) needs intrinsics"):
            Trainer(None, None, 64, cull_invisible=True, **kw)
    with pytest.raises(ValueError, match=r"erode=True\) needs cull_invisible"):
        Trainer(None, None, 64, erode=True)


# ---- the C entries ----------------------------------------------------------
def test_entries_declared_and_bound():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    table = _lib.parse_signature_table(gs.table(hdr))
    for name, codes in (("rn_mark_invisible_cells", MARK_CODES),
                        ("rn_density_update_visible", UPD_CODES + "pip")):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert _lib.binding_signatures()[name] == table[name] == codes
    # the new update entry takes the old one's arguments plus count_grid and erode
    assert table["rn_density_update_sampled"] == UPD_CODES + "p"
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    # the header states the operation order this file's restatement was written from
    for s in ("xc = (R[0][0]*d_0 + R[1][0]*d_1) + R[2][0]*d_2", "px = fx*xc + cx*zc",
              "in_image = zc > 0 && px >= 0 && px < W*zc && py >= 0 && py < H*zc",
              "X_a = ((i_a / (G-1)) * 2 - 1) * (sc - hgs)",
              "(float)n_covered / (float)n_cams",
              "clamp(powf(decay, 1.0f / count), 0.1f, 0.95f)"):
        assert s in hdr, s
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "L.rn_mark_invisible_cells.argtypes" in doc


def _mark(**kw):
    """rn_mark_invisible_cells with valid sizes and no pointer, `kw` replacing arguments"""
    a = dict(poses=None, n_cams=6, fx=100.0, fy=100.0, cx=32.0, cy=24.0, width=64, height=48,
             near=0.01, grid_ptrs=None, bitfield_ptrs=None, n_models=2, cascades=1,
             grid_size=128, scale=0.5, count_grid=None, n_culled=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.lib().mark_invisible_cells(*a.values())


@pytest.mark.parametrize("kw,msg", [
    (dict(n_cams=0), "needs a camera"),
    (dict(n_cams=-1), "needs a camera"),
    (dict(width=0), "positive image size"),
    (dict(height=-3), "positive image size"),
    (dict(n_models=0), "bad sizes"),
    (dict(cascades=0), "bad sizes"),
    (dict(cascades=33), "bad sizes"),
    (dict(grid_size=64), "bad sizes"),
    (dict(), "null pointer"),
    # never dereferenced: the check of the others comes first
    (dict(poses=64, grid_ptrs=64, bitfield_ptrs=64), "null pointer"),
    (dict(poses=64, grid_ptrs=64, count_grid=64), "null pointer"),
])
def test_mark_entry_argument_checks_without_gpu(kw, msg):
    with pytest.raises(RuntimeError, match=r"rn_mark_invisible_cells failed \(status 1\).*" + msg):
        _mark(**kw)


def _update(**kw):
    """rn_density_update_visible with valid sizes and no pointer"""
    a = dict(grid_ptrs=None, bitfield_ptrs=None, n_models=2, cascades=1, grid_size=128,
             scale=0.5, thr=1.0, decay=0.95, seed=1, grid_f16=None, level_offset=None,
             level_hsize=None, level_res=None, level_scale=None, xyz_min=None, extent=None,
             frags=None, tmp=None, occ=None, blk=None, part=None, thr_out=None, all_cells=0,
             count_grid=None, erode=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.lib().density_update_visible(*a.values())


_PTRS = dict.fromkeys(("grid_ptrs", "bitfield_ptrs", "grid_f16", "level_offset", "level_hsize",
                       "level_res", "level_scale", "xyz_min", "extent", "frags", "tmp", "occ",
                       "blk", "part", "thr_out"), 64)


@pytest.mark.parametrize("kw,msg", [
    (dict(n_models=0), "bad sizes"),
    (dict(cascades=33), "bad sizes"),
    (dict(grid_size=256), "bad sizes"),
    (dict(), "null pointer"),
    (dict(count_grid=64, erode=1), "null pointer"),
    (dict(_PTRS, thr_out=None), "null pointer"),
    # never dereferenced: erode without a count_grid is refused first
    (dict(_PTRS, erode=1), "erode needs count_grid"),
])
def test_update_entry_argument_checks_without_gpu(kw, msg):
    with pytest.raises(RuntimeError,
                       match=r"rn_density_update_visible failed \(status 1\).*" + msg):
        _update(**kw)
