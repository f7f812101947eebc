"""CPU: the surface of camera pose refinement (--optimize_ext;
tests/test_gpu_pose.py holds the GPU side).

  * rn_get_rays_pose / rn_get_rays_pose_bw are declared in the header and bound
    in _lib with the codes csrc/gen_sig.py derives from the header; the ABI
    version and rn_get_rays are what they were;
  * the argument checks of rays.pose_rays and trainer.Trainer that run before
    any device is touched.
"""
import importlib.util
import os
import re

import pytest
import torch

from radnerf_amd import _lib
from radnerf_amd.rays import pose_rays
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rn_get_rays_pose", "rn_get_rays_pose_bw")


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
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert sig[name] == table[name], name
    assert sig["rn_get_rays_pose"] == "pppppplppppp"
    assert sig["rn_get_rays_pose_bw"] == "pppppllppppppp"
    # every bound entry still equals the header's (nothing else moved)
    for name, codes in sig.items():
        assert table[name] == codes, name


def test_abi_version_and_get_rays_unchanged():
    hdr, table = _header_table()
    assert _lib.ABI_VERSION == 9
    assert re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    assert _lib.binding_signatures()["rn_get_rays"] == "pppplppppp" == table["rn_get_rays"]


def _cams(n_img=4, n_pix=20):
    g = torch.Generator().manual_seed(0)
    dirs = torch.rand(n_pix, 3, generator=g)
    poses = torch.rand(n_img, 3, 4, generator=g)
    return dirs, poses


def test_pose_rays_argument_checks():
    dirs, poses = _cams()
    z = torch.zeros(4, 3)
    img, pix = torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="dR must be"):
        pose_rays(dirs, poses, torch.zeros(3, 3), z, img, pix)
    with pytest.raises(ValueError, match="dT must be"):
        pose_rays(dirs, poses, z, torch.zeros(4), img, pix)
    with pytest.raises(ValueError, match="poses must be"):
        pose_rays(dirs, poses[0], z, z, img, pix)
    with pytest.raises(ValueError, match="directions must be"):
        pose_rays(dirs[:, :2], poses, z, z, img, pix)
    with pytest.raises(ValueError, match="integer"):
        pose_rays(dirs, poses, z, z, img.float(), pix)
    with pytest.raises(ValueError, match="img_idxs vs"):
        pose_rays(dirs, poses, z, z, img, pix[:4])


def test_pose_parameters_ride_the_flat_buffer():
    """dR / dT appended after the gate: dist.step_ranges' three ranges still
    tile the buffer, [grid, MLP, gate] keep their offsets, and the pose
    gradients lie in "rest" (the collective of the MLP and gate gradients)."""
    from radnerf_amd import dist as rdist
    from radnerf_amd import layout as LY
    lv, K, N = LY.grid_levels(0.5), 2, 7
    n_grid = 2 * int(lv["n_entries"])
    net = [torch.zeros(n_grid), torch.zeros(K, LY.FIELD_PARAMS), torch.zeros(LY.gate_params(K))]
    ar3 = rdist.GradAllReduce(net, "cpu")
    ar5 = rdist.GradAllReduce(net + [torch.zeros(N, 3), torch.zeros(N, 3)], "cpu")
    assert ar5.flat.numel() == ar3.flat.numel() + 6 * N
    for i in range(3):
        assert ar5.param_range(i, i + 1) == ar3.param_range(i, i + 1)
    for split in (0, 8, 15):
        r3 = rdist.step_ranges(ar3, lv["offset"], split)
        r5 = rdist.step_ranges(ar5, lv["offset"], split)
        assert r5["fine"] == r3["fine"] and r5["coarse"] == r3["coarse"]
        assert r5["rest"] == (r3["rest"][0], r3["rest"][1] + 6 * N)
        seen = torch.zeros(ar5.flat.numel(), dtype=torch.int32)
        for a, b in r5.values():
            seen[a:b] += 1
        assert bool((seen == 1).all())
    assert ar5.views[3].shape == (N, 3) and ar5.views[4].shape == (N, 3)
    ar5.views[4].fill_(1.0)
    assert float(ar5.flat[-3 * N:].sum()) == 3 * N and float(ar5.flat[:-3 * N].abs().sum()) == 0


def test_trainer_argument_checks():
    dirs, poses = _cams()
    # raised before the model is looked at: no device, no renderer
    with pytest.raises(ValueError, match="optimize_ext=True"):
        Trainer(None, None, 64, optimize_ext=True)
    with pytest.raises(ValueError, match="optimize_ext=True"):
        Trainer(None, None, 64, optimize_ext=True, directions=dirs)
    with pytest.raises(ValueError, match="together"):
        Trainer(None, None, 64, poses=poses)
    import inspect
    p = inspect.signature(Trainer.__init__).parameters
    assert p["optimize_ext"].default is False and p["pose_lr"].default == 1e-8
    assert p["directions"].default is None and p["poses"].default is None
