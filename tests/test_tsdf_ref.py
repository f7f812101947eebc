"""CPU: the TSDF restatements (tests/tsdf_ref.py) and their scene, by
themselves -- what the GPU tests then hold the kernels to.

  * the scene keeps the exclusion rule's cap: at most 1 % of the lattice has a
    discrete decision within the margin of its boundary (fp64);
  * the fp32 and the fp64 restatement take the same decisions everywhere else;
  * the sphere the reference extracts is one closed component on the sphere,
    with no false shell behind the surface;
  * without carve, miss pixels leave their points unobserved;
  * with every point observed the valid-aware surface nets are
    mesh_ref.surface_nets.
"""
import numpy as np
import pytest

import mesh_clean_ref as MC
import mesh_ref as R
import tsdf_ref as T

KINDS = [False, True]                                  # directions as given / normalised


def _lat(sc, a):
    return a.reshape(sc.res[2] + 1, sc.res[1] + 1, sc.res[0] + 1)


@pytest.mark.parametrize("normalised", KINDS)
def test_scene_keeps_the_exclusion_cap(normalised):
    sc = T.scene(normalised)
    _, _, marginal = T.decisions64(sc)
    share = marginal.mean()
    print(f"marginal {int(marginal.sum())} of {sc.n_pts} ({100 * share:.2f} %)")
    assert share <= 0.01


@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("normalised", KINDS)
def test_fp32_and_fp64_decisions_agree(normalised, carve):
    sc = T.scene(normalised)
    _, code, pix = T.fused(normalised, carve)
    c64, p64, marginal = T.decisions64(sc, carve=carve)
    ok = ~marginal
    assert np.array_equal(code[:, ok], c64[:, ok])
    assert np.array_equal(pix[:, ok], p64[:, ok])
    # every branch is taken somewhere, by every kind of camera
    assert all((code == k).any() for k in (T.SKIP, T.HIT, T.HIT_COLOUR))
    assert (code == T.CARVE).any() == carve
    assert (code[T.SOFT_CAM] == T.HIT_COLOUR).any() and (code[5] == T.SKIP).any()
    assert (pix == -1).any()                            # outside an image / behind a camera


def test_observation_counts():
    """w and wc count the observations and the coloured ones"""
    vol, code, _ = T.fused()
    assert np.array_equal(vol["w"], (code != T.SKIP).sum(0).astype(np.float32))
    assert np.array_equal(vol["wc"], (code == T.HIT_COLOUR).sum(0).astype(np.float32))
    assert np.abs(vol["phi"]).max() <= 1.0
    assert vol["rgb"].min() >= 0.0 and vol["rgb"].max() <= 1.0


def test_batches_fold_as_one():
    """the reference itself: cameras folded in two calls are one call's bits"""
    sc = T.scene()
    vol = T.fresh(sc.n_pts)
    T.integrate(vol, sc, cams=[0, 1])
    T.integrate(vol, sc, cams=[2, 3, 4, 5])
    want = T.fused()[0]
    for k in want:
        assert np.array_equal(vol[k].view(np.int32), want[k].view(np.int32)), k


@pytest.mark.parametrize("normalised", KINDS)
def test_reference_sphere(normalised):
    """One closed component on the sphere.  The bars take the SMALLEST lattice
    step (1/24) for "one lattice step"."""
    sc = T.scene(normalised)
    vol = T.fused(normalised)[0]
    v, f, nr = T.surface_nets_valid(_lat(sc, vol["phi"]), _lat(sc, vol["w"]), 0.0, sc.lo, sc.step)
    assert len(v) > 500 and len(f) > 1000
    _, n_vertices, _ = MC.components(f, len(v))
    assert len(n_vertices) == 1
    chk = R.check_mesh(v, f)
    assert chk["closed"] and chk["volume"] > 0
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    step = float(sc.step.min())
    print(f"V {len(v)} mean|r - R| {np.abs(r - T.RADIUS).mean():.4f} max "
          f"{np.abs(r - T.RADIUS).max():.4f} step {step:.4f} trunc {sc.trunc}")
    assert np.abs(r - T.RADIUS).mean() <= step
    assert np.abs(r - T.RADIUS).max() <= sc.trunc
    # no false shell behind the surface
    assert r.min() >= T.RADIUS - step
    # normals point outwards
    assert (np.einsum("ij,ij->i", nr, v) > 0).mean() > 0.99


def test_unobserved_is_not_empty():
    """What the second rule is for: plain surface nets, reading an unobserved
    point's phi = 0 as a value, put surfaces where nobody looked"""
    sc = T.scene()
    vol = T.fused()[0]
    assert (vol["w"] == 0).any()
    v, _, _ = R.surface_nets(_lat(sc, vol["phi"]), 0.0, sc.lo, sc.step)
    r = np.linalg.norm(v, axis=1)
    assert np.abs(r - T.RADIUS).max() > sc.trunc


def test_no_carve_leaves_misses_unobserved():
    vol, code, _ = T.fused(carve=False)
    carved = T.fused(carve=True)
    assert not (code == T.CARVE).any()
    assert np.array_equal(vol["w"] > 0, (code >= T.HIT).any(0))
    only_missed = (carved[1] == T.CARVE).any(0) & ~(carved[1] >= T.HIT).any(0)
    assert only_missed.sum() > 1000
    assert (vol["w"][only_missed] == 0).all() and (carved[0]["w"][only_missed] > 0).all()
    assert (vol["phi"][only_missed] == 0).all()


@pytest.mark.parametrize("name", ["sphere24", "torus", "one_point", "empty", "half_space",
                                  "noise", "smooth"])
def test_all_valid_is_plain_surface_nets(name):
    lattices = {"sphere24": lambda: R.sphere(24) + (R.SPHERE_ISO,), "torus": lambda: R.torus() + (0.0,),
                "one_point": lambda: R.one_point() + (0.5,), "empty": lambda: R.empty() + (0.5,),
                "half_space": lambda: R.half_space() + (0.0,),
                "noise": lambda: R.noise() + (R.NOISE_ISO,), "smooth": lambda: R.smooth() + (0.0,)}
    s, lo, step, _, iso = lattices[name]()
    want = R.surface_nets(s, iso, lo, step)
    got = T.surface_nets_valid(s, np.ones_like(s), iso, lo, step)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def test_one_unobserved_point_opens_its_cells():
    """a single w = 0 point removes the vertices of its (up to) 8 cells and
    every quad that touches them, nothing else"""
    s, lo, step, _ = R.sphere(12)
    w = np.ones_like(s)
    full = R.surface_nets(s, R.SPHERE_ISO, lo, step)
    # the lattice point nearest a vertex of the surface
    at = np.rint((full[0][len(full[0]) // 2] - lo) / step).astype(int)
    w[at[2], at[1], at[0]] = 0
    v, f, _ = T.surface_nets_valid(s, w, R.SPHERE_ISO, lo, step)
    cell = np.floor((full[0] - lo) / step + 1e-4).astype(int)
    gone = (np.abs(cell + 0.5 - at[None, :]) < 1).all(1)
    assert 0 < gone.sum() <= 8 and len(v) == len(full[0]) - gone.sum()
    assert np.array_equal(v, full[0][~gone])
    quads = full[1].reshape(-1, 6)
    assert len(f) == 2 * int((~gone[quads].any(1)).sum())
    assert not R.check_mesh(v, f)["closed"]


def test_lattice_colors_restatement():
    """a constant colour lattice gives that colour whatever the weights; a
    vertex whose cell has no coloured corner is black; one coloured corner
    gives that corner's colour"""
    res = (3, 2, 2)
    lo, step = R.box_step((0, 0, 0), (3, 2, 2), res)
    n = 4 * 3 * 3
    rgb = np.tile(np.array([0.2, 0.5, 1.0], np.float32), (n, 1))
    wc = np.ones(n, np.float32)
    v = np.array([[0.3, 0.4, 0.5], [2.9, 1.9, 1.2], [3.0, 2.0, 2.0], [-1.0, 5.0, 0.5]], np.float32)
    got = T.lattice_colors(v, res, lo, step, rgb, wc)
    assert got.dtype == np.uint8 and np.abs(got.astype(int) - [51, 127, 255]).max() <= 1
    assert np.array_equal(T.lattice_colors(v, res, lo, step, rgb, 0 * wc), np.zeros((4, 3), np.uint8))
    wc1 = 0 * wc
    wc1[0] = 1
    rgb1 = rgb.copy()
    rgb1[0] = (1.0, 0.0, 0.25)
    got = T.lattice_colors(v[:1], res, lo, step, rgb1, wc1)
    assert np.array_equal(got, [[255, 0, 63]])
