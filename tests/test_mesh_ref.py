"""CPU: the numpy surface-nets reference (tests/mesh_ref.py) on analytic
lattices -- the counts, and the topological facts that may not move: closed
where the surface stays inside the box, the Euler characteristic, every
directed edge once, positive volume (normals from dense to empty).
tests/test_gpu_mesh.py compares the kernels with this reference index for index.
"""
import numpy as np
import pytest

import mesh_ref as R


@pytest.mark.parametrize("n,n_v,n_f", [(8, 110, 216), (16, 438, 872), (24, 976, 1948),
                                       (33, 1852, 3700)])
def test_sphere(n, n_v, n_f):
    s, lo, step, _ = R.sphere(n)
    v, f, nr = R.surface_nets(s, R.SPHERE_ISO, lo, step)
    chk = R.check_mesh(v, f)
    assert chk["edges_once"] and chk["closed"] and chk["euler"] == 2 and chk["volume"] > 0, chk
    # the lattice values are formed in fp32 here: the counts may move by a few
    assert abs(len(v) - n_v) <= 4 and abs(len(f) - n_f) <= 8, (len(v), len(f))
    assert len(f) == 2 * len(v) - 4                        # chi = 2, triangles
    rel = v.astype(np.float64) - np.asarray(R.SPHERE_C)
    r = np.linalg.norm(rel, axis=1)
    assert np.abs(r - R.SPHERE_R).max() <= 0.5 * float(step[0]), np.abs(r - R.SPHERE_R).max()
    # normals: unit, pointing away from the dense centre
    assert np.abs(np.linalg.norm(nr, axis=1) - 1).max() < 1e-5
    assert ((nr * rel).sum(1) / r).min() > 0.9
    # the volume tends to the ball's from below (chords of a convex body)
    ball = 4.0 / 3.0 * np.pi * R.SPHERE_R ** 3
    assert 0.9 * ball < chk["volume"] < ball


def test_torus():
    s, lo, step, _ = R.torus()
    v, f, _ = R.surface_nets(s, 0.0, lo, step)
    chk = R.check_mesh(v, f)
    assert chk["edges_once"] and chk["closed"] and chk["euler"] == 0 and chk["volume"] > 0, chk
    assert abs(len(v) - 1000) <= 4 and len(f) == 2 * len(v), (len(v), len(f))


def test_one_point_and_empty():
    s, lo, step, _ = R.one_point()
    v, f, nr = R.surface_nets(s, 0.5, lo, step)
    chk = R.check_mesh(v, f)
    assert (len(v), len(f)) == (8, 12)
    assert chk["edges_once"] and chk["closed"] and chk["euler"] == 2 and chk["volume"] > 0, chk
    # each of the 8 cells round the point has three crossings at t = 1/2: their
    # mean lies a sixth of a cell's edge (0.5) from the point on every axis
    assert np.allclose(np.abs(v), 0.5 / 6.0, atol=1e-6)
    s, lo, step, _ = R.empty()
    v, f, nr = R.surface_nets(s, 0.5, lo, step)
    assert v.shape == (0, 3) and f.shape == (0, 3) and nr.shape == (0, 3)


def test_half_space_is_an_open_sheet():
    s, lo, step, _ = R.half_space()
    v, f, nr = R.surface_nets(s, 0.0, lo, step)
    chk = R.check_mesh(v, f)
    assert (len(v), len(f)) == (96, 154)
    assert chk["edges_once"] and not chk["closed"], chk
    assert f.min() >= 0 and f.max() < len(v)               # no face refers to a missing vertex
    # every vertex lies on the plane 0.3 - x - 0.5 y = 0 (a linear field is exact)
    assert np.abs(0.3 - v[:, 0] - 0.5 * v[:, 1]).max() < 1e-5
    want = -np.array([-1.0, -0.5, 0.0]) / np.linalg.norm([1.0, 0.5, 0.0])
    assert np.abs(nr - want).max() < 1e-5


def test_noise_with_planted_specials():
    s, lo, step, _ = R.noise()
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any()
    assert (s == np.float32(R.NOISE_ISO)).any()
    v, f, nr = R.surface_nets(s, R.NOISE_ISO, lo, step)
    assert len(v) > 100 and len(f) > 100
    assert np.isfinite(v).all() and np.isfinite(nr).all()
    assert f.min() >= 0 and f.max() < len(v)
    hi = lo + step * np.array([12, 9, 5], np.float32)
    assert (v >= lo - 1e-6).all() and (v <= hi + 1e-6).all()


def test_vertex_order_is_cell_order():
    """ids ascend with c = i + nx (j + ny k): the vertices' cells, recovered
    from the positions, are sorted"""
    s, lo, step, _ = R.smooth((16, 15, 10))
    v, f, _ = R.surface_nets(s, 0.0, lo, step)
    cell = np.floor((v - lo) / step).astype(np.int64)
    c = cell[:, 0] + 16 * (cell[:, 1] + 15 * cell[:, 2])
    assert (np.diff(c) > 0).all()
