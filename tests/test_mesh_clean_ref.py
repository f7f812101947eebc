"""CPU: the numpy restatements of the mesh clean-up rules
(tests/mesh_clean_ref.py) against a plain Python union-find, the known answers
on mesh_ref's lattices, the filter's rules on a hand-made mesh, the floater
property (dropping the floaters of lattice B gives lattice A's mesh bit for
bit), the occupancy cell against a scalar restatement, and the rounds the
labelling scheme needs (what mesh.LABEL_ROUNDS is sized from).
tests/test_gpu_mesh_clean.py compares the kernels with these, index for index.
"""
import math

import numpy as np
import pytest

import mesh_clean_ref as C
import mesh_ref as R
from radnerf_amd import mesh

KNOWN = {"torus": (lambda: R.torus() + (0.0,), 1000, 2000, 1),
         "noise": (lambda: R.noise() + (R.NOISE_ISO,), 522, 1088, 7),
         "smooth": (lambda: R.smooth() + (0.0,), 12415, 23762, 9),
         "one_point": (lambda: R.one_point() + (0.5,), 8, 12, 1)}


def _mesh_of(builder):
    s, lo, step, _, iso = builder()
    return R.surface_nets(s, iso, lo, step)


def _check_components(f, V):
    label, nv, nf = C.components(f, V)
    uf = C.union_find(f, V)
    assert np.array_equal(C.roots(f, V), uf)
    # ids ascend with the root; counts are the sizes
    r = np.unique(uf)
    assert np.array_equal(label, np.searchsorted(r, uf).astype(np.int32))
    assert label.dtype == np.int32 and nv.dtype == np.int64 and nf.dtype == np.int64
    assert np.array_equal(nv, np.bincount(label, minlength=len(r)))
    assert nv.sum() == V and nf.sum() == len(f)
    if len(f):
        assert (label[f] == label[f][:, :1]).all()
    return label, nv, nf


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(name):
    builder, n_v, n_f, n_c = KNOWN[name]
    v, f, _ = _mesh_of(builder)
    assert (len(v), len(f)) == (n_v, n_f)
    _, nv, _ = _check_components(f, len(v))
    assert len(nv) == n_c


@pytest.mark.parametrize("order", ["identity", "reversed", "permuted"])
def test_strip_and_rounds(order):
    f, V = C.strip(4000, order)
    assert V == 8002 and len(f) == 8000
    _, nv, nf = _check_components(f, V)
    assert nv.tolist() == [V] and nf.tolist() == [8000]
    # one batch of the device's rounds covers the worst of the test meshes
    assert C.label_rounds(f, V) <= mesh.LABEL_ROUNDS


def test_isolated_vertices_and_no_faces():
    label, nv, nf = _check_components(np.zeros((0, 3), np.int32), 5)
    assert label.tolist() == [0, 1, 2, 3, 4] and nv.tolist() == [1] * 5 and nf.tolist() == [0] * 5
    f = np.array([[4, 6, 5], [1, 2, 1]], np.int32)              # 0, 3, 7 in no face
    label, nv, nf = _check_components(f, 8)
    assert label.tolist() == [0, 1, 1, 2, 3, 3, 3, 4]
    assert nv.tolist() == [1, 2, 1, 3, 1] and nf.tolist() == [0, 1, 0, 1, 0]
    label, nv, nf = C.components(np.zeros((0, 3), np.int32), 0)
    assert len(label) == 0 and len(nv) == 0 and len(nf) == 0


def test_filter_rules():
    # components by id: {0} (1 vertex), {1, 2, 3} (3), {4, 5, 6} (3), {7, 8} (2)
    f = np.array([[7, 8, 7], [4, 5, 6], [1, 2, 3], [3, 2, 1]], np.int32)
    v = np.arange(27, dtype=np.float32).reshape(9, 3)
    n = -v
    c = (np.arange(27) % 251).astype(np.uint8).reshape(9, 3)
    fl = lambda **kw: C.filter_components(v, f, n, c, **kw)
    # a tie at the top: the lower id wins
    gv, gf, gn, gc = fl(keep_largest=1)
    assert np.array_equal(gv, v[1:4]) and np.array_equal(gn, n[1:4]) and np.array_equal(gc, c[1:4])
    assert gf.tolist() == [[0, 1, 2], [2, 1, 0]] and gf.dtype == np.int32
    gv, gf, _, _ = fl(keep_largest=2)
    assert np.array_equal(gv, v[1:7]) and gf.tolist() == [[3, 4, 5], [0, 1, 2], [2, 1, 0]]
    gv, gf, _, _ = fl(min_vertices=2)
    assert np.array_equal(gv, v[1:]) and gf.tolist() == [[6, 7, 6], [3, 4, 5], [0, 1, 2], [2, 1, 0]]
    # ceil(0.3 * 9) = 3; ceil(0.23 * 9) = 3; ceil(2 / 9 * 9) = 2 in Python floats
    assert len(fl(min_fraction=0.3)[0]) == 6 and len(fl(min_fraction=0.23)[0]) == 6
    assert math.ceil(2 / 9 * 9) == 2 and len(fl(min_fraction=2 / 9)[0]) == 8
    # every criterion must hold
    gv, gf, _, _ = fl(keep_largest=3, min_vertices=3, min_fraction=0.1)
    assert np.array_equal(gv, v[1:7])
    gv, gf, gn, gc = fl(min_vertices=4)
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gn.shape == (0, 3) and gc.shape == (0, 3)
    gv, gf, gn, gc = fl(min_vertices=0)
    assert np.array_equal(gv, v) and np.array_equal(gf, f)
    assert C.filter_components(v, f, keep_largest=9)[2] is None
    with pytest.raises(ValueError):
        C.filter_components(v, f)


def test_floaters():
    """lattice B = lattice A's ball + four blobs + a cavity inside the ball:
    keeping the largest component gives A's mesh bit for bit"""
    a, b = C.floaters(False), C.floaters(True)
    va, fa, na = R.surface_nets(a[0], R.SPHERE_ISO, a[1], a[2])
    vb, fb, nb = R.surface_nets(b[0], R.SPHERE_ISO, b[1], b[2])
    _, nva, _ = _check_components(fa, len(va))
    _, nvb, _ = _check_components(fb, len(vb))
    assert len(va) == 1184 and nva.tolist() == [1184]
    assert len(vb) == 1590 and sorted(nvb.tolist(), reverse=True) == [1184, 204, 64, 56, 50, 32]
    gv, gf, gn, _ = C.filter_components(vb, fb, nb, keep_largest=1)
    assert np.array_equal(gv.view(np.int32), va.view(np.int32))
    assert np.array_equal(gn.view(np.int32), na.view(np.int32))
    assert np.array_equal(gf, fa)
    # the cavity is the second largest: min_vertices alone cannot tell it from the ball's size class
    assert len(C.filter_components(vb, fb, nb, min_vertices=100)[0]) == 1184 + 204
    assert len(C.filter_components(vb, fb, nb, min_fraction=0.5)[0]) == 1184


def _cell_scalar(p, cascades, G, scale):
    """occupancy_cell one point at a time, in Python floats rounded to fp32"""
    f = np.float32
    mx = max(abs(float(p[0])), abs(float(p[1])), abs(float(p[2])))
    e = math.frexp(mx)[1]
    mip = min(cascades - 1, max(0, e + 1))
    mb = min(2.0 ** (mip - 1), scale)
    n = []
    for c in p:
        t = float(f(0.5) * f(f(float(c) / mb) + f(1)) * f(G))    # c / mb: exact, a power of two
        n.append(int(max(0.0, min(t, G - 1.0))))
    m = 0
    for bit in range(10):
        for d in range(3):
            m |= ((n[d] >> bit) & 1) << (3 * bit + d)
    return mip * G ** 3 + m


@pytest.mark.parametrize("scale,cascades", [(0.5, 1), (16.0, 6)])
def test_occupancy_cell(scale, cascades):
    rng = np.random.default_rng(3)
    G = 128
    p = rng.uniform(-scale, scale, (400, 3)).astype(np.float32)
    # the mip boundaries, the cell planes, the box's faces and the origin
    edge = [0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, scale, 1 / 128, 0.5 - 1 / 256]
    p[:len(edge), 0] = edge
    p[len(edge):2 * len(edge), 1] = [-e for e in edge]
    p[40] = 0.0
    p[50:150] *= np.float32(2.0) ** -rng.integers(1, 8, (100, 1)).astype(np.float32)   # the inner mips
    p = np.clip(p, -scale, scale)
    idx = C.occupancy_cell(p, cascades, G, scale)
    want = np.array([_cell_scalar(q, cascades, G, scale) for q in p])
    assert np.array_equal(idx, want)
    assert idx.min() >= 0 and idx.max() < cascades * G ** 3
    if cascades > 1:
        assert len(np.unique(idx // G ** 3)) == cascades      # every mip occurs
    bits = rng.integers(0, 256, cascades * G ** 3 // 8, dtype=np.uint8)
    live = C.occupancy_live(p, bits, cascades, G, scale)
    assert np.array_equal(live, np.unpackbits(bits, bitorder="little")[idx].astype(bool))
    assert live.any() and not live.all()
    with pytest.raises(ValueError):
        C.occupancy_cell(p, 2, G, 1.5)
