"""Numpy restatements of the mesh clean-up rules (include/radnerf.h, rn_mesh_*
and rn_density_lattice_masked), and the meshes and lattices their tests share.

    components(faces, V)          -> label (V,) i32, n_vertices (C,) i64,
                                     n_faces (C,) i64
    filter_components(v, f, n, c, keep_largest, min_vertices, min_fraction)
                                  -> v, f, n, c of the kept components
    occupancy_live(points, bitfield, cascades, grid_size, scale) -> (N,) bool
    label_rounds(faces, V)        -> the rounds the device's labelling scheme
                                     needs, by a sequential model of it
"""
import math

import numpy as np

import mesh_ref as R

F32 = np.float32


def roots(faces, V):
    """root[v] = the lowest vertex index of v's component, by min-label
    propagation to the fixed point (whole-array steps, no order inside one)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    L = np.arange(V, dtype=np.int64)
    while True:
        old = L.copy()
        if len(f):
            m = L[f].min(1)
            for j in range(3):
                np.minimum.at(L, f[:, j], m)
        L = L[L]
        if np.array_equal(L, old):
            return L


def components(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    root = roots(f, V)
    is_root = root == np.arange(V)
    ids = np.cumsum(is_root) - 1                     # exclusive scan at the roots
    label = ids[root].astype(np.int32)
    C = int(is_root.sum())
    n_vertices = np.bincount(label, minlength=C).astype(np.int64)
    n_faces = np.bincount(label[f[:, 0]], minlength=C).astype(np.int64) if len(f) \
        else np.zeros(C, np.int64)
    return label, n_vertices, n_faces


def keep_mask(n_vertices, V, keep_largest=None, min_vertices=None, min_fraction=None):
    if keep_largest is None and min_vertices is None and min_fraction is None:
        raise ValueError("no criterion")
    keep = np.ones(len(n_vertices), bool)
    if min_vertices is not None:
        keep &= n_vertices >= min_vertices
    if min_fraction is not None:
        keep &= n_vertices >= math.ceil(float(min_fraction) * V)
    if keep_largest is not None:
        order = np.argsort(-n_vertices, kind="stable")      # ties: the lower id first
        top = np.zeros(len(n_vertices), bool)
        top[order[:keep_largest]] = True
        keep &= top
    return keep


def filter_components(vertices, faces, normals=None, colors=None, keep_largest=None,
                      min_vertices=None, min_fraction=None):
    V = len(vertices)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    label, nv, _ = components(f, V)
    keep = keep_mask(nv, V, keep_largest, min_vertices, min_fraction)
    kv = keep[label] if V else np.zeros(0, bool)
    new = np.cumsum(kv) - 1
    kf = kv[f[:, 0]] if len(f) else np.zeros(0, bool)
    sel = lambda t: None if t is None else np.ascontiguousarray(t[kv])
    return (sel(vertices), new[f[kf]].astype(np.int32).reshape(-1, 3), sel(normals), sel(colors))


def label_rounds(faces, V, limit=1000):
    """A sequential model of the device's rounds (hook the lowest of a face's
    three labels onto its vertices and onto the vertices those labels name,
    from the labels as the round found them; then two pointer jumps): the
    number of rounds until the check passes.  The device sees lower labels
    sooner inside a round, never later."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    L = np.arange(V, dtype=np.int64)
    for r in range(limit + 1):
        if (len(f) == 0 or (L[f] == L[f][:, :1]).all()) and (L[L] == L).all():
            return r
        l = L[f]
        m = l.min(1)
        for j in range(3):
            np.minimum.at(L, f[:, j], m)
            np.minimum.at(L, l[:, j], m)
        L = np.minimum(L, np.minimum(L[L], L[L[L]]))
    raise RuntimeError("label_rounds: no fixed point")


# ---- the occupancy cell -------------------------------------------------------------
def _expand_bits(v):
    v = v.astype(np.uint32)
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    v = (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
    return v


def morton3d(x, y, z):
    return _expand_bits(x) | (_expand_bits(y) << np.uint32(1)) | (_expand_bits(z) << np.uint32(2))


def occupancy_cell(points, cascades, grid_size, scale):
    """The index of the bit the march queries for a position (the dt term
    dropped).  For the scales the tests use, 0.5 and 16, mbi = 1 / min(2^(mip -
    1), scale) is a power of two: the product inside fmaf(c, mbi, 1) is exact,
    so a fp32 multiply and a fp32 add round once, as the fma does, and fp32
    numpy reproduces the device's cell exactly.  Other scales are refused."""
    if float(scale) not in (0.5, 16.0):
        raise ValueError("occupancy_cell: exact for scale 0.5 and 16 only")
    p = np.asarray(points, F32).reshape(-1, 3)
    mx = np.abs(p).max(1)
    e = np.frexp(mx)[1].astype(np.int64)
    mip = np.minimum(cascades - 1, np.maximum(0, e + 1))
    mb = np.minimum(np.ldexp(F32(1), (mip - 1).astype(np.int32)).astype(F32), F32(scale))
    mbi = (F32(1) / mb).astype(F32)
    G = F32(grid_size)
    n = []
    for d in range(3):
        t = (F32(0.5) * (p[:, d] * mbi + F32(1)).astype(F32) * G).astype(F32)
        n.append(np.maximum(F32(0), np.minimum(t, G - F32(1))).astype(np.int64))
    return mip * grid_size ** 3 + morton3d(n[0], n[1], n[2]).astype(np.int64)


def occupancy_live(points, bitfield, cascades, grid_size, scale):
    idx = occupancy_cell(points, cascades, grid_size, scale)
    b = np.asarray(bitfield, np.uint8)
    return ((b[idx >> 3] >> (idx & 7).astype(np.uint8)) & 1).astype(bool)


# ---- the shared meshes ----------------------------------------------------------------
BALL_R = 0.5
BLOBS = ((0.8, 0.8, 0.8, 0.1), (-0.8, 0.7, 0.0, 0.12), (0.0, -0.8, 0.75, 0.08),
         (0.75, -0.75, -0.75, 0.1))
CAVITY = (0.05, 0.0, 0.0, 0.2)


def _blob(x, y, z, cx, cy, cz, r):
    d = np.sqrt((x - F32(cx)) ** 2 + (y - F32(cy)) ** 2 + (z - F32(cz)) ** 2)
    return (F32(20.0) * np.exp(F32(-3.0) * d / F32(r))).astype(F32)


def floaters(with_floaters, n=32):
    """s = 20 exp(-3 d / r) on UNIT at n cells per axis, level SPHERE_ISO (the
    sphere d = r).  A: one ball of radius BALL_R at the origin.  B: the larger
    of that and of the four BLOBS, with a zeroed cavity inside the ball."""
    lo, step = R.box_step(*R.UNIT, (n,) * 3)
    x, y, z = R.lattice_points(lo, step, (n,) * 3)
    s = _blob(x, y, z, 0.0, 0.0, 0.0, BALL_R)
    if with_floaters:
        for b in BLOBS:
            s = np.maximum(s, _blob(x, y, z, *b))
        cx, cy, cz, r = CAVITY
        d = np.sqrt((x - F32(cx)) ** 2 + (y - F32(cy)) ** 2 + (z - F32(cz)) ** 2)
        s = np.where(d < F32(r), F32(0), s).astype(F32)
    return s, lo, step, np.asarray(R.UNIT[1], F32)


def strip(n_quads=4000, order="identity", seed=5):
    """A strip of n_quads quads (2 n_quads + 2 vertices, one component) whose
    vertex indices are left as they are, reversed, or randomly permuted: a long
    thin mesh is the case that needs the most rounds."""
    q = np.arange(n_quads)
    a, b, c, d = 2 * q, 2 * q + 1, 2 * q + 3, 2 * q + 2
    f = np.stack([a, b, c, a, c, d], 1).reshape(-1, 3)
    V = 2 * n_quads + 2
    if order == "reversed":
        f = V - 1 - f
    elif order == "permuted":
        f = np.random.default_rng(seed).permutation(V)[f]
    elif order != "identity":
        raise ValueError(order)
    return f.astype(np.int32), V


def union_find(faces, V):
    """plain Python union-find -> root (V,) = the lowest index of each set"""
    parent = list(range(V))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(i) for i in range(V)], np.int64)
