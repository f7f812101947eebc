"""GPU: the mesh clean-up against its restatements (tests/mesh_clean_ref.py).

  * mesh.components index for index: label, n_vertices, n_faces; the same bits
    on a second call; label unchanged when the face rows are permuted;
  * mesh.filter_components: every criterion alone and all together, a tie, a
    rule that keeps nothing, one that keeps everything, with and without
    normals and colours -- all bit for bit (the filter only moves rows);
  * the floater property: dropping lattice B's floaters gives lattice A's mesh;
  * a face index outside [0, V) is a ValueError (the kernels guard it);
  * mesh.density_lattice(occupancy=True) against the composition -- the
    unmasked one-hot lattices sigma_k (a weight of 1 is exact) times
    occupancy_live, summed in the documented order -- bit for bit;
  * occupancy=False is the call without the argument;
  * extract_mesh / Trainer.export_mesh with the new arguments end to end.
"""
import numpy as np
import pytest
import torch

import image_out_ref as IR
import mesh_clean_ref as C
import mesh_ref as R
from radnerf_amd import mesh
from radnerf_amd import synthetic as S

pytestmark = pytest.mark.gpu


# ---- components ---------------------------------------------------------------------------
def _surface(builder, iso):
    s, lo, step, _ = builder()
    return R.surface_nets(s, iso, lo, step)


def _strip(order):
    f, V = C.strip(4000, order)
    return np.zeros((V, 3), np.float32), f, None


MESHES = {
    "torus": lambda: _surface(R.torus, 0.0),
    "noise": lambda: _surface(R.noise, R.NOISE_ISO),
    "smooth": lambda: _surface(R.smooth, 0.0),            # 12,415 vertices: 13 counting blocks
    "one_point": lambda: _surface(R.one_point, 0.5),
    "empty": lambda: _surface(R.empty, 0.5),              # V = 0, F = 0
    "no_faces": lambda: (np.zeros((70, 3), np.float32), np.zeros((0, 3), np.int32), None),
    "floaters": lambda: _surface(lambda: C.floaters(True), R.SPHERE_ISO),
    "strip": lambda: _strip("identity"),
    "strip_reversed": lambda: _strip("reversed"),
    "strip_permuted": lambda: _strip("permuted"),
}
_built = {}


def _mesh(name, dev, normals=True, colors=False):
    """the numpy mesh (built once, left unchanged) and its device Mesh"""
    if name not in _built:
        v, f, n = MESHES[name]()
        rng = np.random.default_rng(len(v))
        if n is None:
            n = rng.standard_normal((len(v), 3)).astype(np.float32)
        _built[name] = (v, f, n, rng.integers(0, 256, (len(v), 3), dtype=np.uint8))
    v, f, n, c = _built[name]
    t = lambda a: torch.from_numpy(a).to(dev)
    return _built[name], mesh.Mesh(t(v), t(f), t(n) if normals else None, t(c) if colors else None)


@pytest.mark.parametrize("name", list(MESHES))
def test_components_match_reference(cuda, name):
    (v, f, _, _), m = _mesh(name, cuda)
    label, nv, nf = C.components(f, len(v))
    got = mesh.components(m)
    assert got.label.dtype == torch.int32 and got.label.shape == (len(v),)
    assert got.n_vertices.dtype == torch.int64 and got.n_faces.dtype == torch.int64
    assert got.label.is_cuda and got.n_vertices.is_cuda and got.n_faces.is_cuda
    print(f"V {len(v)} F {len(f)} components {len(nv)}")
    assert torch.equal(got.label.cpu(), torch.from_numpy(label))
    assert torch.equal(got.n_vertices.cpu(), torch.from_numpy(nv))
    assert torch.equal(got.n_faces.cpu(), torch.from_numpy(nf))
    if name == "smooth":
        assert len(v) > 8192 and len(nv) == 9
    again = mesh.components(m)
    assert torch.equal(again.label, got.label) and torch.equal(again.n_vertices, got.n_vertices)
    assert torch.equal(again.n_faces, got.n_faces)
    # the labels do not depend on the order of the face rows
    perm = np.random.default_rng(2).permutation(len(f))
    shuffled = mesh.Mesh(m.vertices, torch.from_numpy(np.ascontiguousarray(f[perm])).to(cuda))
    other = mesh.components(shuffled)
    assert torch.equal(other.label, got.label) and torch.equal(other.n_faces, got.n_faces)


# ---- the filter ---------------------------------------------------------------------------
def _same(got, want, normals, colors):
    v, f, n, c = want
    assert got.vertices.dtype == torch.float32 and got.vertices.shape == (len(v), 3)
    assert got.faces.dtype == torch.int32 and got.faces.shape == (len(f), 3)
    assert torch.equal(got.vertices.cpu().view(torch.int32), torch.from_numpy(v).view(torch.int32))
    assert torch.equal(got.faces.cpu(), torch.from_numpy(f))
    if normals:
        assert got.normals.dtype == torch.float32 and got.normals.shape == (len(v), 3)
        assert torch.equal(got.normals.cpu().view(torch.int32),
                           torch.from_numpy(n).view(torch.int32))
    else:
        assert got.normals is None
    if colors:
        assert got.colors.dtype == torch.uint8 and got.colors.shape == (len(v), 3)
        assert torch.equal(got.colors.cpu(), torch.from_numpy(c))
    else:
        assert got.colors is None


RULES = [dict(keep_largest=1), dict(keep_largest=3), dict(min_vertices=60), dict(min_fraction=0.1),
         dict(keep_largest=4, min_vertices=55, min_fraction=0.03)]


@pytest.mark.parametrize("name", ["floaters", "noise", "smooth"])
@pytest.mark.parametrize("normals,colors", [(True, True), (False, False), (True, False)])
def test_filter_matches_reference(cuda, name, normals, colors):
    (v, f, n, c), m = _mesh(name, cuda, normals, colors)
    for kw in RULES:
        want = C.filter_components(v, f, n if normals else None, c if colors else None, **kw)
        got = mesh.filter_components(m, **kw)
        print(name, kw, "kept", len(want[0]), "of", len(v))
        assert 0 < len(want[0]) < len(v)
        _same(got, want, normals, colors)
    # a rule that keeps nothing; one that keeps everything returns the input's bits
    none = mesh.filter_components(m, min_vertices=len(v) + 1)
    _same(none, (v[:0], f[:0], n[:0], c[:0]), normals, colors)
    _same(mesh.filter_components(m, min_vertices=0), (v, f, n, c), normals, colors)
    _same(mesh.filter_components(m, keep_largest=len(v)), (v, f, n, c), normals, colors)


def test_filter_tie_keeps_the_first(cuda):
    (v, f, n, c), _ = _mesh("torus", cuda)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    twice = mesh.Mesh(t(np.concatenate([v, v + np.float32(3)])),
                      t(np.concatenate([f, f + np.int32(len(v))])),
                      t(np.concatenate([n, -n])), t(np.concatenate([c, 255 - c])))
    comp = mesh.components(twice)
    assert comp.n_vertices.tolist() == [len(v)] * 2 and comp.n_faces.tolist() == [len(f)] * 2
    _same(mesh.filter_components(twice, keep_largest=1), (v, f, n, c), True, True)
    both = mesh.filter_components(twice, keep_largest=2)
    assert both.vertices.shape[0] == 2 * len(v) and torch.equal(both.faces, twice.faces)


def test_filter_small_cases(cuda):
    for name in ("empty", "no_faces", "one_point"):
        (v, f, n, c), m = _mesh(name, cuda, True, True)
        want = C.filter_components(v, f, n, c, keep_largest=1)
        _same(mesh.filter_components(m, keep_largest=1), want, True, True)
    assert len(want[0]) == 8


def test_floaters_are_dropped(cuda):
    """filter_components(surface_nets(B), keep_largest=1) has the bits of
    surface_nets(A)"""
    meshes = []
    for with_floaters in (False, True):
        s, lo, step, hi = C.floaters(with_floaters)
        meshes.append(mesh.surface_nets(torch.from_numpy(s).to(cuda), R.SPHERE_ISO, (lo, hi)))
    a, b = meshes
    assert a.vertices.shape[0] == 1184 and b.vertices.shape[0] == 1590
    comp = mesh.components(b)
    assert sorted(comp.n_vertices.tolist(), reverse=True) == [1184, 204, 64, 56, 50, 32]
    got = mesh.filter_components(b, keep_largest=1)
    assert torch.equal(got.vertices.view(torch.int32), a.vertices.view(torch.int32))
    assert torch.equal(got.normals.view(torch.int32), a.normals.view(torch.int32))
    assert torch.equal(got.faces, a.faces)


@pytest.mark.parametrize("bad", [1000, -1, 2 ** 31 - 1, -2 ** 31])
def test_face_index_out_of_range(cuda, bad):
    """validation: the index is never dereferenced, the call raises"""
    (v, f, _, _), _ = _mesh("torus", cuda)
    assert len(v) == 1000
    f = f.copy()
    f[len(f) // 2, 1] = bad
    m = mesh.Mesh(torch.from_numpy(v).to(cuda), torch.from_numpy(f).to(cuda))
    with pytest.raises(ValueError, match="outside"):
        mesh.components(m)
    with pytest.raises(ValueError, match="outside"):
        mesh.filter_components(m, keep_largest=1)
    with pytest.raises(ValueError, match="outside"):
        mesh.components(mesh.Mesh(torch.zeros(0, 3, device=cuda), m.faces))


# ---- the masked lattice -------------------------------------------------------------------
G = 128
# points per axis -> (resolution, the box as fractions of the model's half-width, or None)
SHAPES = {"9x7x5": ((8, 6, 4), ((-0.6, -0.9, 0.1), (0.82, 0.4, 1.0))),
          "40x33x21": ((39, 32, 20), None),               # 27,720 points: no multiple of 32
          "17x17x17": ((16, 16, 16), None)}               # every point on a cell plane of the grid
MODELS = {"K2": (2, 0.5), "K3s16": (3, 16.0), "K9": (9, 0.5)}
_models, _sigmas = {}, {}


def _model(key, dev):
    if key not in _models:
        K, scale = MODELS[key]
        _models[key] = S.parity_scene(K, scale=scale, device=dev).m
    return _models[key]


def _box(m, shape):
    res, frac = SHAPES[shape]
    if frac is None:
        return res, None, (m._h_min, (m._h_min + m._h_ext).astype(np.float32))
    aabb = tuple(tuple(float(np.float32(c) * np.float32(m.scale)) for c in side) for side in frac)
    return res, aabb, aabb


def _reference(key, shape, dev):
    """per (model, shape), once: the unmasked one-hot lattices sigma_k and the
    lattice's points"""
    if (key, shape) not in _sigmas:
        m = _model(key, dev)
        res, aabb, box = _box(m, shape)
        sig = []
        for k in range(m.size):
            w = np.zeros(m.size, np.float32)
            w[k] = 1.0
            sig.append(mesh.density_lattice(m, res, aabb=aabb, weights=w))
        lo, step = R.box_step(box[0], box[1], res)
        x, y, z = R.lattice_points(lo, step, res)
        _sigmas[(key, shape)] = (sig, np.stack([x, y, z], -1).reshape(-1, 3))
    return _sigmas[(key, shape)]


def _morton_z(cascades):
    """z cell coordinate of every bit of a bitfield"""
    i = np.arange(G ** 3, dtype=np.uint32) >> np.uint32(2)
    i &= np.uint32(0x49249249)
    for s, msk in ((2, 0xC30C30C3), (4, 0x0F00F00F), (8, 0xFF0000FF), (16, 0x0000FFFF)):
        i = (i | (i >> np.uint32(s))) & np.uint32(msk)
    return np.tile(i, cascades)


def _bitfields(kind, K, cascades):
    n = cascades * G ** 3 // 8
    rng = np.random.default_rng(17)
    if kind == "ones":
        return np.full((K, n), 255, np.uint8)
    if kind == "zeros":
        return np.zeros((K, n), np.uint8)
    bits = rng.integers(0, 256, (K, n), dtype=np.uint8)      # a different draw per sub-NeRF
    if kind == "half":                                        # z < 0 cleared: whole dead tiles
        keep = np.packbits(_morton_z(cascades) >= G // 2, bitorder="little")
        bits &= keep[None, :]
    return bits


def _weights(K, kind):
    if kind == "uniform":
        return None
    w = np.linspace(0.7, 0.1, K)
    w[0] = 0.0
    return w.astype(np.float32)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("key", list(MODELS))
def test_masked_lattice_equals_composition(cuda, key, shape):
    m = _model(key, cuda)
    K, scale = MODELS[key]
    assert m.cascades == (1 if scale == 0.5 else 6) and m.grid_size == G
    res, aabb, _ = _box(m, shape)
    sig, pts = _reference(key, shape, cuda)
    saved = [getattr(m, f"density_bitfield_{k}").clone() for k in range(K)]
    try:
        for kind in ("random", "ones", "zeros", "half"):
            bits = _bitfields(kind, K, m.cascades)
            S.set_bitfields(m, bits)
            live = [torch.from_numpy(C.occupancy_live(pts, bits[k], m.cascades, G, scale)
                                     .reshape(sig[0].shape)).to(cuda) for k in range(K)]
            share = float(np.mean([float(l.float().mean()) for l in live]))
            for wk in ("uniform", "zero"):
                w = _weights(K, wk)
                wv = np.full(K, np.float32(1) / np.float32(K), np.float32) if w is None else w
                acc = None
                for k in range(K):
                    if wv[k] != 0:
                        t = float(wv[k]) * (sig[k] * live[k])
                        acc = t if acc is None else acc + t
                got = mesh.density_lattice(m, res, aabb=aabb, weights=w, occupancy=True)
                assert got.shape == sig[0].shape and got.dtype == torch.float32
                diff = int((got.view(torch.int32) != acc.view(torch.int32)).sum())
                print(f"{key} {shape} {kind} {wk}: live share {share:.3f}, differing {diff}")
                assert torch.equal(got, acc)
                plain = mesh.density_lattice(m, res, aabb=aabb, weights=w)
                if kind == "ones":
                    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
                elif kind == "zeros":
                    assert not got.any()
                else:
                    assert got.any() and not torch.equal(got, plain)
                if kind == "half" and aabb is None:          # the whole box: z < 0 is dead
                    dead = torch.from_numpy(pts[:, 2].reshape(sig[0].shape) < 0).to(cuda)
                    assert dead.sum() > 64 and not got[dead].any()
    finally:
        S.set_bitfields(m, saved)


@pytest.mark.parametrize("key", ["K2", "K9"])
def test_unmasked_launch_unchanged(cuda, key):
    m = _model(key, cuda)
    res, aabb, _ = _box(m, "40x33x21")
    a = mesh.density_lattice(m, res, aabb=aabb)
    b = mesh.density_lattice(m, res, aabb=aabb, occupancy=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    sig, _ = _reference(key, "40x33x21", cuda)
    w = np.float32(1) / np.float32(m.size)
    acc = float(w) * sig[0]
    for k in range(1, m.size):
        acc = acc + float(w) * sig[k]
    assert torch.equal(a, acc)


# ---- end to end ---------------------------------------------------------------------------
BALLS = ((0.0, 0.0, 0.0, 0.3), (0.4, 0.4, 0.4, 0.08), (-0.4, 0.38, -0.4, 0.08))


def _ball_bits(K):
    """bitfields (scale 0.5, one cascade) with the cells set whose centre lies
    in one of BALLS (x, y, z, r): the object's ball of occupancy, and two small
    ones in the corners, where a trained grid keeps floaters"""
    c = (np.arange(G, dtype=np.float32) + np.float32(0.5)) / np.float32(G) - np.float32(0.5)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    inside = np.zeros(x.shape, bool)
    for bx, by, bz, r in BALLS:
        inside |= ((x - np.float32(bx)) ** 2 + (y - np.float32(by)) ** 2
                   + (z - np.float32(bz)) ** 2) <= np.float32(r * r)
    n = np.arange(G, dtype=np.uint32)
    idx = C.morton3d(*[a.ravel() for a in np.meshgrid(n, n, n, indexing="ij")][::-1])
    flat = np.zeros(G ** 3, bool)
    flat[idx] = inside.ravel()
    return np.tile(np.packbits(flat, bitorder="little"), (K, 1))


def test_extract_and_export_clean(cuda, tmp_path):
    from radnerf_amd.trainer import Trainer
    sc = S.parity_scene(2, device=cuda)
    m = sc.m
    S.set_bitfields(m, _ball_bits(2))
    sig = mesh.density_lattice(m, 32, occupancy=True)
    plain = mesh.density_lattice(m, 32)
    assert not torch.equal(sig, plain) and sig.any()
    iso = float(plain.median())
    box = (m._h_min, (m._h_min + m._h_ext).astype(np.float32))
    raw = mesh.surface_nets(sig, iso, box)
    v, f, n, _ = (t.cpu().numpy() for t in (raw.vertices, raw.faces, raw.normals, raw.faces))
    _, nv, _ = C.components(f, len(v))
    assert len(nv) > 1 and nv.max() > 0.5 * len(v)           # there is something to drop
    want = C.filter_components(v, f, n, keep_largest=1)
    got = mesh.extract_mesh(m, resolution=32, iso=iso, colors=True, occupancy=True, keep_largest=1)
    _same(mesh.Mesh(got.vertices, got.faces, got.normals), want, True, False)
    one = mesh.components(got)
    assert one.n_vertices.tolist() == [int(nv.max())] and one.n_faces.tolist() == [len(want[1])]
    # every vertex lies in the large ball of occupancy (within a lattice cell of it)
    assert float(got.vertices.norm(dim=1).max()) <= 0.3 + 3 ** 0.5 / 32 + 3 ** 0.5 / 128
    # colours: the forward at the kept vertices and normals
    with torch.no_grad():
        rgb = [m(got.vertices, (-got.normals).contiguous(), k)[1].cpu().numpy() for k in range(2)]
    w = np.float32(0.5)
    ref = IR.quantize_u8((w * rgb[0] + w * rgb[1]) / np.float32(w + w))
    assert got.colors.dtype == torch.uint8 and got.colors.shape == (len(want[0]), 3)
    d = np.abs(got.colors.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
    print("kept", len(want[0]), "of", len(v), "components", len(nv), "colour levels off:",
          np.bincount(d.ravel()))
    assert d.max() <= 1 and ref.std() > 0
    assert torch.equal(got.colors, mesh.vertex_colors(m, got.vertices, got.normals))
    # the other criteria reach the filter too
    some = mesh.extract_mesh(m, resolution=32, iso=iso, occupancy=True, min_vertices=20,
                             min_fraction=0.01, normals=False)
    want2 = C.filter_components(v, f, None, min_vertices=20, min_fraction=0.01)
    _same(some, want2, False, False)
    # Trainer.export_mesh forwards the arguments; the file reads back equal
    tr = Trainer(sc.m, sc.g, 256)
    p = str(tmp_path / "clean.ply")
    out = tr.export_mesh(p, resolution=32, iso=iso, colors=True, occupancy=True, keep_largest=1)
    back = mesh.load_ply(p)
    for name in ("vertices", "faces", "normals", "colors"):
        assert torch.equal(getattr(back, name), getattr(out, name).cpu()), name
        assert torch.equal(getattr(out, name), getattr(got, name)), name
