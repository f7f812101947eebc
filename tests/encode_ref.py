"""The multiresolution hash encoding and its gradients restated in numpy with
fp64 sums (test code: the package does not import it), plus the inputs that
aim at the encode kernels' special cases.

What is fp32 here is what the kernels compute in fp32 and every later step
depends on discretely (csrc/rn_field.h unit_coord, level_pos): the unit
coordinate clip((x - min) / ext, 0, 1), the level position fma(scale_l, u, 0.5),
its cell floor(pos) and fraction pos - floor(pos) (exact), and 1 - f.  The
corner weights' products, the weight x table products and every sum are fp64.
The level table is oracle.field_oracle.grid_levels and the corner index is
tcnn's grid_index with a plain `% hsize` on every level.

Feature order: column 2 l + f is feature f of level l (tcnn's, the MLP's input).
"""
import functools
import types

import numpy as np

from oracle.field_oracle import grid_levels  # noqa: F401  (the level table the tests pass in)

F32 = np.float32
N_LEVELS = 16
P1, P2 = 2654435761, 805459861
U32 = 0xFFFFFFFF


def unit_coords(x, xyz_min, ext):
    """fp32 clip((x - mn) / ext, 0, 1), (N, 3); IEEE division as the kernels'."""
    return np.clip(unit_raw(x, xyz_min, ext), F32(0), F32(1))


def unit_raw(x, xyz_min, ext):
    """the quotient before the clip (the input gradient's mask is 0 <= v <= 1)"""
    x = np.asarray(x, F32)
    return ((x - np.asarray(xyz_min, F32)) / np.asarray(ext, F32)).astype(F32)


def level_cells(u, lv, l):
    """(g int64 (N, 3), f fp32 (N, 3)) of level l: pos = fp32 fma(scale_l, u, 0.5)
    through fp64 (the product of two fp32 is exact there), g = floor(pos),
    f = pos - g."""
    pos = (np.float64(lv["scale"][l]) * np.asarray(u, F32).astype(np.float64) + 0.5).astype(F32)
    g = np.floor(pos)
    f = (pos - g).astype(F32)
    return g.astype(np.int64), f


def is_dense(lv, l):
    return int(lv["res"][l]) ** 3 <= int(lv["hsize"][l])


def corner_raw(lv, l, g):
    """tcnn grid_index of the 8 corners of cells g (N, 3) before the modulo,
    as uint32 values in int64 (N, 8); corner c = bx + 2 by + 4 bz."""
    res = int(lv["res"][l])
    out = np.empty((len(g), 8), np.int64)
    for c in range(8):
        x, y, z = g[:, 0] + (c & 1), g[:, 1] + ((c >> 1) & 1), g[:, 2] + ((c >> 2) & 1)
        if is_dense(lv, l):
            out[:, c] = (x + y * res + z * res * res) & U32
        else:
            out[:, c] = (x ^ ((y * P1) & U32) ^ ((z * P2) & U32)) & U32
    return out


def corner_indices(lv, l, g):
    """entry of each corner within level l, (N, 8)"""
    return corner_raw(lv, l, g) % int(lv["hsize"][l])


def corner_weights(f):
    """(N, 8) fp64 trilinear weights from the fp32 fractions; 1 - f is rounded
    to fp32 as in the kernel, the products are not."""
    f = np.asarray(f, F32)
    lo = (F32(1) - f).astype(F32).astype(np.float64)
    hi = f.astype(np.float64)
    w = np.empty((len(f), 8))
    for c in range(8):
        w[:, c] = ((hi if c & 1 else lo)[:, 0] * (hi if c & 2 else lo)[:, 1] *
                   (hi if c & 4 else lo)[:, 2])
    return w


def _corner_dweights(f):
    """(N, 8, 3): d weight / d f_axis (the cell is floor(pos): right-sided at f == 0)"""
    f = np.asarray(f, F32)
    lo = (F32(1) - f).astype(F32).astype(np.float64)
    hi = f.astype(np.float64)
    d = np.empty((len(f), 8, 3))
    for c in range(8):
        bit = [(c >> a) & 1 for a in range(3)]
        w = [(hi if bit[a] else lo)[:, a] for a in range(3)]
        for a in range(3):
            o = [w[b] for b in range(3) if b != a]
            d[:, c, a] = (1.0 if bit[a] else -1.0) * o[0] * o[1]
    return d


class Cells:
    """Per (sample, level, corner): global entry, weight, weight derivative,
    fraction; computed once per position set and sliced for its prefixes."""

    def __init__(self, x, lv, xyz_min, ext):
        self.lv = lv
        self.x = np.asarray(x, F32)
        self.v = unit_raw(self.x, xyz_min, ext)
        self.u = np.clip(self.v, F32(0), F32(1))
        n = len(self.x)
        self.idx = np.empty((n, N_LEVELS, 8), np.int64)
        self.raw = np.empty((n, N_LEVELS, 8), np.int64)
        self.w = np.empty((n, N_LEVELS, 8))
        self.dw = np.empty((n, N_LEVELS, 8, 3))
        self.f = np.empty((n, N_LEVELS, 3), F32)
        for l in range(N_LEVELS):
            g, f = level_cells(self.u, lv, l)
            self.raw[:, l] = corner_raw(lv, l, g)
            self.idx[:, l] = self.raw[:, l] % int(lv["hsize"][l]) + int(lv["offset"][l])
            self.w[:, l] = corner_weights(f)
            self.dw[:, l] = _corner_dweights(f) * float(lv["scale"][l])
            self.f[:, l] = f
        # d u / d x: 1 / ext where the quotient was not clipped (inclusive)
        self.dudx = np.where((self.v >= 0) & (self.v <= 1), 1.0 / np.asarray(ext, np.float64), 0.0)


def _table64(table_f16):
    t = np.asarray(table_f16)
    assert t.ndim == 2 and t.shape[1] == 2
    t16 = t.astype(np.float16)
    assert np.array_equal(t16.astype(np.float64), t.astype(np.float64)), "table holds non-f16 values"
    return t16.astype(np.float64)


def encode_cells(cells, table_f16):
    """(N, 32) fp64 features of precomputed Cells"""
    t = _table64(table_f16)[cells.idx]                       # (N, 16, 8, 2)
    return (cells.w[..., None] * t).sum(2).reshape(len(cells.x), 2 * N_LEVELS)


def encode(x, table_f16, lv, xyz_min, ext):
    """(N, 32) fp64 hash-grid features of positions x (N, 3) fp32"""
    return encode_cells(Cells(x, lv, xyz_min, ext), table_f16)


def lane_level(q, h):
    return 2 * h + (q & 1) + 4 * (q >> 1)


def decode_cache(feat, n):
    """The kernels' encoding cache [tile of 32 samples][64 lanes][2 k-steps][8]
    f16 -> (n, 32) f16 in feature order: lane c + 32 h holds sample c, element j
    of k-step s is level lane_level(4 s + (j >> 1), h), feature j & 1."""
    feat = np.asarray(feat).reshape(-1, 64, 2, 8)
    assert feat.dtype == np.float16 and feat.shape[0] * 32 >= n
    i = np.arange(n)
    out = np.empty((n, 2 * N_LEVELS), np.float16)
    for h in range(2):
        for s in range(2):
            for j in range(8):
                out[:, 2 * lane_level(4 * s + (j >> 1), h) + (j & 1)] = feat[i // 32, i % 32 + 32 * h, s, j]
    return out


def _slice(cells, sl):
    if sl is None:
        return slice(0, len(cells.x))
    return slice(0, sl) if isinstance(sl, (int, np.integer)) else sl


def grid_grad_entries(cells, dfeat, sl=None):
    """Sparse per-entry gradient of the samples sl (a slice, or a prefix
    length; dfeat holds every sample's row): (entries (M) sorted,
    grad (M, 2) = sum w dfeat, abs (M, 2) = sum |w dfeat|, count (M) = number
    of (sample, corner) contributions), all sums fp64."""
    sl = _slice(cells, sl)
    idx, w = cells.idx[sl], cells.w[sl]
    n = len(idx)
    d = np.asarray(dfeat, np.float64)[sl].reshape(n, N_LEVELS, 1, 2)
    c = w[:, :, :, None] * d                                 # (n, 16, 8, 2)
    ent, inv = np.unique(idx.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1)
    c = c.reshape(-1, 2)
    m = len(ent)
    grad = np.stack([np.bincount(inv, c[:, k], m) for k in range(2)], 1)
    ab = np.stack([np.bincount(inv, np.abs(c[:, k]), m) for k in range(2)], 1)
    return ent, grad, ab, np.bincount(inv, minlength=m)


def _dense(n_entries, ent, val):
    out = np.zeros((n_entries,) + val.shape[1:], val.dtype)
    out[ent] = val
    return out


def grid_grad(x, dfeat, lv, xyz_min, ext):
    """((entries, 2) fp64 sum of w * dfeat, (entries) int64 contribution count)"""
    ent, g, _, cnt = grid_grad_entries(Cells(x, lv, xyz_min, ext), dfeat)
    return _dense(int(lv["n_entries"]), ent, g), _dense(int(lv["n_entries"]), ent, cnt)


def abs_grid_grad(x, dfeat, lv, xyz_min, ext):
    """(entries, 2) fp64 sum of |w * dfeat| (the scale of the per-entry bound)"""
    ent, _, a, _ = grid_grad_entries(Cells(x, lv, xyz_min, ext), dfeat)
    return _dense(int(lv["n_entries"]), ent, a)


def dencode_dx_cells(cells, table_f16):
    """(D, A), both (N, 32, 3) fp64: D = d feature / d x (right-sided at f == 0,
    zero on an axis whose unit coordinate was clipped), A = the same sum over
    the 8 corners of the terms' magnitudes."""
    t = _table64(table_f16)[cells.idx]                       # (N, 16, 8, 2)
    terms = cells.dw[:, :, :, None, :] * t[..., None]         # (N, 16, 8, 2, 3)
    terms = terms * cells.dudx[:, None, None, None, :]
    n = len(cells.x)
    return (terms.sum(2).reshape(n, 2 * N_LEVELS, 3),
            np.abs(terms).sum(2).reshape(n, 2 * N_LEVELS, 3))


def dencode_dx(x, table_f16, lv, xyz_min, ext):
    return dencode_dx_cells(Cells(x, lv, xyz_min, ext), table_f16)[0]


def rn16(v):
    """round to nearest even f16 (subnormals included), returned as fp64"""
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------
# a field MLP that makes dL/dfeature known
# ---------------------------------------------------------------------------
FIELD_PARAMS = 9472
G1, G2 = 0, 2048            # Wg1 [64, 32] | Wg2 [17, 64]  (radnerf_amd.layout, oracle.ml_oracle._split_field)


def transparent_a(K):
    """(K, 32) powers of two in [2^-2, 2^2]: neighbouring features and levels,
    and the sub-NeRFs at one feature, all differ."""
    j = np.arange(2 * N_LEVELS)
    return np.stack([2.0 ** ((2 * j + k) % 5 - 2) for k in range(K)])


def transparent_c():
    """(32) the first layer's factors c_j of transparent_mlp"""
    return np.where(np.arange(2 * N_LEVELS) % 2 == 0, 1.0, 2.0)


def transparent_mlp(K, a):
    """(K, 9472) fp32 field parameters with geo output 0 = sum_j a_j e_j:
    Wg1 rows j / 32 + j are +c_j / -c_j times unit vector j (ReLU keeps one of
    them), Wg2 row 0 is +b_j on column j and -b_j on column 32 + j with
    a_j = c_j b_j (c_j = 1 for even j, 2 for odd), every other weight zero.  So
    sigma = exp(sum a_j e_j), rgb = sigmoid(0) = 0.5 with no gradient, and
    dL/de_j = a_j dsigma sigma wherever e_j != 0.  All factors are powers of
    two and each dot product has one non-zero term: after the one f16
    rounding of the scaled seed the kernels' backward chain is exact."""
    a = np.asarray(a, np.float64)
    assert a.shape == (K, 2 * N_LEVELS)
    p = np.zeros((K, FIELD_PARAMS), F32)
    c = transparent_c()
    for k in range(K):
        g1 = p[k, G1:G1 + 64 * 32].reshape(64, 32)
        g2 = p[k, G2:G2 + 17 * 64].reshape(17, 64)
        for j in range(32):
            g1[j, j], g1[32 + j, j] = c[j], -c[j]
            g2[0, j], g2[0, 32 + j] = a[k, j] / c[j], -a[k, j] / c[j]
    return p


def transparent_sigma(e, a):
    """exp(sum_j a_j rn16(e_j)), fp64: what the field gives with transparent_mlp"""
    return np.exp((rn16(e) * np.asarray(a, np.float64)).sum(1))


def dsigma_seeds(sigma, seed):
    """fp32 dL/dsigma with |dsigma sigma| in [1, 4] and random sign: across a
    batch the scaled seeds stay within a factor 256 of the block's largest, so
    none falls into f16 subnormals at the block's gradient scale."""
    rng = np.random.default_rng(seed)
    n = len(sigma)
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 4.0, n) / np.asarray(sigma, np.float64)).astype(F32)


DOUBT = 2.0 ** -20


def doubtful(e):
    """(N, 32) features so close to zero that their f16 value may be an exact
    zero on one side only: ReLU' there is the one place where kernel and
    reference may legitimately disagree."""
    return np.abs(e) < DOUBT


def doubtful_entries(cells, e, sl=None):
    """sorted entries that receive a contribution from a doubtful (sample,
    feature) among the samples sl (e holds every sample's row)"""
    sl = _slice(cells, sl)
    d = doubtful(e[sl]).reshape(-1, N_LEVELS, 2).any(2)
    return np.unique(cells.idx[sl][d])


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _to_x(u, scale):
    """fp32 position whose unit coordinate is near u (box [-scale, scale]^3)"""
    return (np.asarray(u, np.float64) * (2.0 * scale) - scale).astype(F32)


def _ulp_step(x, k):
    x = np.asarray(x, F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def _snap(x, axes, lv, l, scale):
    """Move x (3,) by up to 3 ulps on `axes` so that level l's position is an
    exact integer there, if such a neighbour exists."""
    mn, ext = F32(-scale), F32(2 * scale)
    x = x.copy()
    for a in axes:
        for k in (0, 1, -1, 2, -2, 3, -3):
            c = _ulp_step(x[a:a + 1], k)
            _, f = level_cells(unit_coords(c, mn, ext), lv, l)
            if f[0] == 0:
                x[a] = c[0]
                break
    return x


def adversarial_points(scale, lv, seed=0):
    """About 3.3 k fp32 positions (N, 3) for the box [-scale, scale]^3:
    faces / corners / outside points, lattice vertices of every level on one
    axis and on all three with their neighbours one ulp above and below,
    dyadic unit coordinates i / 64, and uniform points in +-1.02 scale."""
    rng = np.random.default_rng(1000 + seed)
    out = []
    # box faces, corners, outside
    v = np.array([-1.5, -1.0, 0.0, 1.0, 1.5]) * scale
    out.append(np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3))
    # lattice vertices: u = (k - 0.5) / scale_l
    for l in range(N_LEVELS):
        s = float(lv["scale"][l])
        kmax = int(np.floor(s + 0.5))
        for t in range(20):
            axes = (0, 1, 2) if t >= 15 else (t % 3,)
            u = rng.uniform(0.02, 0.98, 3)
            for a in axes:
                u[a] = (int(rng.integers(1, kmax + 1)) - 0.5) / s
            x = _snap(_to_x(u, scale), axes, lv, l, scale)
            for k in (-1, 0, 1):
                y = x.copy()
                for a in axes:
                    y[a] = _ulp_step(x[a:a + 1], k)[0]
                out.append(y[None])
    # dyadic unit coordinates (the faces i = 0 and i = 64 included)
    i = rng.integers(0, 65, (400, 3))
    out.append(_to_x(i / 64.0, scale))
    out.append(_to_x(np.repeat(np.arange(65)[:, None], 3, 1) / 64.0, scale))
    out.append(rng.uniform(-1.02 * scale, 1.02 * scale, (2000, 3)))
    x = np.concatenate([np.asarray(o, np.float64) for o in out]).astype(F32)
    return np.ascontiguousarray(x[rng.permutation(len(x))])


def ordered_sequences(scale, lv, seed=0):
    """Positions whose ORDER matters (the scatter walks merge runs of samples
    that hit the same corner): one position repeated 2, 63, 64, 65 and 300
    times, two positions of one finest-level cell alternating, two positions
    in x-adjacent finest-level cells alternating."""
    rng = np.random.default_rng(2000 + seed)
    s = float(lv["scale"][N_LEVELS - 1])
    out = []
    for n in (2, 63, 64, 65, 300):
        out.append(np.repeat(_to_x(rng.uniform(0.05, 0.95, (1, 3)), scale), n, 0))
    for dx in (0.0, 1.0):
        g = np.floor(rng.uniform(0.1, 0.9, 3) * s)
        ua = (g + np.array([0.2, 0.3, 0.6]) - 0.5) / s
        ub = (g + np.array([0.7 + dx, 0.5, 0.1]) - 0.5) / s
        pair = _to_x(np.stack([ua, ub]), scale)
        out.append(np.tile(pair, (64, 1)))
    return np.ascontiguousarray(np.concatenate(out).astype(F32))


def lattice_rays(scale, lv, seed=0):
    """24 axis-aligned rays, 8 per axis: direction exactly a unit axis vector,
    origin at -3 scale on that axis and, on the other two, strictly inside
    the box on a lattice plane of some level or one ulp off it."""
    rng = np.random.default_rng(3000 + seed)
    o = np.zeros((24, 3), F32)
    d = np.zeros((24, 3), F32)
    for r in range(24):
        ax = r // 8
        l = int(rng.integers(0, N_LEVELS))
        s = float(lv["scale"][l])
        kmax = int(np.floor(s + 0.5))
        others = [a for a in range(3) if a != ax]
        u = np.full(3, 0.5)
        for a in others:
            u[a] = (int(rng.integers(max(1, kmax // 8), kmax - kmax // 8 + 1)) - 0.5) / s
        x = _snap(_to_x(u, scale), others, lv, l, scale)
        for a in others:
            x[a] = _ulp_step(x[a:a + 1], (r % 8) % 3 - 1)[0]
        assert np.all(np.abs(x[others]) < scale)
        x[ax] = F32(-3.0 * scale)
        o[r], d[r, ax] = x, 1.0
    return o, d


PREFIXES = (1, 31, 32, 33, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def case(scale):
    """The shared, read-only test case of one scale: the adversarial points
    followed by the ordered sequences (x, n_adv of them adversarial), the f16
    table synthetic.grid_params, the reference cells and features, and the
    runs the per-model kernels are given: name -> slice of x."""
    from radnerf_amd import synthetic
    lv = grid_levels(scale)
    adv = adversarial_points(scale, lv)
    x = np.concatenate([adv, ordered_sequences(scale, lv)])
    table = synthetic.grid_params(int(lv["n_entries"])).astype(np.float16)
    mn, ext = np.full(3, -scale, F32), np.full(3, 2 * scale, F32)
    cells = Cells(x, lv, mn, ext)
    e = encode_cells(cells, table)
    for a in (x, table, e, cells.idx, cells.w, cells.dw, cells.f, cells.u, cells.v):
        a.setflags(write=False)
    runs = {"adversarial": slice(0, len(adv)), "sequences": slice(len(adv), len(x))}
    runs.update({f"prefix{n}": slice(0, n) for n in PREFIXES})
    return types.SimpleNamespace(scale=scale, lv=lv, x=x, n_adv=len(adv), table=table, mn=mn,
                                 ext=ext, cells=cells, e=e, runs=runs)
