"""Shared inputs and host restatements for the occupancy-grid march tests
(tests/test_march_ref.py on the CPU, tests/test_gpu_march.py on the GPU).  Not
a test module.

edge_rays()        the rays synthetic.rays() never produces: zero direction
                   components of both signs, origins inside the box, on cell
                   planes and on the box faces, misses, and a plain control.
chunk_ts_serial()  the 64 step times of one chunk of march_ray_wave
chunk_ts_closed()  (rn_march.h), by serial float32 additions and by the
                   kernel's closed-form shortcut for constant dt.
march_plain()      raymarching.cu:195-279 for one ray in numpy float32, written
                   from the reference's text: a second opinion on
                   oracle/vren_oracle.c.
Guarded            exact-size device buffers with a sentinel tail.

The issue's `grazing` family is kept as two: `grazing_exact` has the off-axis
coordinate exactly +-scale; such a ray lies in a face plane, its slab test
yields 0 * inf = NaN, and it misses the box (check_coverage says why), so it
can never have samples.  `grazing` is the same set of rays one float32 ulp
inside the face, which march through the outermost cells.

Inputs out of bounds for every march here (reference, oracle and kernels):
  * no all-zero direction (every cell-exit time is inf or NaN);
  * no non-finite origin or direction;
  * no origin farther than 3 * scale from the centre (in the max norm: no
    coordinate beyond +-3 * scale).
Past these bounds t + dt == t can occur (t so large that dt is below half an
ulp), and then the reference's loop, the oracle's and the kernels' never end.
check_in_bounds() is called by edge_rays() and by every test before a march
starts; bounded_work() states the bound the GPU tests rely on.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

import oracle
from radnerf_amd import synthetic as S

F = np.float32
SQRT3 = F(1.73205080757)            # raymarching.cu:4
NEAR_DISTANCE = F(0.01)             # ml_rendering.py:8
GRID = 128
FAMILIES = ("axis", "planar", "inside", "grazing", "grazing_exact", "miss", "plain")

# (scale, exp_step_factor): the constant-dt march with one cascade, the
# constant-dt march with 1 / scale not a power of two (3 cascades), the
# exponential march (6 cascades)
CONFIGS = ((0.5, 0.0), (1.5, 0.0), (16.0, 1.0 / 256))
OCCUPANCY = (0.5, 1.0)
# both sides of n + 64 < cap, n + emitted + run >= cap and e2 < 64 in
# march_ray_wave, the product's 1024, and two odd values for new d0s
CAPS = (1, 63, 64, 65, 127, 128, 129, 1024, 37, 1000)
FUSED_CAPS = (64, 65, 1024)
RENDER_CAPS = (1, 31, 32, 33, 64, 1024)


def cascades_of(scale):
    """networks.py:44 (NGP.__init__)"""
    return max(1 + int(np.ceil(np.log2(2 * scale))), 1)


def reaches_cap(scale, p, max_samples):
    """The training-march cases that claim rays at the sample cap (the tests
    assert >= 8 such rays there).  Scale 0.5: the chord is at most sqrt(3) and
    dt is sqrt(3) / max_samples, so only max_samples = 1 is reached.  Scale 1.5
    (esf 0): the chord is up to 3 sqrt(3), three caps' worth of steps.  Scale
    16 (esf 1/256): a ray from outside (t1 ~ 32) takes about 256 ln(t2 / t1)
    ~ 200 steps whatever max_samples is, so caps up to 129 are reached; on a
    full grid a ray from inside takes a few hundred steps of dt_min up to
    t = 256 dt_min and 256 ln(t2 / t) more from there, which also reaches 1000
    and 1024."""
    if max_samples == 1:
        return True
    if scale == 1.5:
        return True
    if scale == 16.0:
        return max_samples <= 129 or p == 1.0
    return False


def reaches_cap_test(scale, max_samples):
    """The same claim for the test-time march of hits_entry, whose calc_dt is
    handed `cascades` as its scale (raymarching.cu:370): at scale 0.5 again
    only max_samples = 1; at 1.5 the chord holds three caps' worth of steps;
    at scale 16 the rays from inside start at t < 0 with dt_min and take
    more than 1024 steps to leave the box."""
    return max_samples == 1 or scale > 0.5


# ----------------------------------------------------------------------------
# rays
# ----------------------------------------------------------------------------
def check_in_bounds(o, d, scale):
    o, d = np.asarray(o), np.asarray(d)
    assert o.dtype == np.float32 and d.dtype == np.float32
    assert np.isfinite(o).all() and np.isfinite(d).all(), "non-finite ray"
    assert (np.abs(d).max(axis=1) > 0).all(), "all-zero direction"
    assert (np.abs(o) <= np.float32(3.0 * scale)).all(), "origin farther than 3 * scale"


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def edge_rays(scale, seed=0):
    """float32 (o, d, fam): fam maps each name of FAMILIES to the indices of
    its rays.  788 rays."""
    rng = np.random.default_rng(1000 + seed)
    s = float(scale)
    cell = 2.0 * s / GRID
    O, D, fam = [], [], {}

    def add(name, o, d):
        o = np.asarray(o, np.float64).reshape(-1, 3)
        d = np.asarray(d, np.float64).reshape(-1, 3)
        n0 = sum(len(x) for x in O)
        O.append(o.astype(np.float32))
        D.append(d.astype(np.float32))
        fam[name] = np.concatenate([fam.get(name, np.zeros(0, np.int64)),
                                    np.arange(n0, n0 + len(o), dtype=np.int64)])

    # axis: d = +-e_i, the two zero components +0.0 in one copy, -0.0 in the other
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        for sgn in (1.0, -1.0):
            for kind in range(3):
                for zero in (0.0, -0.0):
                    n = 5
                    o = np.zeros((n, 3))
                    o[:, i] = -sgn * 3.0 * s
                    off = rng.uniform(-0.8 * s, 0.8 * s, (n, 2))
                    if kind == 1:       # on cell planes of the finest cascade
                        off = np.round(off / cell) * cell
                    elif kind == 2:     # one coordinate exactly 0
                        off[np.arange(n), rng.integers(0, 2, n)] = 0.0
                    o[:, j], o[:, k] = off[:, 0], off[:, 1]
                    d = np.full((n, 3), zero)
                    d[:, i] = sgn
                    add("axis", o, d)
    # planar: one zero component (+0.0 / -0.0), the other two random
    for i in range(3):
        for zero in (0.0, -0.0):
            n = 16
            p = rng.uniform(-0.8 * s, 0.8 * s, (n, 3))
            d = rng.normal(size=(n, 3))
            d[:, i] = 0.0
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            o = p - 1.5 * s * d
            d[:, i] = zero
            add("planar", o, d)
    # inside: the training march clamps t1 = 0 to NEAR_DISTANCE, the test
    # march starts at the negative entry time
    add("inside", rng.uniform(-0.9 * s, 0.9 * s, (96, 3)), _unit(rng, 96))
    # grazing: axis rays in a face plane of the box (off-axis coordinate
    # exactly +-scale: 0 * inf = NaN in the slab test) and along an edge (both
    # off-axis coordinates +-scale); and the same rays one float32 ulp inside
    # the box, which do march, through the outermost cells
    inner = float(np.nextafter(F(s), F(0)))
    for name, face in (("grazing_exact", s), ("grazing", inner)):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            for sgn in (1.0, -1.0):
                for edge in (False, True):
                    for side in (1.0, -1.0):
                        for zero in (0.0, -0.0):
                            o = np.zeros(3)
                            o[i] = -sgn * 2.0 * s
                            o[j] = side * face
                            o[k] = (side if rng.random() < 0.5 else -side) * face if edge \
                                else rng.uniform(-0.8 * s, 0.8 * s)
                            d = np.full(3, zero)
                            d[i] = sgn
                            add(name, o, d)
    # miss: synthetic rays pointing away from the box
    mo, md = S.rays(64, scale, seed=seed + 1)
    add("miss", mo, -md.astype(np.float64))
    # plain: the rays every other march test uses, as a control
    po, pd = S.rays(256, scale, seed=seed)
    add("plain", po, pd)
    o = np.ascontiguousarray(np.concatenate(O))
    d = np.ascontiguousarray(np.concatenate(D))
    check_in_bounds(o, d, scale)
    assert len(o) < 1024 and set(fam) == set(FAMILIES)
    return o, d, fam


def box(scale):
    return np.zeros((1, 3), np.float32), np.full((1, 3), scale, np.float32)


def oracle_hits(o, d, scale):
    """(B, 2) hits of the scene box as RayAABBIntersector returns them
    (t1 clamped to 0 at the entry; (-1, -1) for a miss)."""
    c, h = box(scale)
    _, ht, _ = oracle.ray_aabb_intersect(o, d, c, h, 1)
    return np.ascontiguousarray(ht[:, 0])


def near_clamp(hits):
    """ml_rendering.py:50: hits_t[(t1 >= 0) & (t1 < NEAR_DISTANCE), 0] = NEAR_DISTANCE"""
    hits = hits.copy()
    m = (hits[:, 0] >= 0) & (hits[:, 0] < NEAR_DISTANCE)
    hits[m, 0] = NEAR_DISTANCE
    return hits


def entry_hits(o, d, scale):
    """(B, 2) slab times WITHOUT the clamp of t1 to 0: negative t1 for an
    origin inside the box, as the reference's test-time march is handed for
    cameras inside the scene (raymarching.cu:364)."""
    with np.errstate(all="ignore"):
        inv = F(1) / d
        a = (F(-scale) - o) * inv
        b = (F(scale) - o) * inv
        near = np.fmax(np.fmax(np.fmin(a, b)[:, 0], np.fmin(a, b)[:, 1]), np.fmin(a, b)[:, 2])
        far = np.fmin(np.fmin(np.fmax(a, b)[:, 0], np.fmax(a, b)[:, 1]), np.fmax(a, b)[:, 2])
    out = np.stack([near, far], 1).astype(np.float32)
    out[~((near <= far) & (far > 0))] = -1.0
    return np.ascontiguousarray(out)


def dt_min(max_samples):
    return SQRT3 / F(max_samples)


def bounded_work(hits, max_samples):
    """max over rays of (t2 - t1) / dt_min: the number of t += dt steps any
    march of these hits can take (every step is at least dt_min)."""
    h = hits.astype(np.float64)
    live = h[:, 0] < h[:, 1]
    if not live.any():
        return 0.0
    return float(((h[live, 1] - h[live, 0]) / float(dt_min(max_samples))).max())


def _frozen(*arrs):
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def case_rays(scale):
    """edge_rays(scale) with the box hits, computed once per process and
    read-only: (o, d, fam, hits, hits_near, hits_entry).  hits is
    RayAABBIntersector's output, hits_near has the NEAR_DISTANCE clamp,
    hits_entry keeps the negative t1 of the `inside` family and is
    near-clamped for every other ray (the test-time march's input)."""
    o, d, fam = edge_rays(scale)
    hits = oracle_hits(o, d, scale)
    near = near_clamp(hits)
    entry = near.copy()
    ins = fam["inside"]
    entry[ins] = entry_hits(o[ins], d[ins], scale)
    _frozen(o, d, hits, near, entry, *fam.values())
    return o, d, fam, hits, near, entry


@functools.lru_cache(maxsize=None)
def case_bits(scale, p, n_models=1):
    return _frozen(S.bitfields(n_models, cascades_of(scale), p=p))[0]


@functools.lru_cache(maxsize=None)
def case_noise(n_models, n_rays):
    return _frozen(S.noise(n_models, n_rays))[0]


@functools.lru_cache(maxsize=None)
def oracle_train(scale, esf, p, max_samples):
    """oracle.raymarching_train on case_rays(scale): rays_a, xyz, dir, dt, t"""
    o, d, fam, _, near, _ = case_rays(scale)
    assert bounded_work(near, max_samples) <= 65536
    ra, x, dr, dl, ts, tot = oracle.raymarching_train(
        o, d, near, case_bits(scale, p)[0], cascades_of(scale), scale, esf,
        case_noise(1, len(o))[0], GRID, max_samples)
    assert tot == ra[:, 2].sum()
    return _frozen(ra, x, dr, dl, ts)


@functools.lru_cache(maxsize=None)
def oracle_fused(scale, esf, p, max_samples, n_models):
    """oracle.ml_march on case_rays(scale): counts [K, B], starts, xyz, t, dt"""
    o, d, fam, _, near, _ = case_rays(scale)
    assert bounded_work(near, max_samples) <= 65536
    c, h = box(scale)
    cnt, st, x, ts, dl, tot = oracle.ml_march(
        o, d, c[0], h[0], case_noise(n_models, len(o)), case_bits(scale, p, n_models),
        cascades_of(scale), scale, esf, GRID, max_samples, float(NEAR_DISTANCE))
    assert tot == cnt.sum()
    return _frozen(cnt, st, x, ts, dl)


def oracle_test_march(scale, esf, p, max_samples, n_samples, alive, hits):
    """oracle.raymarching_test; `hits` (B, 2) is advanced in place."""
    o, d = case_rays(scale)[:2]
    assert bounded_work(hits, max_samples) <= 65536
    return oracle.raymarching_test(o, d, hits, alive, case_bits(scale, p)[0], cascades_of(scale),
                                   scale, esf, GRID, max_samples, n_samples)


def check_coverage(counts, fam, max_samples, claims_cap, tag=""):
    """What every march case must contain, whatever edge_rays() becomes: rays
    with samples in every family that can have them, rays without, and rays at
    the cap where the case says so.  `grazing_exact` rays lie in a face plane:
    one slab gives (0 * inf = NaN, +-inf), fminf / fmaxf drop the NaN, both
    bounds of that slab are the same infinity and the ray misses."""
    counts = np.asarray(counts)
    for name in FAMILIES:
        n = counts[fam[name]]
        if name in ("miss", "grazing_exact"):
            assert (n == 0).all(), (tag, name)
        else:
            assert (n > 0).sum() >= 8, (tag, name, int((n > 0).sum()))
    assert (counts == 0).sum() >= 8, tag
    assert counts.max() <= max_samples, tag
    if claims_cap:
        assert (counts == max_samples).sum() >= 8, (tag, int((counts == max_samples).sum()))


def fma32(a, b, c):
    """Elementwise float32 fma(a, b, c), exactly rounded: the product is exact
    in float64, the float64 sum is made sticky (round to odd, from the TwoSum
    error), and 53 sticky bits round to 24 as the exact value does."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        r = p + c
        bb = r - p
        e = (p - (r - bb)) + (c - bb)
        fix = np.isfinite(r) & (e != 0) & ((np.atleast_1d(r).view(np.int64).reshape(r.shape) & 1) == 0)
        r = np.where(fix, np.nextafter(r, np.where(e > 0, np.inf, -np.inf)), r)
        return r.astype(np.float32)


def cells_occupied(xyz, ts, bits, cascades, scale, esf, max_samples, dt_scale=None,
                   grid_size=GRID):
    """Per sample: the occupancy bit of the cell raymarching.cu:207-220 queries
    at (xyz, t), and calc_dt(t); vectorised float32."""
    x = np.asarray(xyz, np.float32)
    t = np.asarray(ts, np.float32)
    lo = SQRT3 / F(max_samples)
    hi = SQRT3 * F(2) * F(scale if dt_scale is None else dt_scale) / F(grid_size)
    dt = np.fmax(lo, np.fmin(t * F(esf), hi))
    mx = np.abs(x).max(axis=1)
    mip_p = np.clip(np.frexp(mx)[1] + 1, 0, cascades - 1)
    mip_d = np.clip(np.frexp(dt * F(grid_size))[1], 0, cascades - 1)
    mip = np.maximum(mip_p, mip_d).astype(np.int64)
    mb = np.fmin(np.ldexp(F(1), mip - 1).astype(np.float32), F(scale))
    mbi = (F(1) / mb).astype(np.float32)
    v = F(0.5) * fma32(x, mbi[:, None], np.ones_like(x)) * F(grid_size)
    n = np.fmax(F(0), np.fmin(v, F(grid_size) - F(1))).astype(np.int64)
    idx = mip * grid_size ** 3 + (_expand_bits(n[:, 0]) | (_expand_bits(n[:, 1]) << 1) |
                                  (_expand_bits(n[:, 2]) << 2))
    occ = (np.asarray(bits)[idx // 8] >> (idx % 8).astype(np.uint8)) & 1
    return occ.astype(bool), dt


# ----------------------------------------------------------------------------
# the 64 step times of one chunk (rn_march.h march_ray_wave, esf == 0)
# ----------------------------------------------------------------------------
def d0_of(max_samples):
    """calc_dt(t, esf = 0, ...) = clamp(0, sqrt3 / max_samples, ...): the lower bound"""
    return dt_min(max_samples)


def chunk_ts_serial(tb, d0):
    """t_0 = tb, t_{j+1} = fl(t_j + d0): the reference's own additions."""
    t = np.empty(64, np.float32)
    t[0] = F(tb)
    d0 = F(d0)
    for j in range(63):
        t[j + 1] = t[j] + d0
    return t


def chunk_ts_closed(tb, d0):
    """The kernel's shortcut: s1 = tb + d0, r = s1 - tb, s2 = s1 + d0, bend =
    the next power of two above tb, t_j = fma(j, r, tb); None where the guard
    (s2 - s1 == r, tb > 0, every t_j < bend) rejects it.

    The fma is exactly rounded (fma32)."""
    tb, d0 = F(tb), F(d0)
    s1 = F(tb + d0)
    r = F(s1 - tb)
    s2 = F(s1 + d0)
    bits = np.array([tb], np.float32).view(np.uint32)
    bend = ((bits & np.uint32(0x7f800000)) + np.uint32(0x00800000)).view(np.float32)[0]
    tj = fma32(np.arange(64, dtype=np.float32), r, tb)
    if F(s2 - s1) == r and tb > 0 and np.all(tj < bend):
        return tj
    return None


# ----------------------------------------------------------------------------
# raymarching.cu:195-279 for one ray
# ----------------------------------------------------------------------------
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _fma(a, b, c):
    """a * b + c rounded once.  nvcc contracts the reference's multiply-adds
    (-fmad=true, its default); DESIGN.md's contraction policy lists the sites."""
    return F(_libm.fmaf(float(a), float(b), float(c)))


def _calc_dt(t, esf, max_samples, grid_size, scale):
    """raymarching.cu:11-13; helper_math.h clamp(f, a, b) = fmaxf(a, fminf(f, b))"""
    lo = SQRT3 / F(max_samples)
    hi = SQRT3 * F(2) * F(scale) / F(grid_size)
    return np.fmax(lo, np.fmin(F(t) * F(esf), hi))


def _expand_bits(v):
    v = (v * 0x00010001) & 0xFF0000FF
    v = (v * 0x00000101) & 0x0F00F00F
    v = (v * 0x00000011) & 0xC30C30C3
    v = (v * 0x00000005) & 0x49249249
    return v & 0xFFFFFFFF


def morton3d(x, y, z):
    """raymarching.cu:35-52"""
    return _expand_bits(x) | (_expand_bits(y) << 1) | (_expand_bits(z) << 2)


def _mip_from_pos(x, y, z, cascades):
    mx = np.fmax(np.abs(x), np.fmax(np.abs(y), np.abs(z)))
    e = int(np.frexp(mx)[1])
    return min(cascades - 1, max(0, e + 1))


def _mip_from_dt(dt, grid_size, cascades):
    e = int(np.frexp(F(dt * F(grid_size)))[1])
    return min(cascades - 1, max(0, e))


def cell_of(x, y, z, t, bits, cascades, scale, esf, grid_size, max_samples, dt_scale=None):
    """(mip, nx, ny, nz, occupied) of the query at a sample position
    (raymarching.cu:207-220)."""
    dt = _calc_dt(t, esf, max_samples, grid_size, scale if dt_scale is None else dt_scale)
    mip = max(_mip_from_pos(x, y, z, cascades), _mip_from_dt(dt, grid_size, cascades))
    mb = np.fmin(F(np.ldexp(F(1), mip - 1)), F(scale))
    mbi = F(1) / mb
    gs, gm1 = F(grid_size), F(grid_size) - F(1)
    n = [int(np.fmax(F(0), np.fmin(F(0.5) * _fma(v, mbi, F(1)) * gs, gm1))) for v in (x, y, z)]
    idx = mip * grid_size ** 3 + morton3d(*n)
    occ = bool(bits[idx // 8] & (1 << (idx % 8)))
    return mip, n[0], n[1], n[2], occ, mb, dt


def march_plain(o, d, hit, noise, bits, cascades, scale, esf, grid_size=GRID, max_samples=1024):
    """One ray of raymarching_train_kernel: returns (t, dt, xyz) of its
    samples as float32 arrays.  The count loop (:204-234) and the write loop
    (:245-279) visit the same samples, so one loop serves."""
    with np.errstate(all="ignore"):
        ox, oy, oz = (F(v) for v in o)
        dx, dy, dz = (F(v) for v in d)
        dxi, dyi, dzi = F(1) / dx, F(1) / dy, F(1) / dz
        gsi = F(1) / F(grid_size)
        t1, t2 = F(hit[0]), F(hit[1])
        if t1 >= 0:                                         # :195-198
            t1 = _fma(_calc_dt(t1, esf, max_samples, grid_size, scale), F(noise), t1)
        t, n = t1, 0
        ts, dts, xyz = [], [], []
        while 0 <= t and t < t2 and n < max_samples:        # :204
            x, y, z = _fma(t, dx, ox), _fma(t, dy, oy), _fma(t, dz, oz)
            mip, nx, ny, nz, occ, mb, dt = cell_of(x, y, z, t, bits, cascades, scale, esf,
                                                   grid_size, max_samples)
            if occ:                                         # :222-223, :263-268
                ts.append(t); dts.append(dt); xyz.append((x, y, z))
                t = F(t + dt)
                n += 1
                continue
            tq = []
            for nn, dv, dvi, v in ((nx, dx, dxi, x), (ny, dy, dyi, y), (nz, dz, dzi, z)):
                e = _fma(F(0.5), np.copysign(F(1), dv), F(nn) + F(0.5))     # :225-227
                e = _fma(F(e * gsi), F(2), F(-1))
                tq.append(F(_fma(e, mb, -v) * dvi))
            t_target = F(t + np.fmax(F(0), np.fmin(tq[0], np.fmin(tq[1], tq[2]))))
            while True:                                     # :230-232
                t = F(t + _calc_dt(t, esf, max_samples, grid_size, scale))
                if not t < t_target:
                    break
    return (np.array(ts, np.float32), np.array(dts, np.float32),
            np.array(xyz, np.float32).reshape(-1, 3))


# ----------------------------------------------------------------------------
# exact-size device buffers with a guard tail
# ----------------------------------------------------------------------------
class Guarded:
    """A device buffer of n elements followed by a tail of `tail` sentinels
    (NaN for floats, -7 for ints).  The whole buffer starts as sentinels, so a
    slot the kernel should have written and did not shows too.  check()
    asserts the tail still holds its sentinel bits and returns the first n
    elements as numpy."""
    TAIL = 64

    def __init__(self, shape, dtype, device, tail=TAIL):
        import torch
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.shape, self.n = shape, int(np.prod(shape))
        self.is_float = dtype.is_floating_point
        self.buf = torch.full((self.n + tail,), float("nan") if self.is_float else -7,
                              dtype=dtype, device=device)
        self._bits = self._raw(self.buf[self.n:]).clone()

    @staticmethod
    def _raw(t):
        import torch
        return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what=""):
        import torch
        assert torch.equal(self._raw(self.buf[self.n:]), self._bits), f"guard tail written: {what}"
        return self.buf[:self.n].reshape(self.shape).cpu().numpy()
