"""The field's two MLPs (geo 32 -> 64 -> 17, rgb 32 -> 64 -> 64 -> 3, no bias,
ReLU; csrc/rn_field.h mlp_forward, csrc/field.hip bwd_window) restated in numpy
with fp64 sums, every value carrying a running bound on how far a correct
kernel may be from it (test code: the package does not import it; numpy only).

Taken as given (verified elsewhere, or bit-level facts): the f16 encoding (the
kernel's own cache, encode_ref.decode_cache; test_gpu_encode.py bar (a)), the
f16 weights, the fp32 directions and the fp32 seeds.  Everything else is
recomputed here.  What is shared with the kernels is only what is discrete:
where a value is rounded to f16, which power of two scales it, which unit a
ReLU mask belongs to, which row of the geo layer is output 0.

Forward (the rounding points of oracle.field_oracle.field_forward): hidden
activations and geo outputs 1..16 are f16, g0 and the rgb pre-activation stay
wide, sigma = exp(g0), rgb = sigmoid.  SH degree 4 in fp64 from the fp32
direction on ((d/|d| + 1)/2) 2 - 1, as sh_lane.

Bounds, e = 2^-24 (fp32 unit roundoff).
* A layer with k inputs, reference inputs x within b_in of the kernel's:
  the kernel's fp32 accumulator (exact f16 products, k fp32 additions in any
  order) lies within  a = |W| b_in + (k + 1) e |W| (|x| + b_in)  of v = W x.
* The stored f16 is the rounding of a value in [v - a, v + a]; rounding is
  monotone, so it lies in [rn16(v - a), rn16(v + a)] (ReLU, also monotone,
  applied to both ends), and its distance b to the reference's rn16(v) is the
  larger of the two gaps.  This is never more than the a + 2^-11 (|v| + a) +
  2^-25 of a rounding taken blindly, and it is 0 where the interval holds one
  f16 value.
* SH: x = d/|d| carries 3.5 e |x| from the norm (three products, two sums, the
  root, the division) and e from the + 1; the / 2, the fma(., 2, -1) are
  exact: 4.5 e.  A coefficient is a polynomial of degree <= 3 with
  sum |dY/d(x, y, z)| <= 2.9 on the sphere except for the two zonal degree-3
  terms at the poles (4.5), and 3 to 6 roundings of intermediates below 3:
  13 e + <= 3 e typical, 16 e = 2^-20 = s, the bar test_gpu_encode.py (a)
  derived the same way; the stored f16 lies in [rn16(Y - s), rn16(Y + s)].
  Where the fp64 coefficient is exactly 0.0 the kernel's is too, and s = 0
  there: an exact zero only comes from a factor that is an exact zero of the
  input (a zero component of the direction, or x^2 - y^2 at |x| = |y|), and
  the fp32 evaluation forms the same factor from the same fp32 inputs.
  This interval is cut by a second one, relative where a coefficient
  vanishes with a factor, from sh_lane's own fp32 x, y, z (sh_interval): near
  a pole, where |Y| < s, it decides the ReLU masks the first leaves open.
* sigma and rgb go through exp and the sigmoid by evaluating them at both ends
  of the interval, plus 4 ulp (2^-21 relative) for expf and the division.
* Every FINAL bound (what a test compares against) is twice this budget:
  Forward.geo_lo / geo_hi use 2 a, sigma_bound / rgb_bound and the Backward's
  *_bound fields carry the factor.  The running bounds do not.
The forward bounds are anchored where the kernels expose intermediates: the
geo net runs from the cache (b = 0) to the 16 geo features and sigma, two
layers; with geo_given (the kernel's own stored geo features, b = 0) the rgb
net runs from [SH, geo features] to rgb, three layers.

Backward: bwd_window step by step.  Seeds o_c = drgb_c y (1 - y) and
gsig = dsigma exp(clamp(g0, -15, 15)); per group of `group` consecutive samples
(256 in rn_field_bwd, 32 in rn_field_dinput) the rgb chain is scaled by the
power of two that maps the group's largest |o_c| into [8, 16), the geo chain
by that of the largest seed of both kinds; every dY is rounded to f16 in its
scaled domain by the interval rule above at the reference's own scale G, which
puts the subnormal floor 2^-25 / G where it belongs (with `floor` given, the
merged kernels' case whose grouping the plan decides: err + 2^-11 (|v| + err)
+ floor + the reference's own rounding); the rgb-path rows of dL/dgeo are
brought to the geo scale before their cast.  rounded=False leaves every dY
unrounded with the same bounds otherwise: the fp32 oracle's backward, whose
r16 passes gradients through, is compared with that form.
ReLU' uses the reference activation; where the kernel's activation interval
[lo, hi] contains both a zero and a positive value the mask is undecided and
the whole |dY| of that unit joins the bound (the sample is not excluded:
nothing can be excluded from a sum the kernel forms).
dW_l = sum_s dY_l (x) X_l per element with the bound
  sum_s (err(dY) |X| + |dY| err(X) + err(dY) err(X)) + n 2^-23 sum_s |dY| |X|.

Weight families, all f16-representable:
* dense(seed): synthetic.mlp_params rounded to f16, the production-like case.
* banded(b), b = 0..7.  The hidden layers (g1, r1, r2; 64 rows): weight [j, i]
  is non-zero where (i - j) mod 32 falls in the b-th eighth of 32, so 4 terms
  per dot product for 32 inputs and 8 for 64, and rows j and 32 + j read the
  same columns.  The two short layers: g2 [o, i] is non-zero where
  (o - i) mod 17 is b or b + 8 (and 16 in band 0), 7 or 8 terms per row and 2
  or 3 rows per column; r3 [c, i] where (i + b) mod 3 == c, 21 or 22 terms per
  row, one row per column (with the plain (i - j) rule a hidden unit feeds none
  of the 17 geo rows or 3 rgb rows in most bands and its slots could not be
  observed).  The union over b is every slot.  Tuned until the CPU power
  checks see every slot (tests/test_mlp_ref.py):
  - magnitudes in [0.26, 0.33] where row + column is even and 1.5 times that
    where it is odd, random sign: the two slots a swap exchanges (neighbours
    along a row in the forward fragments, along a column in the transposed
    ones) differ by 0.06 at least (with U[0.25, 0.5] eight pairs came out
    within 0.003 of each other and their swap could not be seen);
  - row 32 + j is minus row j, as in transparent_mlp: at every sample one
    unit of the pair is active, so no unit is dead (with independent rows a
    row of r2, whose inputs are ReLU outputs, drew eight negative weights, and
    the constant SH coefficient acted as a bias that silenced others);
  - r2 [j, 32 + i] has the sign opposite to r2 [j, i]: its inputs i and
    32 + i are the two ReLU branches of one value, so the unit's
    pre-activation changes sign with its inputs' (eight weights of one sign
    on non-negative inputs are a unit that is dead, or whose partner is);
  - column 0 of r1, the constant SH coefficient 0.282, is a quarter of the
    rest: at full size it is a bias that leaves one unit of a pair active at
    3 samples in 1000;
  - g1 times 4 and g2 times 2, so that the geo features are of the size of
    the SH coefficients (0.1 to 0.3) and their columns of r1 count.
* probe(shift): one non-zero term per dot product through all five layers,
  signed powers of two, units paired with opposite signs (rows j and 32 + j
  of g1 and r1 are +-c_j times unit vector j), so every hidden activation is
  exactly a power of two times an input: sigma = exp(+-2^k e16_i),
  rgb_c = sigmoid(+-2^k relu(+-x_i)) with x_i an SH coefficient: r3 row c
  reads unit PROBE_UNITS[(3 shift + c) mod 32], so shifts 0..10 bring every SH
  coefficient to an output with each sign.
"""
import types

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24
SH_S = 2.0 ** -20
FIELD_PARAMS = 9472
SIZES = {"g1": (64, 32), "g2": (17, 64), "r1": (64, 32), "r2": (64, 64), "r3": (3, 64)}
OFF = {"g1": 0, "g2": 2048, "r1": 3136, "r2": 5184, "r3": 9280}
LAYERS = ("g1", "g2", "r1", "r2", "r3")


def rn16(v):
    """round to nearest even f16 (subnormals included), as fp64"""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def split(flat):
    """one sub-NeRF's (9472,) master vector -> the five [out, in] fp64 matrices;
    the values must be f16-representable"""
    flat = np.asarray(flat)
    assert flat.shape == (FIELD_PARAMS,)
    w = flat.astype(np.float64)
    assert np.array_equal(rn16(w), w), "weights are not f16 values"
    return {k: w[OFF[k]:OFF[k] + r * c].reshape(r, c) for k, (r, c) in SIZES.items()}


def join(W):
    out = np.zeros(FIELD_PARAMS)
    for k, (r, c) in SIZES.items():
        out[OFF[k]:OFF[k] + r * c] = np.asarray(W[k], np.float64).reshape(-1)
    return out


def mat(flat, name):
    """layer `name` of a flat (9472,) vector as its [out, in] matrix"""
    r, c = SIZES[name]
    return np.asarray(flat)[OFF[name]:OFF[name] + r * c].reshape(r, c)


def where(p):
    """names flat parameter p: layer, row (output), column (input)"""
    for k in reversed(LAYERS):
        if p >= OFF[k]:
            r, c = divmod(int(p) - OFF[k], SIZES[k][1])
            return f"layer {k} row {r} column {c}"


# ---------------------------------------------------------------------------
# weight families
# ---------------------------------------------------------------------------
def dense(seed=5):
    from radnerf_amd import synthetic
    return synthetic.mlp_params(1, FIELD_PARAMS, seed=seed)[0].astype(np.float16).astype(F32)


def banded_mask(name, b):
    r, c = SIZES[name]
    j, i = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
    if name == "g2":
        d = (j - i) % 17
        return (d == b) | (d == b + 8) | ((d == 16) & (b == 0))
    if name == "r3":
        return (i + b) % 3 == j
    d = (i - j) % 32
    return (d >= 4 * b) & (d < 4 * (b + 1))


BANDED_GAIN = {"g1": 4.0, "g2": 2.0, "r1": 1.0, "r2": 1.0, "r3": 1.0}


def banded(b, seed=0):
    rng = np.random.default_rng(7000 + 16 * seed + b)
    out = np.zeros(FIELD_PARAMS, F32)
    for k, (r, c) in SIZES.items():
        j, i = np.meshgrid(np.arange(r), np.arange(c), indexing="ij")
        m = rng.uniform(0.26, 0.33, (r, c)) * np.where((i + j) & 1, 1.5, 1.0) * rng.choice([-1.0, 1.0], (r, c))
        if k == "r1":
            m[:, 0] *= 0.25
        if k == "r2":
            m[:, 32:] = -np.sign(m[:, :32]) * np.abs(m[:, 32:])
        if r == 64:
            m[32:] = -m[:32]
        m = m * BANDED_GAIN[k] * banded_mask(k, b)
        out[OFF[k]:OFF[k] + r * c] = m.astype(np.float16).astype(F32).reshape(-1)
    return out


# hidden units of r2 (= units of r1, identity wiring) that carry +SH_i (i) and -SH_i (32 + i)
PROBE_UNITS = tuple(range(16)) + tuple(range(32, 48))
PROBE_SHIFTS = tuple(range(11))


def probe_c(j):
    """first-layer factors of probe(): 1 on even, 2 on odd inputs"""
    return np.where(np.asarray(j) % 2 == 0, 1.0, 2.0)


def probe_wiring(shift):
    """The non-zero terms of probe(shift) past the paired first layers:
    g0 = s0 2^k0 h1[u0]; rgb_c = sigmoid(sc 2^kc r2[uc]), r2[u] = m_u r1[u];
    returns (u0, sign0, [(u_c, sign_c) for c in 0..2], m (64))."""
    u0 = 2 * (shift % 16) + 32 * ((shift // 16) % 2)           # an even input: c = 1
    s0 = 1.0 if shift % 2 == 0 else -1.0
    outs = [(PROBE_UNITS[(3 * shift + c) % 32], -1.0 if (c == 2 and shift % 2) else 1.0) for c in range(3)]
    j = np.arange(64)
    m = 2.0 ** ((j + shift) % 3)
    m = np.where((j % 8 == 7) & ((j % 32) >= 16), -m, m)        # a few dead units on the geo half
    return u0, s0, outs, m


def probe(shift, g0_gain=4.0, rgb_gain=1.0):
    W = {k: np.zeros(s) for k, s in SIZES.items()}
    u0, s0, outs, m = probe_wiring(shift)
    for j in range(32):
        W["g1"][j, j], W["g1"][32 + j, j] = probe_c(j), -probe_c(j)
        W["r1"][j, j], W["r1"][32 + j, j] = probe_c(j), -probe_c(j)
    W["g2"][0, u0] = s0 * g0_gain
    for o in range(1, 17):
        W["g2"][o, (4 * (o - 1) + shift) % 64] = (1.0 if (o + shift) % 2 == 0 else -1.0) * 2.0 ** (o % 3)
    for j in range(64):
        W["r2"][j, j] = m[j]
    for c, (u, s) in enumerate(outs):
        W["r3"][c, u] = s * rgb_gain
    flat = join(W).astype(F32)
    assert np.array_equal(rn16(flat), flat)
    return flat


def probe_saturated_sets():
    """name -> (9472,) fp32: probe weights with g0 beyond the TruncExp clamp in
    both signs, the rgb pre-activation beyond +-30, and a plain one"""
    return {"g0+": probe(2, g0_gain=512.0), "g0-": probe(3, g0_gain=512.0),
            "rgb+": probe(4, rgb_gain=8.0), "rgb-": probe(5, rgb_gain=8.0), "plain": probe(0)}


def probe_tight(b, n):
    """bar (c)'s tight bound of test_gpu_encode.py: (2^-9 + n 2^-23) sum |terms|"""
    return (2.0 ** -9 + n * 2.0 ** -23) * b.dW_mag


def weight_sets():
    """name -> (9472,) fp32: the sets the forward and dW tests run"""
    sets = {"dense": dense()}
    sets.update({f"banded{b}": banded(b) for b in range(8)})
    return sets


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
N_SAMPLES = 600                                   # three 256-sample iterations, the last ragged
INPUT_CASES = ((0.5, 0), (16.0, 0), (0.5, 1), (16.0, 1))      # (scale, directions seed) of the full-set runs
COUNTS = (1, 31, 32, 33, 255, 256, 257, N_SAMPLES)    # encode_ref.PREFIXES and the full set
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def directions(n, seed=0):
    """(n, 3) fp32, five classes in turn: unit vectors, lengths 1e-3..1e3, the
    six axis directions (exact zeros in SH), near-pole vectors (an axis plus
    1e-7..1e-2 off it), axis directions of other lengths.  Never zero."""
    rng = np.random.default_rng(4000 + seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = u.copy()
    i = np.arange(n)
    k = i % 5
    d[k == 1] *= 10.0 ** rng.uniform(-3, 3, (int((k == 1).sum()), 1))
    d[k == 2] = AXES[(i[k == 2] // 5) % 6]
    near = AXES[(i[k == 3] // 5) % 6] + u[k == 3] * 10.0 ** rng.uniform(-7, -2, (int((k == 3).sum()), 1))
    d[k == 3] = near
    d[k == 4] = AXES[(i[k == 4] // 5) % 6] * 10.0 ** rng.uniform(-3, 3, (int((k == 4).sum()), 1))
    d = d.astype(F32)
    assert np.all(np.abs(d).sum(1) > 0)
    return np.ascontiguousarray(d)


def seed_sets(n, seed=0):
    """name -> (dsigma (n), drgb (n, 3)) fp32: the backward's scale cases"""
    rng = np.random.default_rng(5000 + seed)
    ds = rng.normal(0, 1, n)
    dr = rng.normal(0, 1, (n, 3))
    z1, z3 = np.zeros(n), np.zeros((n, 3))
    sets = {"normal": (ds, dr), "dsigma_only": (ds, z3), "drgb_only": (z1, dr),
            "two_scales": (ds, dr * 2.0 ** -30)}
    hole = np.ones(n)
    hole[256:512] = 0                    # a whole iteration
    hole[32:64] = 0                      # whole tiles inside live iterations
    hole[128:192] = 0
    hole[544:576] = 0
    sets["zero_iter"] = (ds * hole, dr * hole[:, None])
    mag = np.ones(n)
    mag[:256], mag[512:] = 2.0 ** -40, 2.0 ** -20
    sets["steps"] = (ds * mag, dr * mag[:, None])
    for g, sl in enumerate((slice(0, 256), slice(256, 512), slice(512, None))):
        only = np.zeros(n)
        only[sl] = mag[sl]
        if only.any():
            sets[f"steps_group{g}"] = (ds * only, dr * only[:, None])
    return {k: (np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)) for k, (a, b) in sets.items()}


# ---------------------------------------------------------------------------
# SH degree 4
# ---------------------------------------------------------------------------
C1, C4, C6A, C6B = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999
C8, C9, C10, C11 = 0.54627421529603959, 0.59004358992664352, 2.8906114426405538, 0.45704579946446572
C12, C14 = 0.3731763325901154, 1.4453057213202769


def sh_input(d):
    """(q, |d|): fp64 ((d/|d| + 1)/2) 2 - 1 of fp32 directions (n, 3)"""
    d = np.asarray(d, F32).astype(np.float64)
    nrm = np.sqrt((d * d).sum(1, keepdims=True))
    return ((d / nrm + 1.0) / 2.0) * 2.0 - 1.0, nrm[:, 0]


def sh_input32(d):
    """sh_lane's own fp32 x, y, z (as fp64 values): every step there is one
    correctly rounded IEEE operation (no contraction, correctly rounded
    division and root), so numpy's fp32 arithmetic in the same order gives the
    same bits; the fma(t, 2, -1) is exact in fp64 and rounded once."""
    d = np.asarray(d, F32)
    n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    t = (d / n[:, None] + F32(1)) / F32(2)
    assert t.dtype == F32
    return (t.astype(np.float64) * 2.0 - 1.0).astype(F32).astype(np.float64)


def sh4_abs(q):
    """(n, 16): the sum of the magnitudes of each coefficient's monomials"""
    x, y, z = np.abs(q[:, 0]), np.abs(q[:, 1]), np.abs(q[:, 2])
    x2, y2, z2 = x * x, y * y, z * z
    return np.stack([np.full_like(x, 0.28209479177387814), C1 * y, C1 * z, C1 * x, C4 * x * y, C4 * y * z,
                     C6A * z2 + C6B, C4 * x * z, C8 * x2 + C8 * y2, C9 * y * (3.0 * x2 + y2), C10 * x * y * z,
                     C11 * y * (1.0 + 5.0 * z2), C12 * z * (5.0 * z2 + 3.0), C11 * x * (1.0 + 5.0 * z2),
                     C14 * z * (x2 + y2), C9 * x * (x2 + 3.0 * y2)], 1)


def sh_interval(dirs, relative=True):
    """(Y, lo, hi): the fp64 coefficients of the fp32 directions and the f16
    interval the kernel's stored coefficient must lie in: the issue's
    [rn16(Y - s), rn16(Y + s)], s = 2^-20 (0 where Y is exactly 0), cut by
    [rn16(Y' - s'), rn16(Y' + s')] with Y' the fp64 coefficients of sh_lane's
    own fp32 x, y, z (sh_input32) and s' = 8 e sum |monomials| (at most 6.5
    roundings on any path from x, y, z to a coefficient).  s' is relative
    where a coefficient vanishes with a factor: near a pole, where |Y| < s,
    the first interval straddles zero although the fp32 coefficient's sign,
    or its being exactly zero, is not in doubt; the second decides it.  The
    cut is never wider than the issue's interval.  relative=False: the first
    interval alone, all that holds for another fp32 evaluation of the
    coefficients (the torch oracle's, whose operations differ from sh_lane's)."""
    q, _ = sh_input(dirs)
    y = sh4(q)
    s = np.where(y == 0.0, 0.0, SH_S)
    if not relative:
        return y, rn16(y - s), rn16(y + s)
    q32 = sh_input32(dirs)
    y32, s32 = sh4(q32), 8.0 * EPS * sh4_abs(q32)
    lo = np.maximum(rn16(y - s), rn16(y32 - s32))
    hi = np.minimum(rn16(y + s), rn16(y32 + s32))
    assert np.all(lo <= hi), "the two SH intervals do not meet"
    return y, lo, hi


def sh4(q):
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    return np.stack([np.full_like(x, 0.28209479177387814), -C1 * y, C1 * z, -C1 * x, C4 * x * y,
                     -C4 * y * z, C6A * z2 - C6B, -C4 * x * z, C8 * x2 - C8 * y2,
                     C9 * y * (-3.0 * x2 + y2), C10 * x * y * z, C11 * y * (1.0 - 5.0 * z2),
                     C12 * z * (5.0 * z2 - 3.0), C11 * x * (1.0 - 5.0 * z2), C14 * z * (x2 - y2),
                     C9 * x * (-x2 + 3.0 * y2)], 1)


def sh4_jac(q):
    """(n, 16, 3) dY_i / d(x, y, z)"""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    o = np.zeros_like(x)
    J = [[o, o, o], [o, -C1 + o, o], [o, o, C1 + o], [-C1 + o, o, o], [C4 * y, C4 * x, o],
         [o, -C4 * z, -C4 * y], [o, o, 2 * C6A * z], [-C4 * z, o, -C4 * x], [2 * C8 * x, -2 * C8 * y, o],
         [-6 * C9 * x * y, C9 * (3 * y2 - 3 * x2), o], [C10 * y * z, C10 * x * z, C10 * x * y],
         [o, C11 * (1 - 5 * z2), -10 * C11 * y * z], [o, o, C12 * (15 * z2 - 3)],
         [C11 * (1 - 5 * z2), o, -10 * C11 * x * z], [2 * C14 * x * z, -2 * C14 * y * z, C14 * (x2 - y2)],
         [C9 * (3 * y2 - 3 * x2), 6 * C9 * x * y, o]]
    return np.stack([np.stack(r, 1) for r in J], 1)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
def _layer(W, x, bx):
    """(v, a): v = W x in fp64 and the bound a of the kernel's fp32 accumulator"""
    aW = np.abs(W)
    k = W.shape[1]
    return x @ W.T, bx @ aW.T + (k + 1) * EPS * ((np.abs(x) + bx) @ aW.T)


def _store16(v, a, relu):
    """the reference's stored f16 of v, the bound b of the kernel's against it,
    and the interval [lo, hi] of the kernel's (for the ReLU masks)"""
    x, lo, hi = rn16(v), rn16(v - a), rn16(v + a)
    if relu:
        x, lo, hi = np.maximum(x, 0.0), np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    return x, np.maximum(hi - x, x - lo), lo, hi


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def forward(e16, dirs, W, geo_given=None, mutate=None, sh_relative=True):
    """e16 (n, 32) f16 values, dirs (n, 3) fp32, W = split(...).  geo_given
    (n, 16): the kernel's stored geo features, taken as the rgb net's input
    (bound 0) instead of the reference's own.  mutate(name, v) -> v may alter a
    layer's pre-activation (the power checks).  sh_relative=False: the SH
    interval without its relative cut (sh_interval), for the oracle."""
    e = np.asarray(e16, np.float64)
    n = len(e)
    mut = mutate or (lambda name, v: v)
    f = types.SimpleNamespace(n=n, e=e)
    v, a = _layer(W["g1"], e, np.zeros_like(e))
    f.v_h1, f.a_h1 = mut("g1", v), a
    f.h1, f.b_h1, f.lo_h1, f.hi_h1 = _store16(f.v_h1, a, True)
    v, a = _layer(W["g2"], f.h1, f.b_h1)
    f.v_g, f.a_g = mut("g2", v), a
    f.g0, f.a_g0 = f.v_g[:, 0], a[:, 0]
    f.g16, f.b_g16, _, _ = _store16(f.v_g[:, 1:], a[:, 1:], False)
    f.geo_lo, f.geo_hi = rn16(f.v_g[:, 1:] - 2 * a[:, 1:]), rn16(f.v_g[:, 1:] + 2 * a[:, 1:])
    with np.errstate(over="ignore"):
        f.sigma = np.exp(f.g0)
        f.sigma_bound = 2.0 * (np.maximum(np.exp(f.g0 + f.a_g0) - f.sigma, f.sigma - np.exp(f.g0 - f.a_g0))
                               + 2.0 ** -21 * f.sigma)
    f.q, f.dnorm = sh_input(dirs)
    f.y_sh, f.sh_lo, f.sh_hi = sh_interval(dirs, sh_relative)
    f.sh = np.clip(rn16(f.y_sh), f.sh_lo, f.sh_hi)
    f.b_sh = np.maximum(f.sh_hi - f.sh, f.sh - f.sh_lo)
    if geo_given is None:
        geo, b_geo = f.g16, f.b_g16
    else:
        geo, b_geo = np.asarray(geo_given, np.float64), np.zeros((n, 16))
    f.xin, f.b_xin = np.concatenate([f.sh, geo], 1), np.concatenate([f.b_sh, b_geo], 1)
    v, a = _layer(W["r1"], f.xin, f.b_xin)
    f.v_r1, f.a_r1 = mut("r1", v), a
    f.r1, f.b_r1, f.lo_r1, f.hi_r1 = _store16(f.v_r1, a, True)
    v, a = _layer(W["r2"], f.r1, f.b_r1)
    f.v_r2, f.a_r2 = mut("r2", v), a
    f.r2, f.b_r2, f.lo_r2, f.hi_r2 = _store16(f.v_r2, a, True)
    v, a = _layer(W["r3"], f.r2, f.b_r2)
    f.out, f.a_out = mut("r3", v), a
    f.rgb = sigmoid(f.out)
    f.rgb_bound = 2.0 * (np.maximum(np.abs(sigmoid(f.out + a) - f.rgb), np.abs(sigmoid(f.out - a) - f.rgb))
                         + 2.0 ** -21 * f.rgb)
    return f


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def grad_scale(m):
    """rn_wave_grad_scale: the power of two that maps m into [8, 16)"""
    m = float(F32(m))
    if not (m > 0.0) or not np.isfinite(m):
        return 1.0
    e = int(np.frexp(m)[1])
    return 2.0 ** max(-100, min(100, 4 - e))


def _round_scaled(v, err, G, floor, rounded=True):
    """f16 rounding of v at scale G (n, 1): the reference's value x and the
    bound of the kernel's f16, the rounding of a value in [v - err, v + err],
    against it: the larger gap to the interval's rounded ends (monotone
    rounding, as in the forward).  With `floor` (the merged kernels, whose
    scale is not the reference's) the blind form err + 2^-11 (|v| + err) +
    floor + |x - v|.  rounded=False: no rounding at all (the fp32 oracle's
    backward), the bound passes through."""
    if not rounded:
        return v, err
    x = rn16(v * G) / G
    if floor is None:
        lo, hi = rn16((v - err) * G) / G, rn16((v + err) * G) / G
        return x, np.maximum(hi - x, x - lo)
    return x, err + 2.0 ** -11 * (np.abs(v) + err) + floor + np.abs(x - v)


def _masked(v, err, act, lo, hi, roll=False):
    on = act > 0
    und = (lo > 0) != (hi > 0)
    if roll:                                    # seeded defect: the mask of the other k-step
        idx = np.arange(act.shape[1]) ^ 16
        on = on[:, idx]
    return v * on, np.where(und, np.abs(v) + err, err * on)


def _dw(dy, ey, x, bx, n):
    val = dy.T @ x
    mag = np.abs(dy).T @ np.abs(x)
    return val, 2.0 * (ey.T @ (np.abs(x) + bx) + np.abs(dy).T @ bx + n * 2.0 ** -23 * mag), mag


DEFECTS = ("mask_kstep", "rgb_scale", "no_clamp", "no_remap")


def backward(f, W, dsigma, drgb, group=256, floor=None, defect=None, rounded=True):
    """bwd_window on the forward f.  Returns dW / dW_bound / dW_mag (9472),
    dE / dE_bound (n, 32), dSH / dSH_bound (n, 16), the seeds and scales.
    defect: one of DEFECTS, a wrong kernel restated (tests of the tests).  A
    fifth candidate, the rgb3 guard `row < 3` widened, is not among them: rows
    3..31 of that tile are dO's zero padding times r2, exact zeros, so the
    wider guard adds 0.0 to whatever follows the layer and changes no value."""
    assert defect is None or defect in DEFECTS
    n = f.n
    ds = np.asarray(dsigma, F32).astype(np.float64)
    dr = np.asarray(drgb, F32).astype(np.float64).reshape(n, 3)
    y = f.rgb
    sp = y * (1.0 - y)
    spe = np.maximum(np.abs(sigmoid(f.out + f.a_out) * (1 - sigmoid(f.out + f.a_out)) - sp),
                     np.abs(sigmoid(f.out - f.a_out) * (1 - sigmoid(f.out - f.a_out)) - sp))
    o = dr * sp
    # y carries 2^-22 y (expf, 1 + e, the division), 1 - y and the products 3 e
    e_o = np.abs(dr) * (spe + 2.0 ** -21 * y + 3 * EPS * sp) + f.a_out * f.a_out * np.abs(dr)
    clamp = (lambda v: v) if defect == "no_clamp" else (lambda v: np.clip(v, -15.0, 15.0))
    with np.errstate(over="ignore"):
        ex = np.exp(clamp(f.g0))
        gsig = ds * ex
        e_g = np.abs(ds) * (np.maximum(np.exp(clamp(f.g0 + f.a_g0)) - ex, ex - np.exp(clamp(f.g0 - f.a_g0)))
                            + 2.0 ** -21 * ex)
    # block scales
    R, G = np.ones((n, 1)), np.ones((n, 1))
    for s0 in range(0, n, group):
        sl = slice(s0, min(n, s0 + group))
        bmr = float(np.abs(o[sl].astype(F32)).max())
        bm = max(bmr, float(np.abs(gsig[sl].astype(F32)).max()))
        R[sl], G[sl] = grad_scale(bmr), grad_scale(bm)
    dO, e_dO = _round_scaled(o, e_o, R, floor, rounded)
    # rgb3 -> rgb2 -> rgb1
    v, a = _layer(W["r3"].T, dO, e_dO)
    v, a = _masked(v, a, f.r2, f.lo_r2, f.hi_r2)
    dR2, e_dR2 = _round_scaled(v, a, R, floor, rounded)
    v, a = _layer(W["r2"].T, dR2, e_dR2)
    v, a = _masked(v, a, f.r1, f.lo_r1, f.hi_r1, roll=defect == "mask_kstep")
    dR1, e_dR1 = _round_scaled(v, a, R, floor, rounded)
    v, a = _layer(W["r1"].T, dR1, e_dR1)                       # (n, 32): dSH | dgeo 1..16
    dSH, e_dSH = v[:, :16], a[:, :16]
    vg, ag = v[:, 16:], a[:, 16:]
    if defect == "rgb_scale":                                   # left at the rgb scale, read at the geo scale
        vg, ag = vg * (R / G), ag * (R / G)
    dG, e_dG = _round_scaled(np.concatenate([gsig[:, None], vg], 1),
                             np.concatenate([e_g[:, None], ag], 1), G, floor, rounded)
    # geo2 -> geo1
    v, a = _layer(W["g2"].T, dG, e_dG)
    v, a = _masked(v, a, f.h1, f.lo_h1, f.hi_h1)
    dH1, e_dH1 = _round_scaled(v, a, G, floor, rounded)
    dE, e_dE = _layer(W["g1"].T, dH1, e_dH1)
    parts = {"r3": _dw(dO, e_dO, f.r2, f.b_r2, n), "r2": _dw(dR2, e_dR2, f.r1, f.b_r1, n),
             "r1": _dw(dR1, e_dR1, f.xin, f.b_xin, n), "g2": _dw(dG, e_dG, f.h1, f.b_h1, n),
             "g1": _dw(dH1, e_dH1, f.e, np.zeros_like(f.e), n)}
    if defect == "no_remap":                                    # acc row r -> output r (row 16 dropped)
        val, bnd, mag = parts["g2"]
        parts["g2"] = (np.concatenate([val[1:], val[:1]]), bnd, mag)
    b = types.SimpleNamespace(o=o, gsig=gsig, R=R[:, 0], G=G[:, 0], dE=dE, dE_bound=2.0 * e_dE,
                              dSH=dSH, dSH_bound=2.0 * e_dSH, dG=dG, dR1=dR1, dR2=dR2, dH1=dH1, dO=dO)
    b.dW, b.dW_bound, b.dW_mag = (join({k: p[i] for k, p in parts.items()}) for i in range(3))
    return b
