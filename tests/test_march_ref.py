"""CPU: the march tests' own inputs and restatements (tests/march_ref.py).

Before anything runs on a GPU: the oracle finishes on edge_rays() in every
configuration tests/test_gpu_march.py uses, the inputs cover what those tests
claim, every march is bounded, the kernel's closed-form chunk times equal the
serial additions wherever its guard accepts, and a plain restatement of
raymarching.cu agrees with the C oracle on rays of every family.
"""
import numpy as np
import pytest

import march_ref as M


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_edge_rays_families(scale, esf):
    o, d, fam, hits, near, entry = M.case_rays(scale)
    M.check_in_bounds(o, d, scale)
    assert 600 <= len(o) < 1024
    assert sorted(np.concatenate(list(fam.values()))) == list(range(len(o)))
    zero = d == 0
    ax = fam["axis"]
    assert (zero[ax].sum(1) == 2).all()
    # both signs of zero, on every axis and in both directions
    neg = np.signbit(d) & zero
    for i in range(3):
        for sgn in (1.0, -1.0):
            m = d[ax, i] == sgn
            assert (neg[ax][m].sum(1) == 2).any() and (neg[ax][m].sum(1) == 0).any()
    assert (zero[fam["planar"]].sum(1) == 1).all() and neg[fam["planar"]].any()
    # origins on cell planes and with a coordinate exactly 0
    cell = 2.0 * scale / M.GRID
    on_plane = np.abs(o[ax] / cell - np.round(o[ax] / cell)) == 0
    assert (on_plane.sum(1) == 3).sum() >= 30 and ((o[ax] == 0).sum(1) >= 1).sum() >= 30
    assert (np.abs(o[fam["inside"]]) < scale).all()
    assert ((np.abs(o[fam["grazing_exact"]]) == np.float32(scale)).sum(1) >= 1).all()
    assert ((np.abs(o[fam["grazing_exact"]]) == np.float32(scale)).sum(1) == 2).any()
    # the box test itself: no NaN comes out, face-plane rays and misses miss,
    # inside rays enter at t1 = 0 (-> NEAR_DISTANCE) / at a negative time
    assert not np.isnan(hits).any()
    assert (hits[fam["grazing_exact"]] == -1).all() and (hits[fam["miss"]] == -1).all()
    assert (hits[fam["inside"], 0] == 0).all() and (near[fam["inside"], 0] == M.NEAR_DISTANCE).all()
    assert (entry[fam["inside"], 0] < 0).all() and (entry[fam["inside"], 1] > 0).all()
    assert np.array_equal(_u(entry[fam["inside"], 1]), _u(hits[fam["inside"], 1]))
    for name in ("axis", "planar", "grazing", "plain"):
        assert (hits[fam[name], 1] > hits[fam[name], 0]).all(), name


@pytest.mark.parametrize("scale,esf", M.CONFIGS)
@pytest.mark.parametrize("p", M.OCCUPANCY)
def test_oracle_train_runs_and_covers(scale, esf, p):
    """the drop-in training march cases of test_gpu_march.py (a)"""
    o, d, fam, hits, near, _ = M.case_rays(scale)
    for ms in M.CAPS:
        assert M.bounded_work(near, ms) <= 65536
        ra, x, dr, dl, ts = M.oracle_train(scale, esf, p, ms)
        assert not np.isnan(ts).any() and not np.isnan(x).any()
        M.check_coverage(ra[:, 2], fam, ms, M.reaches_cap(scale, p, ms), (scale, p, ms))
    if scale == 0.5:        # the cap cases other than 1 belong to the larger scales
        assert all(M.oracle_train(scale, esf, p, ms)[0][:, 2].max() < ms for ms in M.CAPS if ms > 1)


@pytest.mark.parametrize("scale,esf", M.CONFIGS)
@pytest.mark.parametrize("p", M.OCCUPANCY)
def test_oracle_fused_runs_and_covers(scale, esf, p):
    """the fused march cases of test_gpu_march.py (b)"""
    fam = M.case_rays(scale)[2]
    for K in (1, 3):
        for ms in M.FUSED_CAPS:
            cnt = M.oracle_fused(scale, esf, p, ms, K)[0]
            for k in range(K):
                M.check_coverage(cnt[k], fam, ms, M.reaches_cap(scale, p, ms), (scale, p, ms, K, k))


@pytest.mark.parametrize("scale,esf", M.CONFIGS)
@pytest.mark.parametrize("p", M.OCCUPANCY)
def test_oracle_test_march_runs_and_covers(scale, esf, p):
    """the test-time march cases of test_gpu_march.py (c) and (d): negative t1
    for the inside family; with n_samples = max_samples the count is the
    fused render's per-ray n_samples"""
    o, d, fam, _, _, entry = M.case_rays(scale)
    alive = np.arange(len(o), dtype=np.int64)
    assert (entry[fam["inside"], 0] < 0).sum() >= 8
    for ms in M.RENDER_CAPS:
        assert M.bounded_work(entry, ms) <= 65536
        h = entry.copy()
        x, dr, dl, ts, ne = M.oracle_test_march(scale, esf, p, ms, ms, alive, h)
        # at test time calc_dt gets `cascades` as its scale (raymarching.cu:370)
        M.check_coverage(ne, fam, ms, M.reaches_cap_test(scale, ms), (scale, p, ms))
        assert (ne[fam["inside"]] > 0).sum() >= 8


# ------------------------------------------------- closed form == serial adds
def test_fma32_is_libm_fmaf():
    rng = np.random.default_rng(0)
    n = 20000
    a = rng.normal(size=n).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, n)
    b = rng.normal(size=n).astype(np.float32)
    c = (-a * b * (1 + rng.normal(size=n) * 1e-3)).astype(np.float32)      # cancellation
    c[::3] = rng.normal(size=len(c[::3]))
    # products that land on float32 midpoints plus a tiny addend: the cases a
    # float64 sum rounded twice gets wrong
    a[:2000] = (1 + rng.integers(0, 2 ** 12, 2000) * 2.0 ** -12).astype(np.float32)
    b[:2000] = (1 + 2.0 ** -12 * (2 * rng.integers(0, 2 ** 11, 2000) + 1)).astype(np.float32)
    c[:2000] = (rng.choice([-1.0, 1.0], 2000) * 2.0 ** -60).astype(np.float32)
    got = M.fma32(a, b, c)
    want = np.array([M._fma(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(_u(got), _u(want))
    twice = (a.astype(np.float64) * b + c).astype(np.float32)
    assert (twice != want).any()            # the set does contain double-rounding cases


def test_chunk_closed_form_equals_serial_adds():
    """march_ray_wave's t_j = fma(j, r, tb) against the 63 additions it
    replaces, chained chunk by chunk as the kernel chains them (tb' = t_63 +
    d0), over many d0 = sqrt3 / max_samples and starts.  Bitwise wherever the
    guard accepts; both outcomes of the guard occur."""
    rng = np.random.default_rng(5)
    starts = [0.01, 0.25, 0.5, 1.0, 2.0] + list(rng.uniform(0.01, 2.0, 6))
    caps = sorted(set(range(16, 1100, 7)) | {64, 100, 128, 256, 512, 1024, 2048, 4096})
    n_chunks = n_acc = 0
    for ms in caps:
        d0 = M.d0_of(ms)
        for t1 in starts:
            tb = np.float32(t1)
            while tb < 4.0:
                ser = M.chunk_ts_serial(tb, d0)
                clo = M.chunk_ts_closed(tb, d0)
                n_chunks += 1
                if clo is not None:
                    n_acc += 1
                    assert np.array_equal(_u(clo), _u(ser)), (ms, t1, float(tb))
                tb = np.float32(ser[63] + d0)
    print(f"chunks {n_chunks}, accepted {n_acc}")
    assert n_acc >= 10000 and n_chunks - n_acc >= 1000
    # the guard's three parts each reject something
    assert M.chunk_ts_closed(np.float32(0.0), M.d0_of(1024)) is None            # tb > 0
    assert M.chunk_ts_closed(np.float32(0.99), M.d0_of(1024)) is None           # leaves the binade
    assert M.chunk_ts_closed(np.float32(-0.5), M.d0_of(1024)) is None           # NEG mode's t < 0


# ------------------------------------------------- second opinion on the oracle
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_march_plain_equals_oracle(scale, esf):
    """8 rays of every family: counts and the bits of t, dt and xyz."""
    p, ms = 0.5, 1024
    o, d, fam, _, near, _ = M.case_rays(scale)
    ra, x, dr, dl, ts = M.oracle_train(scale, esf, p, ms)
    bits, nz = M.case_bits(scale, p)[0], M.case_noise(1, len(o))[0]
    with_samples = 0
    for name in M.FAMILIES:
        idx = fam[name]
        for r in idx[np.linspace(0, len(idx) - 1, 8).astype(int)]:
            t, dt, xyz = M.march_plain(o[r], d[r], near[r], nz[r], bits, M.cascades_of(scale), scale,
                                       esf, M.GRID, ms)
            s0, n = int(ra[r, 1]), int(ra[r, 2])
            assert len(t) == n, (name, r, len(t), n)
            assert np.array_equal(_u(t), _u(ts[s0:s0 + n])), (name, r)
            assert np.array_equal(_u(dt), _u(dl[s0:s0 + n])), (name, r)
            assert np.array_equal(_u(xyz), _u(x[s0:s0 + n])), (name, r)
            with_samples += n > 0
    assert with_samples >= 30


@pytest.mark.parametrize("scale,esf", M.CONFIGS)
@pytest.mark.parametrize("ms", [65, 1024])
def test_oracle_sample_properties(scale, esf, ms):
    """Every sample of every ray: t strictly increasing, t1 <= t < t2, dt =
    calc_dt(t), xyz = fma(t, d, o), dir = d, and the cell at xyz is occupied."""
    p = 0.5
    o, d, fam, _, near, _ = M.case_rays(scale)
    ra, x, dr, dl, ts = M.oracle_train(scale, esf, p, ms)
    nz = M.case_noise(1, len(o))[0]
    ray = np.repeat(ra[:, 0], ra[:, 2])
    assert np.array_equal(ra[:, 1], np.cumsum(ra[:, 2]) - ra[:, 2])
    first = np.zeros(len(ts), bool)
    first[ra[ra[:, 2] > 0, 1]] = True
    assert (np.diff(ts)[~first[1:]] > 0).all()
    lo = M.SQRT3 / np.float32(ms)
    hi = M.SQRT3 * np.float32(2) * np.float32(scale) / np.float32(M.GRID)
    dt1 = np.fmax(lo, np.fmin(near[:, 0] * np.float32(esf), hi))
    t1 = M.fma32(dt1, nz, near[:, 0])
    assert (ts >= t1[ray]).all() and (ts < near[ray, 1]).all()
    occ, dt = M.cells_occupied(x, ts, M.case_bits(scale, p)[0], M.cascades_of(scale), scale, esf, ms)
    assert np.array_equal(_u(dt), _u(dl))
    assert occ.all()
    assert np.array_equal(_u(M.fma32(ts[:, None], d[ray], o[ray])), _u(x))
    assert np.array_equal(_u(dr), _u(d[ray]))
    # on a full grid the first sample is the jittered entry itself
    raf, _, _, _, tsf = M.oracle_train(scale, esf, 1.0, ms)
    assert np.array_equal(_u(tsf[raf[raf[:, 2] > 0, 1]]), _u(t1[raf[:, 2] > 0]))
