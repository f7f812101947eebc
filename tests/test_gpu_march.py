"""GPU: the occupancy-grid march at its edges, sample by sample.

rn_march.h / march.hip / the march inside render.hip against the CPU oracle on
march_ref.edge_rays(): zero direction components of both signs, origins inside
the box, on cell planes and on the box faces, misses.  Parts (a) to (d) are
bit-exact (counts, rays_a and the uint32 views of t, dt, xyz, dir); part (e)
compares the march backwards with fp64 segment sums under a derived bar.
Every output is exactly sized with a sentinel tail (march_ref.Guarded), every
case asserts its own coverage (march_ref.check_coverage), and every march is
bounded before it starts (march_ref.bounded_work; tests/test_march_ref.py runs
the same cases through the oracle on the CPU).
"""
import functools

import numpy as np
import pytest
import torch

import march_ref as M
import oracle
from march_ref import Guarded
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
SEG_ALIGN = 128          # fused.py SEG_ALIGN


def _st(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


def _g(a, cuda):
    return torch.tensor(np.asarray(a), device=cuda)         # copies (the cached inputs are read-only)


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq_bits(got, want, what):
    got, want = _u(got), _u(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1)) if len(got) else []
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first {bad[:5]}"


def _family_of(fam, r):
    return next(n for n, idx in fam.items() if r in idx)


def _eq_counts(got, want, fam, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} rays differ: " + ", ".join(
        f"ray {r} ({_family_of(fam, r)}) {got[r]} vs {want[r]}" for r in bad[:6]))


def _gpu_hits(cuda, o, d, scale):
    """rn_ray_aabb_intersect of the scene box, asserted bit-equal to the
    oracle's (face-plane rays with their 0 * inf = NaN slabs included)."""
    c, h = M.box(scale)
    n = len(o)
    cnt, ht, hi = Guarded(n, I32, cuda), Guarded((n, 1, 2), F32, cuda), Guarded((n, 1), I64, cuda)
    go, gd, gc, gh = _g(o, cuda), _g(d, cuda), _g(c, cuda), _g(h, cuda)
    lib().ray_aabb_intersect(go.data_ptr(), gd.data_ptr(), gc.data_ptr(), gh.data_ptr(), n, 1, 1,
                             cnt.ptr(), ht.ptr(), hi.ptr(), _st(cuda))
    ocnt, oht, ohi = oracle.ray_aabb_intersect(o, d, c, h, 1)
    assert np.array_equal(cnt.check("hit_cnt"), ocnt)
    got = ht.check("hits_t").reshape(n, 2)
    _eq_bits(got, oht.reshape(n, 2), "hits_t")
    assert np.array_equal(hi.check("hit_idx"), ohi)
    return go, gd, np.ascontiguousarray(got)


# ----------------------------------------------------- (a) drop-in training march
@pytest.mark.parametrize("max_samples", M.CAPS)
@pytest.mark.parametrize("p", M.OCCUPANCY)
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_train_march_edges(cuda, scale, esf, p, max_samples):
    """rn_raymarching_train_count -> rn_scan_segments -> rn_raymarching_train_write
    on edge_rays, hits from the GPU's own ray/AABB test: counts, rays_a and the
    bits of every sample's t, dt, xyz and dir equal the oracle's."""
    o, d, fam, _, near, _ = M.case_rays(scale)
    M.check_in_bounds(o, d, scale)
    n, C, st, L = len(o), M.cascades_of(scale), _st(cuda), lib()
    go, gd, hits = _gpu_hits(cuda, o, d, scale)
    h2 = M.near_clamp(hits)
    assert np.array_equal(_u(h2), _u(near))
    assert M.bounded_work(h2, max_samples) <= 65536
    ora, oxyz, odir, odl, ots = M.oracle_train(scale, esf, p, max_samples)
    M.check_coverage(ora[:, 2], fam, max_samples, M.reaches_cap(scale, p, max_samples))
    gh, gb = _g(h2, cuda), _g(M.case_bits(scale, p)[0], cuda)
    gn = _g(M.case_noise(1, n)[0], cuda)
    args = (go.data_ptr(), gd.data_ptr(), gh.data_ptr(), gb.data_ptr(), C, scale, esf,
            gn.data_ptr(), M.GRID, max_samples, n)
    counts, offsets = Guarded(n, I32, cuda), Guarded(n, I32, cuda)
    seg_base, seg_count, meta = Guarded(1, I32, cuda), Guarded(1, I32, cuda), Guarded(2, I32, cuda)
    L.raymarching_train_count(*args, counts.ptr(), st)
    _eq_counts(counts.check("counts"), ora[:, 2], fam, "count pass")
    L.scan_segments(counts.ptr(), 1, n, 1, offsets.ptr(), seg_base.ptr(), seg_count.ptr(),
                    meta.ptr(), st)
    total = int(ora[:, 2].sum())
    assert list(meta.check("meta")) == [total, total] and total > 0
    assert np.array_equal(offsets.check("offsets"), ora[:, 1])
    rays_a = Guarded((n, 3), I64, cuda)
    xyzs, dirs = Guarded((total, 3), F32, cuda), Guarded((total, 3), F32, cuda)
    deltas, ts = Guarded(total, F32, cuda), Guarded(total, F32, cuda)
    L.raymarching_train_write(*args, counts.ptr(), offsets.ptr(), rays_a.ptr(), xyzs.ptr(),
                              dirs.ptr(), deltas.ptr(), ts.ptr(), st)
    assert np.array_equal(rays_a.check("rays_a"), ora)
    ray = np.repeat(np.arange(n), ora[:, 2])
    for name, got, want in (("t", ts, ots), ("dt", deltas, odl), ("xyz", xyzs, oxyz),
                            ("dir", dirs, odir)):
        a, b = _u(got.check(name)), _u(want)
        bad = np.flatnonzero((a != b).reshape(total, -1).any(1))
        assert len(bad) == 0, (f"{name}: {len(bad)} samples differ, first at ray {ray[bad[0]]} "
                               f"({_family_of(fam, ray[bad[0]])})")
    assert np.array_equal(counts.check("counts after write"), ora[:, 2])


# ------------------------------------------------------------- (b) fused march
@pytest.mark.parametrize("max_samples", M.FUSED_CAPS)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("p", M.OCCUPANCY)
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_fused_march_edges(cuda, scale, esf, p, K, max_samples):
    """The staged path (rn_ml_march_count with staging -> scan -> rn_ml_compact)
    and the two-pass path (rn_ml_march_count without -> scan ->
    rn_ml_march_write) both equal oracle.ml_march and each other, bit for bit;
    staging slots at or beyond a ray's count keep their sentinel; ray_of is
    the owning ray.  K = 3 at max_samples 65 scans with fused.py's segment
    alignment (gaps between the segments keep their sentinel)."""
    o, d, fam, _, near, _ = M.case_rays(scale)
    M.check_in_bounds(o, d, scale)
    assert M.bounded_work(near, max_samples) <= 65536
    n, C, st, L = len(o), M.cascades_of(scale), _st(cuda), lib()
    align = SEG_ALIGN if (K == 3 and max_samples == 65) else 1
    ocnt, ostart, _, ots, odl = M.oracle_fused(scale, esf, p, max_samples, K)
    for k in range(K):
        M.check_coverage(ocnt[k], fam, max_samples, M.reaches_cap(scale, p, max_samples), k)
    c, h = M.box(scale)
    go, gd, gc, gh = _g(o, cuda), _g(d, cuda), _g(c[0], cuda), _g(h[0], cuda)
    bits = M.case_bits(scale, p, K)
    gb, gn = _g(bits, cuda), _g(M.case_noise(K, n), cuda)
    march = (go.data_ptr(), gd.data_ptr(), gc.data_ptr(), gh.data_ptr(), float(M.NEAR_DISTANCE),
             gn.data_ptr(), gb.data_ptr(), bits.shape[1], K, C, scale, esf, M.GRID, max_samples, n)
    # staged count, and the count alone
    cnt_s, cnt_c = Guarded((K, n), I32, cuda), Guarded((K, n), I32, cuda)
    stage_ts = Guarded((K * n, max_samples), F32, cuda)
    stage_dt = Guarded((K * n, max_samples), F32, cuda)
    L.ml_march_count(*march, cnt_s.ptr(), stage_ts.ptr(), stage_dt.ptr(), st)
    L.ml_march_count(*march, cnt_c.ptr(), None, None, st)
    for k in range(K):
        _eq_counts(cnt_s.check("staged counts")[k], ocnt[k], fam, f"staged count, model {k}")
        _eq_counts(cnt_c.check("counts")[k], ocnt[k], fam, f"count pass, model {k}")
    # staging: slot j of (k, ray) holds its sample j, or the sentinel
    flat = ocnt.reshape(-1).astype(np.int64)
    used = np.arange(max_samples)[None, :] < flat[:, None]
    for name, stage, want in (("t", stage_ts, ots), ("dt", stage_dt, odl)):
        s = _u(stage.check("stage " + name))
        assert (s[~used] == 0x7fc00000).all(), f"stage {name}: a slot beyond the count was written"
        assert np.array_equal(s[used], _u(want)), f"stage {name}"       # row-major = model-major
    # scan (the single block for K = 1, one block per segment for K = 3)
    offsets = Guarded((K, n), I32, cuda)
    seg_base, seg_count, meta = Guarded(K, I32, cuda), Guarded(K, I32, cuda), Guarded(2, I32, cuda)
    L.scan_segments(cnt_s.ptr(), K, n, align, offsets.ptr(), seg_base.ptr(), seg_count.ptr(),
                    meta.ptr(), st)
    seg_n = ocnt.sum(1).astype(np.int64)
    base = np.zeros(K, np.int64)
    for k in range(1, K):
        base[k] = -(-(base[k - 1] + seg_n[k - 1]) // align) * align
    end = int(-(-(base[-1] + seg_n[-1]) // align) * align)
    assert np.array_equal(seg_base.check("seg_base"), base)
    assert np.array_equal(seg_count.check("seg_count"), seg_n)
    assert list(meta.check("meta")) == [end, int(seg_n.sum())]
    want_off = base[:, None] + np.cumsum(ocnt, 1) - ocnt
    assert np.array_equal(offsets.check("offsets"), want_off)
    if align == 1:
        assert np.array_equal(want_off, ostart)
    else:
        assert end > seg_n.sum()                                # the alignment leaves gaps
    # where each oracle sample (dense, model-major) lands
    dst = np.concatenate([base[k] + np.arange(seg_n[k]) for k in range(K)])
    owner = np.concatenate([np.repeat(np.arange(n), ocnt[k]) for k in range(K)])
    gap = np.ones(end, bool)
    gap[dst] = False
    outs = {}
    for path in ("staged", "two-pass"):
        ts, dl, ray_of = Guarded(end, F32, cuda), Guarded(end, F32, cuda), Guarded(end, I32, cuda)
        if path == "staged":
            L.ml_compact(cnt_s.ptr(), offsets.ptr(), n, K, max_samples, stage_ts.ptr(),
                         stage_dt.ptr(), ts.ptr(), dl.ptr(), ray_of.ptr(), st)
        else:
            L.ml_march_write(*march, cnt_c.ptr(), offsets.ptr(), ts.ptr(), dl.ptr(), ray_of.ptr(), st)
        t_, d_, r_ = ts.check(path + " t"), dl.check(path + " dt"), ray_of.check(path + " ray_of")
        for name, got, want in (("t", t_, ots), ("dt", d_, odl)):
            bad = np.flatnonzero(_u(got)[dst] != _u(want))
            assert len(bad) == 0, (f"{path} {name}: {len(bad)} samples differ, first at ray "
                                   f"{owner[bad[0]]} ({_family_of(fam, owner[bad[0]])})")
            assert (_u(got)[gap] == 0x7fc00000).all(), f"{path} {name}: alignment gap written"
        assert np.array_equal(r_[dst], owner), f"{path} ray_of"
        assert (r_[gap] == -7).all()
        outs[path] = (t_, d_, r_)
    for a, b in zip(outs["staged"], outs["two-pass"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# -------------------------------------------------------- (c) test-time march
def _test_march(cuda, scale, esf, p, max_samples, n_samples, alive, g_hits):
    o, d = M.case_rays(scale)[:2]
    na, st = len(alive), _st(cuda)
    go, gd, ga = _g(o, cuda), _g(d, cuda), _g(alive, cuda)
    gb = _g(M.case_bits(scale, p)[0], cuda)
    xyz, dirs = Guarded((na, n_samples, 3), F32, cuda), Guarded((na, n_samples, 3), F32, cuda)
    dl, ts = Guarded((na, n_samples), F32, cuda), Guarded((na, n_samples), F32, cuda)
    ne = Guarded(na, I32, cuda)
    lib().raymarching_test(go.data_ptr(), gd.data_ptr(), g_hits.ptr(), ga.data_ptr(), na,
                           gb.data_ptr(), M.cascades_of(scale), scale, esf, M.GRID, max_samples,
                           n_samples, xyz.ptr(), dirs.ptr(), dl.ptr(), ts.ptr(), ne.ptr(), st)
    return (xyz.check("xyz"), dirs.check("dir"), dl.check("dt"), ts.check("t"), ne.check("n_eff"),
            g_hits.check("hits_t"))


def _alive(n, seed=3):
    """a permuted subset: two thirds of the rays"""
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(n)[:2 * n // 3]).astype(np.int64)


def _hits_buf(cuda, hits):
    g = Guarded(hits.shape, F32, cuda)
    g.buf[:g.n] = _g(hits, cuda).reshape(-1)
    return g


@pytest.mark.parametrize("n_samples", [1, 4, 64])
@pytest.mark.parametrize("p", M.OCCUPANCY)
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_test_march_edges(cuda, scale, esf, p, n_samples):
    """rn_raymarching_test from the unclamped hits of the inside family
    (negative t1) and the near-clamped hits of the rest, alive a permuted
    subset: samples, n_eff and the in-place hits_t equal the oracle's; slots
    at or beyond n_eff are not written."""
    max_samples = 1024
    o, d, fam, _, _, entry = M.case_rays(scale)
    M.check_in_bounds(o, d, scale)
    assert M.bounded_work(entry, max_samples) <= 65536
    alive = _alive(len(o))
    assert (entry[np.intersect1d(alive, fam["inside"]), 0] < 0).sum() >= 8
    oh = entry.copy()
    oxyz, odir, odl, ots, one = M.oracle_test_march(scale, esf, p, max_samples, n_samples, alive, oh)
    assert (one == n_samples).sum() >= 8 and (one == 0).sum() >= 8
    for name in ("axis", "planar", "inside", "grazing", "plain"):
        assert (one[np.isin(alive, fam[name])] > 0).sum() >= 8, name
    xyz, dirs, dl, ts, ne, hits = _test_march(cuda, scale, esf, p, max_samples, n_samples, alive,
                                              _hits_buf(cuda, entry))
    _eq_counts(ne, one, {k: np.flatnonzero(np.isin(alive, v)) for k, v in fam.items()}, "n_eff")
    used = np.arange(n_samples)[None, :] < one[:, None]
    for name, got, want in (("t", ts, ots), ("dt", dl, odl), ("xyz", xyz, oxyz), ("dir", dirs, odir)):
        g, w = _u(got), _u(want)
        assert np.array_equal(g[used], w[used]), name
        assert (g[~used] == 0x7fc00000).all(), f"{name}: a slot beyond n_eff was written"
    _eq_bits(hits, oh, "hits_t in place")
    assert (hits[alive, 0] != entry[alive, 0]).sum() >= 8       # it did advance


@pytest.mark.parametrize("max_samples,step", [(64, 1), (64, 4), (1024, 64)])
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_test_march_steps_concatenate(cuda, scale, esf, max_samples, step):
    """The reference's loop calls the test march with steps of 1 to 64 and
    carries t in hits_t: repeated calls with step s give the same samples as
    one call with n_samples = (max_samples // s + 2) * s, which is also the
    bound on the number of calls here.  The loop ends early, with every n_eff
    0, exactly when every ray has at most (calls - 1) * s samples; at scale
    0.5 (chord <= max_samples steps) it always does."""
    p = 0.5
    o, d, fam, _, _, entry = M.case_rays(scale)
    M.check_in_bounds(o, d, scale)
    assert M.bounded_work(entry, max_samples) <= 65536
    alive = _alive(len(o))
    assert (entry[np.intersect1d(alive, fam["inside"]), 0] < 0).sum() >= 8
    iters = max_samples // step + 2
    big = iters * step
    oh = entry.copy()
    oxyz, odir, odl, ots, one = M.oracle_test_march(scale, esf, p, max_samples, big, alive, oh)
    bxyz, bdir, bdl, bts, bne, bhits = _test_march(cuda, scale, esf, p, max_samples, big, alive,
                                                   _hits_buf(cuda, entry))
    assert np.array_equal(bne, one)
    _eq_bits(bhits, oh, "hits_t, one call")
    used = np.arange(big)[None, :] < one[:, None]
    assert np.array_equal(_u(bts)[used], _u(ots)[used]) and np.array_equal(_u(bxyz)[used], _u(oxyz)[used])
    g_hits = _hits_buf(cuda, entry)
    got = np.zeros(len(alive), np.int64)
    cat_t = np.full((len(alive), big), np.nan, np.float32)
    cat_dt = np.full((len(alive), big), np.nan, np.float32)
    cat_x = np.full((len(alive), big, 3), np.nan, np.float32)
    done = False
    for it in range(iters):
        xyz, dirs, dl, ts, ne, hits = _test_march(cuda, scale, esf, p, max_samples, step, alive, g_hits)
        if not ne.any():
            done = True
            break
        for j in range(step):
            m = ne > j
            cat_t[m, got[m] + j] = ts[m, j]
            cat_dt[m, got[m] + j] = dl[m, j]
            cat_x[m, got[m] + j] = xyz[m, j]
        got += ne
    assert done == bool(one.max() <= (iters - 1) * step), (done, it)
    assert done or scale > 0.5
    assert np.array_equal(got, one)
    for a, b in ((cat_t, bts), (cat_dt, bdl), (cat_x, bxyz)):
        assert np.array_equal(_u(a)[used], _u(b)[used])
    _eq_bits(g_hits.check("hits_t"), bhits, "hits_t, repeated calls")
    assert (one > step).sum() >= 8 and (one == 0).sum() >= 8


# ------------------------------------------- (d) the fused test-time render's march
@functools.lru_cache(maxsize=None)
def _model(cuda, scale, K, p):
    from radnerf_amd.networks import MNGP
    m = MNGP(scale, size=K, seed=3)
    bits = M.case_bits(scale, p, K)
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(S.mlp_params(K, LY.FIELD_PARAMS)))
    S.set_bitfields(m, bits)
    assert m.cascades == M.cascades_of(scale) and m.grid_size == M.GRID
    return m.to(cuda)


@pytest.mark.parametrize("max_samples", M.RENDER_CAPS)
@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_render_test_march_counts(cuda, scale, esf, max_samples):
    """rn_render_test with T_threshold = -1 (T <= thr never holds, so no early
    stop): a ray's n_samples is min(count, max_samples) of the test-time march
    from the same hits -- the tile-by-tile re-entry of march_ray_wave at
    cap <= 32, NEG mode included (inside rays start at t1 < 0)."""
    K, p = 2, 0.5
    o, d, fam, _, _, entry = M.case_rays(scale)
    M.check_in_bounds(o, d, scale)
    assert M.bounded_work(entry, max_samples) <= 65536
    n = len(o)
    alive = np.arange(n, dtype=np.int64)
    want = np.zeros((K, n), np.int32)
    for k in range(K):
        h = entry.copy()
        want[k] = oracle.raymarching_test(o, d, h, alive, M.case_bits(scale, p, K)[k],
                                          M.cascades_of(scale), scale, esf, M.GRID, max_samples,
                                          max_samples)[4]
        M.check_coverage(want[k], fam, max_samples, M.reaches_cap_test(scale, max_samples), k)
        assert (want[k][fam["inside"]] > 0).sum() >= 8 and (entry[fam["inside"], 0] < 0).all()
    if max_samples > 32 and (scale > 0.5 or max_samples == 1024):
        assert (want > 32).sum() >= 8                           # more than one tile
    m = _model(cuda, scale, K, p)
    bits = torch.stack([getattr(m, f"density_bitfield_{i}").view(-1) for i in range(K)]).contiguous()
    go, gd, gh = _g(o, cuda), _g(d, cuda), _g(entry, cuda)
    op, de = Guarded((K, n), F32, cuda), Guarded((K, n), F32, cuda)
    rgb, ns = Guarded((K, n, 3), F32, cuda), Guarded((K, n), I32, cuda)
    enc = m.xyz_encoder
    lib().render_test(go.data_ptr(), gd.data_ptr(), gh.data_ptr(), n, K, bits.data_ptr(),
                      bits.shape[1], m.cascades, float(scale), float(esf), m.grid_size, max_samples,
                      enc.params_f16().data_ptr(), *enc.level_ptrs(), m._h_min.ctypes.data,
                      m._h_ext.ctypes.data, m.packed_frags().data_ptr(), -1.0, op.ptr(), de.ptr(),
                      rgb.ptr(), ns.ptr(), max(1, min((n + 3) // 4, 512 // K)), _st(cuda))
    got = ns.check("n_samples")
    for k in range(K):
        _eq_counts(got[k], want[k], fam, f"n_samples, model {k}")
    # every ray's outputs were written (no sentinel left), rays without samples exactly 0
    o_, d_, c_ = op.check("opacity"), de.check("depth"), rgb.check("rgb")
    assert not np.isnan(o_).any() and not np.isnan(d_).any() and not np.isnan(c_).any()
    assert (o_[want == 0] == 0).all() and (c_[want == 0] == 0).all()


# ------------------------------------------------------- (e) march backwards
BW_COUNTS = (0, 1, 63, 64, 65, 1024)


def _bw_bar(n, terms_abs_sum):
    """(n + 2) 2^-24 sum |terms| for a segment of n samples: each of the n - 1
    additions of any summation order, the product and the inner addition of a
    term round once, relative to a partial sum bounded by sum |terms|."""
    return (n + 2) * 2.0 ** -24 * terms_abs_sum


def _segment_sums(gx, gd, ts, segs):
    """fp64: per row, sum gx and sum (gx t + gd) over the row's (start, n)
    pieces, with the sums of the terms' magnitudes"""
    gx, gd, ts = gx.astype(np.float64), gd.astype(np.float64), ts.astype(np.float64)
    R = len(segs)
    go, gdir, ao, ad = (np.zeros((R, 3)) for _ in range(4))
    for r, pieces in enumerate(segs):
        for s0, n in pieces:
            x, t = gx[s0:s0 + n], ts[s0:s0 + n, None]
            go[r] += x.sum(0)
            ao[r] += np.abs(x).sum(0)
            gdir[r] += (x * t + gd[s0:s0 + n]).sum(0)
            ad[r] += (np.abs(x * t) + np.abs(gd[s0:s0 + n])).sum(0)
    return go, gdir, ao, ad


def _bw_check(go, gdir, segs, ref, what):
    wo, wd, ao, ad = ref
    for r, pieces in enumerate(segs):
        n = sum(c for _, c in pieces)
        if n == 0:
            assert (_u(go[r]) == 0).all() and (_u(gdir[r]) == 0).all(), (what, r)     # +0.0 exactly
            continue
        eo, ed = np.abs(go[r] - wo[r]), np.abs(gdir[r] - wd[r])
        assert (eo <= _bw_bar(n, ao[r])).all(), (what, "d_o", r, n, eo, _bw_bar(n, ao[r]))
        assert (ed <= _bw_bar(n, ad[r])).all(), (what, "d_d", r, n, ed, _bw_bar(n, ad[r]))


def test_train_march_bw_segment_sums(cuda):
    """rn_raymarching_train_bw: rays_a rows in arbitrary order (as the
    reference's atomics leave them), counts 0, 1, 63, 64, 65, 1024 among them."""
    rng = np.random.default_rng(21)
    counts = np.concatenate([BW_COUNTS, BW_COUNTS, rng.integers(0, 200, 120)]).astype(np.int64)
    counts = counts[rng.permutation(len(counts))]
    starts = np.cumsum(counts) - counts
    N, R = int(counts.sum()), len(counts)
    gx = rng.normal(0, 1, (N, 3)).astype(np.float32)
    gd = rng.normal(0, 1, (N, 3)).astype(np.float32)
    ts = rng.uniform(0.01, 60, N).astype(np.float32)
    perm = rng.permutation(R)
    rays_a = np.stack([perm, starts[perm], counts[perm]], 1).astype(np.int64)
    segs = [[(int(s), int(c))] for _, s, c in rays_a]
    for c in BW_COUNTS:
        assert (rays_a[:, 2] == c).sum() >= 2
    go, gdir = Guarded((R, 3), F32, cuda), Guarded((R, 3), F32, cuda)
    dev = [_g(a, cuda) for a in (gx, gd, ts, rays_a)]        # held until the results are read
    lib().raymarching_train_bw(*(t.data_ptr() for t in dev), R, go.ptr(), gdir.ptr(), _st(cuda))
    _bw_check(go.check("d_o"), gdir.check("d_d"), segs, _segment_sums(gx, gd, ts, segs), "train_bw")


@pytest.mark.parametrize("K", [1, 3])
def test_ml_march_bw_segment_sums(cuda, K):
    """rn_ml_march_bw: per ray over the K sub-NeRFs' segments in the fused
    layout (model-major, segments aligned as fused.py scans them)."""
    rng = np.random.default_rng(22 + K)
    B = 150
    counts = rng.integers(0, 200, (K, B)).astype(np.int32)
    counts[:, :len(BW_COUNTS)] = 0
    counts[0, :len(BW_COUNTS)] = BW_COUNTS                  # rays whose total is exactly the count
    if K > 1:
        counts[1, 6:9] = (1, 63, 1024)                      # and rays that sum two models' segments
        counts[2, 6:9] = (63, 1, 1024)
    base, offsets = 0, np.zeros((K, B), np.int32)
    for k in range(K):
        offsets[k] = base + np.cumsum(counts[k]) - counts[k]
        base = -(-(base + int(counts[k].sum())) // SEG_ALIGN) * SEG_ALIGN
    N = base
    gx = rng.normal(0, 1, (N, 3)).astype(np.float32)
    gd = rng.normal(0, 1, (N, 3)).astype(np.float32)
    ts = rng.uniform(0.01, 60, N).astype(np.float32)
    segs = [[(int(offsets[k, r]), int(counts[k, r])) for k in range(K)] for r in range(B)]
    tot = counts.sum(0)
    for c in BW_COUNTS:
        assert (tot == c).any()
    go, gdir = Guarded((B, 3), F32, cuda), Guarded((B, 3), F32, cuda)
    dev = [_g(a, cuda) for a in (counts, offsets, ts, gx, gd)]
    lib().ml_march_bw(dev[0].data_ptr(), dev[1].data_ptr(), B, K, *(t.data_ptr() for t in dev[2:]),
                      go.ptr(), gdir.ptr(), _st(cuda))
    _bw_check(go.check("d_o"), gdir.check("d_d"), segs, _segment_sums(gx, gd, ts, segs), "ml_march_bw")
