"""GPU: the march's chain walk on structured occupancy grids.

The other march tests use random occupancy 0.5 and 1.0, where a chain element
is a short run or a short skip.  Here the 128^3 bitfield of every cascade is a
pattern: one occupied cell, slabs of 1, 2 and 3 cells alternating along x, a
full grid with one empty slab, half of the box empty, a 3-D checkerboard.  64
rays of march_ref.edge_rays (16 each of plain, axis, planar, inside) are marched
through them for march_ref.CONFIGS and max_samples 1, 63, 64, 65, 1024 by

  * rn_ml_march_count (staged) -> rn_scan_segments -> rn_ml_compact, K = 1, 2,
  * rn_raymarching_train_count -> scan -> rn_raymarching_train_write, K = 1,
  * rn_raymarching_test with n_samples 64, K = 1,

and counts and the bits of t, dt (xyz, dir where the path has them) and ray_of
are compared with the C oracle.  Outputs are exactly sized with a sentinel tail.

Coverage.  Before anything is launched each case places the oracle's samples
on the ray's own step sequence t_0 = t1, t_{k+1} = t_k + dt(t_k) (every sample
time must be one of them, bit for bit) and counts the rays with

  skip   an empty query whose cell exit lies beyond its 64-step chunk: a
         stretch without samples that starts before a multiple of 64 with an
         empty step (the step after a sample, or step 0, is always queried)
         and ends at or after it, at the next sample or, for a ray that
         stays below its cap, at the ray's last step;
  run    a run of occupied steps across a multiple of 64;
  capped the cap reached inside a run: max_samples samples, and the next step
         is inside [t1, t2) and occupied;
  none   no sample.

claims() says which of these a (pattern, configuration, max_samples) case must
show in at least 8 rays, and why.
"""
import functools

import numpy as np
import pytest
import torch

import march_ref as M
import oracle
from march_ref import Guarded
from radnerf_amd._lib import lib

pytestmark = pytest.mark.gpu

F = np.float32
F32, I32, I64 = torch.float32, torch.int32, torch.int64
PATTERNS = ("cell", "slab1", "slab2", "slab3", "full_gap", "half", "checker")
MAX_SAMPLES = (1, 63, 64, 65, 1024)
N_PER_FAMILY = 16
RAY_FAMILIES = ("plain", "axis", "planar", "inside")


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pattern_bits(name, cascades):
    """uint8 [cascades * 128^3 / 8]: the same pattern in every cascade, bit
    idx = mip * 128^3 + morton3d(x, y, z) (raymarching.cu:218-220)"""
    g = M.GRID
    x, y, z = np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij")
    if name == "cell":
        occ = (x == 70) & (y == 61) & (z == 66)
    elif name.startswith("slab"):
        occ = (x // int(name[4:])) % 2 == 0
    elif name == "full_gap":
        occ = x != 40
    elif name == "half":
        occ = x >= g // 2
    elif name == "checker":
        occ = (x + y + z) % 2 == 0
    flat = np.zeros(g ** 3, np.uint8)
    flat[M.morton3d(x.ravel(), y.ravel(), z.ravel())] = occ.ravel()
    one = np.packbits(flat, bitorder="little")
    out = np.tile(one, cascades)
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def rays64(scale):
    """(o, d, near, entry, fam): 16 rays spread over each of four families"""
    o, d, fam, _, near, entry = M.case_rays(scale)
    pick, sub = [], {}
    for name in RAY_FAMILIES:
        idx = fam[name][np.linspace(0, len(fam[name]) - 1, N_PER_FAMILY).astype(int)]
        sub[name] = np.arange(len(pick), len(pick) + len(idx))
        pick += list(idx)
    pick = np.array(pick)
    out = tuple(np.ascontiguousarray(a[pick]) for a in (o, d, near, entry))
    for a in out:
        a.flags.writeable = False
    M.check_in_bounds(out[0], out[1], scale)
    return out + (sub,)


@functools.lru_cache(maxsize=None)
def step_times(scale, esf, max_samples):
    """Per ray the times of its steps inside [t1, t2), from the jittered t1
    (raymarching.cu:195-198) by t += dt(t): list of float32 arrays."""
    o, d, near, _, _ = rays64(scale)
    noise = M.case_noise(1, len(o))[0]
    assert M.bounded_work(near, max_samples) <= 65536
    out = []
    for r in range(len(o)):
        t1, t2 = F(near[r, 0]), F(near[r, 1])
        seq = []
        if t1 >= 0:
            t = M._fma(M._calc_dt(t1, esf, max_samples, M.GRID, scale), F(noise[r]), t1)
            while t < t2:
                seq.append(t)
                t = F(t + M._calc_dt(t, esf, max_samples, M.GRID, scale))
        out.append(np.array(seq, np.float32))
    return out


@functools.lru_cache(maxsize=None)
def train_oracle(pattern, scale, esf, max_samples):
    o, d, near, _, _ = rays64(scale)
    C = M.cascades_of(scale)
    ra, x, dr, dl, ts, tot = oracle.raymarching_train(
        o, d, near, pattern_bits(pattern, C), C, scale, esf, M.case_noise(1, len(o))[0], M.GRID,
        max_samples)
    assert tot == ra[:, 2].sum()
    for a in (ra, x, dr, dl, ts):
        a.flags.writeable = False
    return ra, x, dr, dl, ts


def coverage(pattern, scale, esf, max_samples):
    """rays with (skip, run, capped, none), see the module docstring"""
    o, d, near, _, _ = rays64(scale)
    C = M.cascades_of(scale)
    ra, _, _, _, ts = train_oracle(pattern, scale, esf, max_samples)
    seqs = step_times(scale, esf, max_samples)
    bits = pattern_bits(pattern, C)
    skip = run = capped = none = 0
    for r in range(len(o)):
        n, s0 = int(ra[r, 2]), int(ra[r, 1])
        T, t = seqs[r], ts[s0:s0 + n]
        if n == 0:
            none += 1
            skip += len(T) > 64                         # step 0 is queried; nothing but empty steps
            continue
        k = np.searchsorted(T, t)
        assert k.max() < len(T) and np.array_equal(T[k].view(np.uint32), t.view(np.uint32)), \
            (pattern, r, "a sample time is not a step of the ray")
        prev = np.concatenate([[-1], k[:-1]])
        tail = n < max_samples and ((len(T) - 1) // 64) * 64 > k[-1] + 1
        skip += bool(((k // 64) * 64 > prev + 1).any() or tail)
        run += bool(((k == prev + 1) & (k % 64 == 0) & (k > 0)).any())
        if n == max_samples and k[-1] + 1 < len(T):
            tn = T[k[-1] + 1:k[-1] + 2]
            xyz = M.fma32(tn[:, None], d[r][None, :], o[r][None, :])
            capped += bool(M.cells_occupied(xyz, tn, bits, C, scale, esf, max_samples)[0][0])
    return skip, run, capped, none


def claims(pattern, scale, max_samples):
    """Which coverage a case must show in >= 8 of its 64 rays.

    A ray crosses the box in at most 2 sqrt(3) scale / dt_min steps, and
    dt_min = sqrt(3) / max_samples: at scale 0.5 that is max_samples steps, at
    1.5 three times as many; at scale 16 a ray from outside (t1 ~ 32) takes
    about 256 ln(t2 / t1) ~ 200 steps (march_ref.reaches_cap).
      skip   the stretch must hold a multiple of 64, so it is longer than 64
             steps or a long ray has many of them.  cell (all empty): rays
             longer than 64 steps, i.e. max_samples 1024, or >= 63 at the
             larger scales.  half: the empty half is 64 steps deep at
             max_samples 1024, and at scale 16 (16 units at dt ~ 0.1); at
             scale 1.5 and max_samples <= 65 it is 1.5 / 0.027 = 55 steps, no
             claim.  slabs and checker at 1024: ten or more boundaries per
             ray, half of the steps empty.
      run    a run that starts at step 0 crosses step 64 only with 65 samples,
             so max_samples >= 65.  full_gap and half (occupied for hundreds
             of steps) where rays are longer than 64 steps; slabs and checker
             at 1024 as above.
      capped more occupied steps than max_samples on a ray: never at scale 0.5
             (the chord is at most max_samples steps and one sample of
             max_samples 1 has no next step); full_gap and half at scale 1.5
             (three caps' worth of steps) and at scale 16 for caps below the
             ~200 steps, i.e. all but 1024.
      none   cell: the rays miss the one cell.  half: the 16 inside rays'
             origins are uniform in the box, so not claimed for them; the
             other patterns are met by every ray that crosses the box.
    """
    many = max_samples == 1024 or (scale > 0.5 and max_samples >= 63)      # rays of > 64 steps
    dense = pattern in ("full_gap", "half")
    mixed = pattern.startswith("slab") or pattern == "checker"
    return {
        "skip": (pattern == "cell" and many) or (mixed and max_samples == 1024)
                or (pattern == "half" and (max_samples == 1024 or (scale == 16.0 and max_samples >= 63))),
        "run": max_samples >= 65 and ((dense and many) or (mixed and max_samples == 1024)),
        "capped": dense and (scale == 1.5 or (scale == 16.0 and max_samples < 1024)),
        "none": pattern == "cell",
    }


CASES = [(p, s, e) for p in PATTERNS for (s, e) in M.CONFIGS]


def _check_coverage(pattern, scale, esf, max_samples):
    got = dict(zip(("skip", "run", "capped", "none"), coverage(pattern, scale, esf, max_samples)))
    for name, must in claims(pattern, scale, max_samples).items():
        if must:
            assert got[name] >= 8, (pattern, scale, max_samples, name, got)
    return got


# ----------------------------------------------------------------------------
# device helpers
# ----------------------------------------------------------------------------
def _st(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


def _g(a, cuda):
    return torch.tensor(np.asarray(a), device=cuda)


def _u(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, what):
    got, want = _u(got), _u(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1)) if len(got) else []
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first {bad[:5]}"


def _fused(cuda, pattern, scale, esf, max_samples, K):
    o, d, _, _, _ = rays64(scale)
    n, C, st, L = len(o), M.cascades_of(scale), _st(cuda), lib()
    other = PATTERNS[(PATTERNS.index(pattern) + 3) % len(PATTERNS)]
    bits = np.stack([pattern_bits(pattern, C), pattern_bits(other, C)][:K])
    noise = M.case_noise(K, n)
    c, h = M.box(scale)
    ocnt, _, _, ots, odl, tot = oracle.ml_march(o, d, c[0], h[0], noise, bits, C, scale, esf, M.GRID,
                                                max_samples, float(M.NEAR_DISTANCE))
    assert tot == ocnt.sum()
    go, gd, gc, gh = _g(o, cuda), _g(d, cuda), _g(c[0], cuda), _g(h[0], cuda)
    gb, gn = _g(bits, cuda), _g(noise, cuda)
    cnt = Guarded((K, n), I32, cuda)
    stage_ts, stage_dt = Guarded((K * n, max_samples), F32, cuda), Guarded((K * n, max_samples), F32, cuda)
    L.ml_march_count(go.data_ptr(), gd.data_ptr(), gc.data_ptr(), gh.data_ptr(), float(M.NEAR_DISTANCE),
                     gn.data_ptr(), gb.data_ptr(), bits.shape[1], K, C, scale, esf, M.GRID, max_samples,
                     n, cnt.ptr(), stage_ts.ptr(), stage_dt.ptr(), st)
    got = cnt.check("staged counts")
    assert np.array_equal(got, ocnt), (f"K {K} staged counts: rays "
                                       f"{np.argwhere(got != ocnt)[:6].tolist()} differ")
    used = np.arange(max_samples)[None, :] < ocnt.reshape(-1).astype(np.int64)[:, None]
    for name, stage in (("t", stage_ts), ("dt", stage_dt)):
        assert (_u(stage.check("stage " + name))[~used] == 0x7fc00000).all(), \
            f"stage {name}: a slot beyond the count was written"
    offsets = Guarded((K, n), I32, cuda)
    seg_base, seg_count, meta = Guarded(K, I32, cuda), Guarded(K, I32, cuda), Guarded(2, I32, cuda)
    L.scan_segments(cnt.ptr(), K, n, 1, offsets.ptr(), seg_base.ptr(), seg_count.ptr(), meta.ptr(), st)
    total = int(ocnt.sum())
    assert list(meta.check("meta")) == [total, total]
    ts, dl, ray_of = Guarded(total, F32, cuda), Guarded(total, F32, cuda), Guarded(total, I32, cuda)
    L.ml_compact(cnt.ptr(), offsets.ptr(), n, K, max_samples, stage_ts.ptr(), stage_dt.ptr(), ts.ptr(),
                 dl.ptr(), ray_of.ptr(), st)
    _eq(ts.check("t"), ots, f"K {K} t")
    _eq(dl.check("dt"), odl, f"K {K} dt")
    owner = np.concatenate([np.repeat(np.arange(n), ocnt[k]) for k in range(K)]) if total else []
    assert np.array_equal(ray_of.check("ray_of"), owner), f"K {K} ray_of"


def _dropin(cuda, pattern, scale, esf, max_samples):
    o, d, near, _, _ = rays64(scale)
    n, C, st, L = len(o), M.cascades_of(scale), _st(cuda), lib()
    ora, oxyz, odir, odl, ots = train_oracle(pattern, scale, esf, max_samples)
    go, gd, gh = _g(o, cuda), _g(d, cuda), _g(near, cuda)
    gb, gn = _g(pattern_bits(pattern, C), cuda), _g(M.case_noise(1, n)[0], cuda)
    args = (go.data_ptr(), gd.data_ptr(), gh.data_ptr(), gb.data_ptr(), C, scale, esf, gn.data_ptr(),
            M.GRID, max_samples, n)
    counts, offsets = Guarded(n, I32, cuda), Guarded(n, I32, cuda)
    seg_base, seg_count, meta = Guarded(1, I32, cuda), Guarded(1, I32, cuda), Guarded(2, I32, cuda)
    L.raymarching_train_count(*args, counts.ptr(), st)
    got = counts.check("counts")
    assert np.array_equal(got, ora[:, 2]), f"count pass: rays {np.flatnonzero(got != ora[:, 2])[:6]} differ"
    L.scan_segments(counts.ptr(), 1, n, 1, offsets.ptr(), seg_base.ptr(), seg_count.ptr(), meta.ptr(), st)
    total = int(ora[:, 2].sum())
    assert list(meta.check("meta")) == [total, total]
    rays_a = Guarded((n, 3), I64, cuda)
    xyzs, dirs = Guarded((total, 3), F32, cuda), Guarded((total, 3), F32, cuda)
    deltas, ts = Guarded(total, F32, cuda), Guarded(total, F32, cuda)
    L.raymarching_train_write(*args, counts.ptr(), offsets.ptr(), rays_a.ptr(), xyzs.ptr(), dirs.ptr(),
                              deltas.ptr(), ts.ptr(), st)
    assert np.array_equal(rays_a.check("rays_a"), ora)
    for name, buf, want in (("t", ts, ots), ("dt", deltas, odl), ("xyz", xyzs, oxyz), ("dir", dirs, odir)):
        _eq(buf.check(name), want, "drop-in " + name)


def _test_march(cuda, pattern, scale, esf, max_samples, n_samples=64):
    o, d, _, entry, _ = rays64(scale)
    n, C, st = len(o), M.cascades_of(scale), _st(cuda)
    assert M.bounded_work(entry, max_samples) <= 65536
    alive = np.arange(n, dtype=np.int64)
    oh = entry.copy()
    oxyz, odir, odl, ots, one = oracle.raymarching_test(o, d, oh, alive, pattern_bits(pattern, C), C,
                                                        scale, esf, M.GRID, max_samples, n_samples)
    go, gd, ga, gb = _g(o, cuda), _g(d, cuda), _g(alive, cuda), _g(pattern_bits(pattern, C), cuda)
    hits = Guarded(entry.shape, F32, cuda)
    hits.buf[:hits.n] = _g(entry, cuda).reshape(-1)
    xyz, dirs = Guarded((n, n_samples, 3), F32, cuda), Guarded((n, n_samples, 3), F32, cuda)
    dl, ts, ne = Guarded((n, n_samples), F32, cuda), Guarded((n, n_samples), F32, cuda), Guarded(n, I32, cuda)
    lib().raymarching_test(go.data_ptr(), gd.data_ptr(), hits.ptr(), ga.data_ptr(), n, gb.data_ptr(), C,
                           scale, esf, M.GRID, max_samples, n_samples, xyz.ptr(), dirs.ptr(), dl.ptr(),
                           ts.ptr(), ne.ptr(), st)
    assert np.array_equal(ne.check("n_eff"), one)
    used = np.arange(n_samples)[None, :] < one[:, None]
    for name, buf, want in (("t", ts, ots), ("dt", dl, odl), ("xyz", xyz, oxyz), ("dir", dirs, odir)):
        g, w = _u(buf.check(name)), _u(want)
        assert np.array_equal(g[used], w[used]), "test march " + name
        assert (g[~used] == 0x7fc00000).all(), f"test march {name}: a slot beyond n_eff was written"
    _eq(hits.check("hits_t"), oh, "hits_t in place")


@pytest.mark.parametrize("max_samples", MAX_SAMPLES)
@pytest.mark.parametrize("pattern,scale,esf", CASES)
def test_structured_grids(cuda, pattern, scale, esf, max_samples):
    _check_coverage(pattern, scale, esf, max_samples)       # from the oracle alone, before any launch
    for K in (1, 2):
        _fused(cuda, pattern, scale, esf, max_samples, K)
    _dropin(cuda, pattern, scale, esf, max_samples)
    _test_march(cuda, pattern, scale, esf, max_samples)
