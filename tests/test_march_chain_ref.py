"""CPU: the chunk step of march_ray_wave (rn_march.h) as a numpy model.

After the 64 parallel queries of a chunk every lane computes its own link of
the chain (the span of steps it marks, and the lane the chain visits next); a
short hop loop follows the links; the sample cap is applied after the loop.
new_chunk() restates that.  old_chunk() is a transcription of the scalar walk
it replaced: one iteration per run of occupied steps or per empty query, the
cap tested inside the loop.  Both are fed random and adversarial chunks, and
the new step, put into a whole-ray march, is compared with
march_ref.march_plain (the reference's serial loop).

What is compared when the cap is reached: the old walk stops inside the run
that reaches the cap, the new one follows the chain to the end of the chunk
and keeps the first cap - n marked occupied steps.  The ray ends there, so
marks behind the last emitted step and the carried `need` are not observable;
marks are compared up to that step, `need` when the cap is not reached, and
emitted masks, n and full always.
"""
import numpy as np
import pytest

import march_ref as M

F = np.float32
W = 64
INF = F(np.inf)
ALL = (1 << W) - 1


def _mask(bits):
    return sum(1 << j for j in range(W) if bits[j])


def _bits(lo, hi):
    """steps [lo, hi)"""
    return ((1 << int(hi)) - 1) & ~((1 << int(lo)) - 1)


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32),
                          np.asarray(b, np.float32).view(np.uint32)) or (np.isnan(a) and np.isnan(b))


# ----------------------------------------------------------------------------
# the scalar walk this replaced
# ----------------------------------------------------------------------------
def old_chunk(occ, alive, t, target, need, n, cap):
    occ = np.asarray(occ, bool) & np.asarray(alive, bool)
    mark, emitted, full = 0, 0, False
    cand = [j for j in range(W) if alive[j] and t[j] >= need]
    cur = cand[0] if cand else W
    capfree = n + W < cap
    while cur < W:
        if occ[cur]:
            stop = [j for j in range(cur, W) if not occ[j]]
            end = stop[0] if stop else W
            need = -INF
            if not capfree and n + emitted + (end - cur) >= cap:
                e2 = cur + (cap - n - emitted)
                mark |= _bits(cur, e2)
                emitted += e2 - cur
                full = True
                break
            mark |= _bits(cur, end)
            emitted += end - cur
            cur = end if end < W and alive[end] else W
        else:
            mark |= 1 << cur
            need = F(target[cur])
            nxt = [j for j in range(cur + 1, W) if alive[j] and t[j] >= need]
            cur = nxt[0] if nxt else W
    emit_m = mark & _mask(occ)
    return mark, emit_m, need, n + bin(emit_m).count("1"), full


# ----------------------------------------------------------------------------
# per-lane links, hop loop, need carry, post-loop cap
# ----------------------------------------------------------------------------
def lower_bound_lanes(key, target):
    """Per lane: the first j with key[j] >= target[lane] (64: none), by the
    kernel's search: six probes of the lanes' key values at lb + h - 1, then
    the last lane's key."""
    key, target = np.asarray(key, np.float32), np.asarray(target, np.float32)
    lb = np.zeros(W, np.int64)
    with np.errstate(invalid="ignore"):
        h = W // 2
        while h > 0:
            lb += np.where(key[lb + h - 1] >= target, 0, h)
            h //= 2
        lb += (lb == W - 1) & ~(key[W - 1] >= target)
    return lb


def lane_links(occ, alive, t, target):
    """(span_lo, span_hi, link) per lane: the chain marks steps
    [span_lo, span_hi) at this lane and visits lane `link` next (64: none)."""
    occ, alive = np.asarray(occ, bool), np.asarray(alive, bool)
    key = np.where(alive, np.asarray(t, np.float32), INF).astype(np.float32)
    lb = lower_bound_lanes(key, target)
    lo, hi, link = np.arange(W), np.zeros(W, np.int64), np.zeros(W, np.int64)
    for k in range(W):
        if occ[k]:
            stop = np.flatnonzero(~occ[k:])
            to = hi[k] = k + stop[0] if len(stop) else W
        else:
            hi[k] = k + 1
            to = max(lb[k], k + 1)
        link[k] = to if to < W and alive[to] else W
    return lo, hi, link


def new_chunk(occ, alive, t, target, need, n, cap):
    occ = np.asarray(occ, bool) & np.asarray(alive, bool)
    lo, hi, link = lane_links(occ, alive, t, target)
    cand = [j for j in range(W) if alive[j] and t[j] >= need]
    cur = cand[0] if cand else W
    mark, last = 0, -1
    while cur < W:
        mark |= _bits(lo[cur], hi[cur])
        last = cur
        cur = link[cur]
    if last >= 0:
        need = -INF if occ[last] else F(target[last])
    emit_m = mark & _mask(occ)
    room, found = cap - n, bin(emit_m).count("1")
    full = found >= room
    kept = 0
    for j in range(W):
        if (emit_m >> j) & 1 and bin(emit_m & ((1 << j) - 1)).count("1") < room:
            kept |= 1 << j
    return mark, kept, need, n + min(found, room), full


def check(occ, alive, t, target, need, n, cap, tag=""):
    assert n < cap
    o = old_chunk(occ, alive, t, target, need, n, cap)
    w = new_chunk(occ, alive, t, target, need, n, cap)
    assert o[1] == w[1], (tag, "emitted", hex(o[1]), hex(w[1]))
    assert o[3] == w[3] and o[4] == w[4], (tag, "n / full", o[3:], w[3:])
    if o[4]:
        upto = (1 << o[1].bit_length()) - 1          # steps up to the last emitted one
        assert o[0] & upto == w[0] & upto, (tag, "marks up to the cap", hex(o[0]), hex(w[0]))
    else:
        assert o[0] == w[0], (tag, "marks", hex(o[0]), hex(w[0]))
        assert _same(o[2], w[2]), (tag, "need", o[2], w[2])
    return w


def _chunk(rng, p_occ, n_alive, mean_skip, tb=None, d0=None, inf_frac=0.0, tie_frac=0.0):
    """A chunk as the kernel sees one: t non-decreasing, alive a prefix,
    target >= t (t + max(0, exit))."""
    d0 = F(d0 if d0 is not None else rng.uniform(1e-3, 2e-3))
    t = M.chunk_ts_serial(F(tb if tb is not None else rng.uniform(0.01, 3.0)), d0)
    alive = np.arange(W) < n_alive
    occ = (rng.random(W) < p_occ) & alive
    target = (t + (rng.exponential(mean_skip, W) * d0).astype(np.float32)).astype(np.float32)
    ties = rng.random(W) < tie_frac                         # exactly some later lane's t
    target[ties] = t[np.minimum(np.arange(W) + rng.integers(0, 12, W), W - 1)][ties]
    target[rng.random(W) < inf_frac] = INF
    return occ, alive, t, target


def test_lower_bound_search_is_exact():
    rng = np.random.default_rng(5)
    for _ in range(300):
        na = int(rng.integers(0, W + 1))
        t = np.sort(rng.uniform(0, 4, W)).astype(np.float32)
        t[rng.integers(0, W, 8)] = t[rng.integers(0, W)]    # repeated values
        t = np.sort(t)
        key = np.where(np.arange(W) < na, t, INF).astype(np.float32)
        target = rng.uniform(-1, 5, W).astype(np.float32)
        target[:8] = key[rng.integers(0, W, 8)]             # ties
        target[8], target[9], target[10] = INF, np.nan, -INF
        want = np.array([next((j for j in range(W) if key[j] >= x), W) for x in target])
        assert np.array_equal(lower_bound_lanes(key, target), want)


def test_random_chunks():
    rng = np.random.default_rng(11)
    full = some_need = 0
    for i in range(1500):
        na = int(rng.choice([W, W, W, rng.integers(0, W + 1)]))
        c = _chunk(rng, rng.choice([0.0, 0.2, 0.5, 0.8, 1.0]), na, rng.choice([0.5, 4.0, 30.0, 200.0]),
                   inf_frac=rng.choice([0.0, 0.05]), tie_frac=rng.choice([0.0, 0.3]))
        need = F(rng.choice([-np.inf, c[2][rng.integers(0, W)], c[2][-1] + F(1), np.inf]))
        n = int(rng.integers(0, 200))
        cap = n + int(rng.choice([1, 2, 5, 30, 63, 64, 65, 500]))
        w = check(*c, need, n, cap, i)
        full += w[4]
        some_need += np.isfinite(w[2])
    assert full >= 100 and some_need >= 100              # the inputs do reach both


def test_all_empty_targets_beyond_the_chunk():
    rng = np.random.default_rng(12)
    occ, alive, t, _ = _chunk(rng, 0.0, W, 1.0)
    for target in (np.full(W, t[-1] + F(1), np.float32), np.full(W, INF, np.float32)):
        mark, emit, need, n, full = check(occ, alive, t, target, -INF, 3, 10)
        assert mark == 1 and emit == 0 and n == 3 and not full and _same(need, target[0])
        # the carried need lies beyond this chunk too: no element, need unchanged
        mark, emit, need2, n, full = check(occ, alive, t, target, need, 3, 10)
        assert mark == 0 and _same(need2, need)


def test_target_equal_to_own_t_steps_to_the_next_lane():
    rng = np.random.default_rng(13)
    occ, alive, t, _ = _chunk(rng, 0.0, W, 1.0)
    mark, emit, need, n, full = check(occ, alive, t, t.copy(), -INF, 0, 5)
    assert mark == ALL and emit == 0 and _same(need, t[-1])       # link = lane + 1 every time
    lo, hi, link = lane_links(occ, alive, t, t.copy())
    assert np.array_equal(link, np.arange(1, W + 1))


def test_ties_land_on_the_tied_lane():
    rng = np.random.default_rng(14)
    occ, alive, t, target = _chunk(rng, 0.0, W, 1.0)
    for k, j in ((0, 1), (0, 63), (5, 40), (62, 63)):
        target[:] = INF
        target[k] = t[j]
        lo, hi, link = lane_links(occ, alive, t, target)
        assert link[k] == j
        check(occ, alive, t, target, -INF, 0, 9, (k, j))
        target[k] = np.nextafter(t[j], INF)                 # one ulp past the tie: the lane after
        assert lane_links(occ, alive, t, target)[2][k] == (j + 1 if j + 1 < W else W)
        check(occ, alive, t, target, -INF, 0, 9, (k, j))


@pytest.mark.parametrize("na", [0, 1, 2, 63, 64])
def test_alive_prefix_ends(na):
    rng = np.random.default_rng(15 + na)
    for p in (0.0, 0.5, 1.0):
        for _ in range(20):
            c = _chunk(rng, p, na, 3.0, tie_frac=0.2)
            w = check(*c, -INF, 0, 1024, (na, p))
            assert w[0] >> na == 0                          # nothing marked beyond the alive prefix
            if na == 0:
                assert w[0] == 0 and _same(w[2], -INF)


def test_caps_inside_runs():
    """A run of occupied steps [8, 40) after empty lanes: caps on its first,
    an inner and its last step, one beyond it, and n + E == cap exactly."""
    rng = np.random.default_rng(16)
    _, alive, t, target = _chunk(rng, 0.0, W, 1.0)
    occ = np.zeros(W, bool)
    occ[8:40] = True
    occ[50:60] = True
    target[:] = t                                           # every empty step is queried
    E = 42
    for n in (0, 7, 100):
        for room, want_full in ((1, True), (2, True), (17, True), (31, True), (32, True), (33, True),
                                (41, True), (E, True), (E + 1, False), (500, False)):
            mark, emit, need, n2, full = check(occ, alive, t, target, -INF, n, n + room, (n, room))
            assert full == want_full and n2 == n + min(room, E)
            lanes = np.flatnonzero(occ)[:min(room, E)]
            assert emit == sum(1 << int(j) for j in lanes)


def test_need_carry():
    rng = np.random.default_rng(17)
    occ, alive, t, target = _chunk(rng, 0.0, W, 1.0)
    # last element an occupied run to the chunk's end: -inf
    occ[:] = False
    occ[60:] = True
    target[:] = t
    assert _same(check(occ, alive, t, target, -INF, 0, 99)[2], -INF)
    # last element an empty query: its target, +inf included
    occ[:] = False
    target[63] = INF
    assert _same(check(occ, alive, t, target, -INF, 0, 99)[2], INF)
    # the chain enters at `need`, not at lane 0
    target[:] = t + F(100)
    mark = check(occ, alive, t, target, t[17], 0, 99)[0]
    assert mark == 1 << 17


# ----------------------------------------------------------------------------
# a whole ray through new_chunk against the reference's serial loop
# ----------------------------------------------------------------------------
def _queries(t, o, d, bits, cascades, scale, esf, max_samples):
    """occupancy, dt and skip target of the 64 steps (rn_march.h march_query),
    vectorised; the targets by raymarching.cu:225-230 with fused multiply-adds"""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        xyz = M.fma32(t[:, None], d[None, :], o[None, :])
        occ, dt = M.cells_occupied(xyz, t, bits, cascades, scale, esf, max_samples)
        mx = np.abs(xyz).max(axis=1)
        mip = np.maximum(np.clip(np.frexp(mx)[1] + 1, 0, cascades - 1),
                         np.clip(np.frexp(dt * F(M.GRID))[1], 0, cascades - 1)).astype(np.int64)
        mb = np.fmin(np.ldexp(F(1), mip - 1).astype(np.float32), F(scale))
        mbi = (F(1) / mb).astype(np.float32)
        v = F(0.5) * M.fma32(xyz, mbi[:, None], np.ones_like(xyz)) * F(M.GRID)
        n = np.fmax(F(0), np.fmin(v, F(M.GRID) - F(1))).astype(np.int64).astype(np.float32)
        e = M.fma32(np.full_like(xyz, 0.5), np.copysign(F(1), d)[None, :], n + F(0.5))
        e = M.fma32((e * (F(1) / F(M.GRID))).astype(np.float32), np.full_like(xyz, 2), np.full_like(xyz, -1))
        tq = (M.fma32(e, mb[:, None], -xyz) * (F(1) / d)[None, :]).astype(np.float32)
        skip = np.fmin(tq[:, 0], np.fmin(tq[:, 1], tq[:, 2]))
        target = (t + np.fmax(F(0), skip)).astype(np.float32)
    return occ, dt, xyz, target


def march_chunks(o, d, hit, noise, bits, cascades, scale, esf, max_samples):
    """march_ray_wave with new_chunk as its chunk step: (t, dt) of the samples"""
    t1, t2 = F(hit[0]), F(hit[1])
    if t1 >= 0:
        t1 = M._fma(M._calc_dt(t1, esf, max_samples, M.GRID, scale), F(noise), t1)
    ts, dts = [], []
    if not (0 <= t1 < t2):
        return np.array(ts, np.float32), np.array(dts, np.float32)
    tb, need, n = t1, -INF, 0
    while True:
        t = np.empty(W, np.float32)
        t[0] = tb
        for j in range(W - 1):
            t[j + 1] = t[j] + M._calc_dt(t[j], esf, max_samples, M.GRID, scale)
        alive = t < t2
        occ, dt, _, target = _queries(t, o, d, bits, cascades, scale, esf, max_samples)
        _, emit, need, n, full = new_chunk(occ, alive, t, target, need, n, max_samples)
        for j in range(W):
            if (emit >> j) & 1:
                ts.append(t[j]); dts.append(dt[j])
        if full or not alive.all():
            break
        tb = F(t[-1] + M._calc_dt(t[-1], esf, max_samples, M.GRID, scale))
        if not tb < t2:
            break
    assert n == len(ts)
    return np.array(ts, np.float32), np.array(dts, np.float32)


@pytest.mark.parametrize("scale,esf", M.CONFIGS)
def test_whole_ray_equals_march_plain(scale, esf):
    """8 rays per family of edge_rays, occupancy 0.5, caps 1024 and 65."""
    o, d, fam, _, near, _ = M.case_rays(scale)
    bits = M.case_bits(scale, 0.5)[0]
    noise = M.case_noise(1, len(o))[0]
    C = M.cascades_of(scale)
    with_samples = 0
    for name in M.FAMILIES:
        for r in fam[name][:8]:
            for ms in (1024, 65):
                want = M.march_plain(o[r], d[r], near[r], noise[r], bits, C, scale, esf, M.GRID, ms)
                got = march_chunks(o[r], d[r], near[r], noise[r], bits, C, scale, esf, ms)
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (name, r, ms)
                assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (name, r, ms)
                with_samples += len(want[0]) > 0
    assert with_samples >= 5 * 8
