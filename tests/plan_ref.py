"""Host restatement of rn_bwd_plan (csrc/field_plan.hip) and the inputs that
tests/test_gpu_plan.py feeds it by direct calls (numpy only).

The plan changes no arithmetic: it decides which sample every merged block
touches.  Its outputs are integers, or fp32 values that are bit-exact by
design, so everything here is compared for equality:

  merged_order   perm / mstart: samples by (ray, t, model), np.lexsort
  chunk_bounds   the merged-position bound of every chunk (chunk_plan)
  chunk_rows     chunk_first and the 20-word descriptors (rn_merge.h)
  prep_rows      the level forward's per-position input (unit x, y, z, id)
  cases          the input families: K = 1..8, every interleaving, ties,
                 empty runs and rays, rays around the plan's LDS slice

test_plan_ref.py (CPU) asserts that cases() holds what its table claims, so
the GPU file cannot lose a family quietly."""
import functools

import numpy as np

import march_ref

SEG_ALIGN = 128          # fused.py SEG_ALIGN: every model's segment starts on a multiple
KMAX = 8                 # rn_merge.h MB_KMAX
DESC = 20                # rn_merge.h CH_DESC
LDS = 2048               # field_plan.hip PLAN_LDS, PLANM_LDS: samples of a ray staged in LDS
DT = np.float32(2.0 ** -12)
# (head_chunks, head_size, max_chunk, min_chunk, balance_blocks) of the chunk-row checks
CONFIGS = ((0, 0, 64, 16, 0), (0, 0, 64, 64, 0), (3, 64, 64, 16, 3), (3, 48, 96, 16, 3),
           (0, 0, 96, 16, 5))


# ----------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------
def sample_table(counts, offsets):
    """(sample, ray, model) of every valid sample, model-major like the compact layout."""
    counts, offsets = np.asarray(counts, np.int64), np.asarray(offsets, np.int64)
    K, B = counts.shape
    n = counts.ravel()
    total = int(n.sum())
    within = np.arange(total) - np.repeat(np.cumsum(n) - n, n)
    smp = np.repeat(offsets.ravel(), n) + within
    ray = np.repeat(np.tile(np.arange(B), K), n)
    mod = np.repeat(np.repeat(np.arange(K), B), n)
    return smp, ray, mod


def merged_order(counts, offsets, ts):
    """perm [total] and mstart [B + 1] (mstart[B] = total): the samples ordered
    by ray, then t, ties by model."""
    smp, ray, mod = sample_table(counts, offsets)
    t = np.asarray(ts)[smp]
    assert np.isfinite(t).all(), "a valid sample reads a gap"
    order = np.lexsort((mod, t, ray))
    per_ray = np.asarray(counts, np.int64).sum(0)
    mstart = np.concatenate([[0], np.cumsum(per_ray)])
    return smp[order].astype(np.int32), mstart.astype(np.int32)


def chunk_bounds(total, head_n, head, max_chunk, min_chunk, blocks):
    """host restatement of field_plan.hip chunk_plan: the merged-position bound of
    every chunk (head chunks ramping from ~0 to head, big chunks over 15/16 of
    the work -- with blocks > 0 a multiple of blocks in number, each <=
    max_chunk -- then min_chunk)"""
    main_end = total - total // 16
    head_n = head_n if head > 0 and head * (head_n + 1) // 2 <= main_end else 0

    def hbound(c):
        return (head * c * (c + 1)) // (2 * head_n) if head_n else 0
    H = hbound(head_n)
    big, mm = max_chunk, 0
    if blocks > 0 and main_end > H:
        per = blocks * max_chunk
        mm = -(-(main_end - H) // per)
        big = min(max(-(-(main_end - H) // (blocks * mm)), min_chunk), max_chunk)
    c1 = head_n + ((main_end - H) // big if main_end > H else 0)

    def bound(c):
        if c < head_n:
            return hbound(c)
        if c <= c1:
            return H + (c - head_n) * big
        return H + (c1 - head_n) * big + (c - c1) * min_chunk
    rest = total - bound(c1)
    n = c1 + (-(-rest // min_chunk) if rest > 0 else 0)
    return [bound(c) for c in range(n)], c1 - head_n, big, mm


def chunk_rows(mstart, offsets, seg_base, seg_count, bounds, n_kept, K):
    """chunk_first [n_kept + 1] and the descriptor rows [n_kept][20] of the
    first n_kept chunks of the schedule `bounds` (all of it: n_kept =
    len(bounds)), restating rn_merge.h:

      words 0, 1     the chunk's rays [r0, r1): r0 the first ray whose merged
                     start reaches the chunk's bound, r1 the next chunk's r0;
                     the complete schedule ends at B
      words 2, 3     0
      word 4 + k     model k's first sample of the chunk, offsets[k][r0]
      word 12 + k    its count: up to offsets[k][r1], or to seg_base[k] +
                     seg_count[k] at r1 = B
      a chunk past the last ray (r0 = B), and every k >= K: zeros

    (A chunk with r0 = r1 < B -- a long ray spans several bounds -- has counts
    0 and keeps offsets[k][r0] as its first sample, by the rule above.)"""
    mstart, offsets = np.asarray(mstart, np.int64), np.asarray(offsets, np.int64)
    B = len(mstart) - 1
    assert 0 <= n_kept <= len(bounds) and offsets.shape == (K, B)
    first = np.searchsorted(mstart[:B], np.asarray(bounds[:n_kept + 1], np.int64), side="left")
    if n_kept == len(bounds):
        first = np.concatenate([first, [B]])
    first = first.astype(np.int32)
    rows = np.zeros((n_kept, DESC), np.int32)
    r0, r1 = first[:-1].astype(np.int64), first[1:].astype(np.int64)
    rows[:, 0], rows[:, 1] = r0, r1
    live = r0 < B
    for k in range(K):
        end = np.concatenate([offsets[k], [int(seg_base[k]) + int(seg_count[k])]])
        a0 = end[r0]                     # (r0 = B reads the end: masked below)
        rows[:, 4 + k] = np.where(live, a0, 0)
        rows[:, 4 + KMAX + k] = np.where(live, end[r1] - a0, 0)
    return first, rows


def prep_rows(perm, ray_of_position, ts, rays_o, rays_d, xyz_min, extent):
    """[total][4] uint32: the bits of (unit x, unit y, unit z) and the sample
    index of every merged position.  Position = fma(t, d, o) exactly rounded;
    unit coordinate min(max((v - mn) / ext, 0), 1) in float32 (rn_field.h
    unit_coord).  For power-of-two extents the kernel multiplies by 1 / ext,
    which gives the same float, so this one form covers both paths."""
    perm = np.asarray(perm, np.int64)
    ray = np.asarray(ray_of_position, np.int64)
    t = np.asarray(ts, np.float32)[perm][:, None]
    o, d = np.asarray(rays_o, np.float32)[ray], np.asarray(rays_d, np.float32)[ray]
    v = march_ref.fma32(np.broadcast_to(t, d.shape), d, o)
    mn, ext = np.asarray(xyz_min, np.float32), np.asarray(extent, np.float32)
    u = ((v - mn).astype(np.float32) / ext).astype(np.float32)
    u = np.minimum(np.maximum(u, np.float32(0)), np.float32(1)).astype(np.float32)
    out = np.empty((len(perm), 4), np.uint32)
    out[:, :3] = u.view(np.uint32)
    out[:, 3] = perm.astype(np.int32).view(np.uint32)
    return out


def ray_of_positions(mstart):
    """the ray of every merged position"""
    ms = np.asarray(mstart, np.int64)
    return np.repeat(np.arange(len(ms) - 1), np.diff(ms))


def box_rays(case, xyz_min, extent):
    """The case's rays (kept in unit-box coordinates) mapped into the box
    [xyz_min, xyz_min + extent): float32 inputs for the kernel and prep_rows
    alike.  About a third of the positions leave the box on some axis."""
    mn, ext = np.asarray(xyz_min, np.float32), np.asarray(extent, np.float32)
    o = (case["rays_o"] * ext + mn).astype(np.float32)
    d = (case["rays_d"] * ext).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
KINDS = ("disjoint", "disjoint_rev", "alternating", "ties", "tie_blocks", "random")


def make_runs(kind, ns, rng):
    """One ray's K runs of t (float32 multiples of 2^-12, strictly increasing
    inside every run), interleaved as `kind` says."""
    K = len(ns)
    if kind in ("disjoint", "disjoint_rev"):        # all of model 0 before model 1, or the reverse
        order = range(K) if kind == "disjoint" else range(K - 1, -1, -1)
        idx, j = [None] * K, 1
        for k in order:
            idx[k] = np.arange(j, j + ns[k])
            j += ns[k]
    elif kind == "alternating":                     # model k's i-th sample between k - 1's and k + 1's
        idx = [np.arange(n) * K + k + 1 for k, n in enumerate(ns)]
    elif kind == "ties":                            # the same t in every run (a prefix of the longest)
        idx = [np.arange(n) + 1 for n in ns]
    elif kind == "tie_blocks":                      # subsets of one short grid: ties among some models
        grid = max(max(ns) + max(ns) // 2, 1)
        idx = [np.sort(rng.choice(grid, n, replace=False)) + 1 for n in ns]
    elif kind == "random":                          # no ties
        pool = rng.permutation(4 * max(sum(ns), 1))
        cut = np.cumsum([0] + list(ns))
        idx = [np.sort(pool[cut[k]:cut[k + 1]]) + 1 for k in range(K)]
    else:
        raise ValueError(kind)
    return [(np.asarray(i, np.float32) * DT).astype(np.float32) for i in idx]


def _split(total, K, rng):
    """K positive counts (<= 1024) that sum to total"""
    while True:
        w = rng.random(K) + 0.25
        ns = np.floor(w / w.sum() * (total - K)).astype(int) + 1
        ns[0] += total - ns.sum()
        if ns.max() <= 1024 and ns.min() >= 1:
            return [int(n) for n in ns]


def build_case(name, K, rays, seed):
    """rays: list of (kind, counts per model, family names).  Model bases are
    128-aligned; ts holds NaN wherever no valid sample lies."""
    rng = np.random.default_rng(seed)
    B = len(rays)
    assert 1 <= B <= 64
    runs = [make_runs(kind, ns, rng) for kind, ns, _ in rays]
    counts = np.array([[len(runs[r][k]) for r in range(B)] for k in range(K)], np.int32).reshape(K, B)
    seg_count = counts.sum(1).astype(np.int32)
    seg_base = np.zeros(K, np.int32)
    for k in range(1, K):
        seg_base[k] = -(-(int(seg_base[k - 1]) + int(seg_count[k - 1])) // SEG_ALIGN) * SEG_ALIGN
    offsets = (seg_base[:, None] + np.cumsum(counts, 1) - counts).astype(np.int32)
    end = int(seg_base[-1]) + int(seg_count[-1])
    ts = np.full(max(-(-end // SEG_ALIGN) * SEG_ALIGN, SEG_ALIGN), np.nan, np.float32)
    for r in range(B):
        for k in range(K):
            ts[offsets[k, r]:offsets[k, r] + counts[k, r]] = runs[r][k]
    # rays in unit-box coordinates: unit position u0 + t * dv, leaving [0, 1] for some samples
    tmax = np.array([max([float(x[-1]) for x in rr if len(x)] + [1.0]) for rr in runs])
    u0 = rng.uniform(-0.2, 1.2, (B, 3))
    u1 = rng.uniform(-0.2, 1.2, (B, 3))
    fam = {}
    for r, (kind, _, names) in enumerate(rays):
        for nm in (kind,) + tuple(names):
            fam.setdefault(nm, []).append(r)
    case = dict(name=name, K=K, B=B, counts=counts, offsets=offsets, seg_base=seg_base,
                seg_count=seg_count, ts=ts, total=int(seg_count.sum()),
                rays_o=u0.astype(np.float32), rays_d=((u1 - u0) / tmax[:, None]).astype(np.float32),
                fam=fam)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _holes(K):
    """count patterns with empty models: (family name, 0 / 1 mask per model)"""
    out = [("empty_first", [0] + [1] * (K - 1)), ("empty_last", [1] * (K - 1) + [0])]
    if K >= 3:
        out.append(("empty_middle", [1] * (K // 2) + [0] + [1] * (K - K // 2 - 1)))
    for nm, k in (("only_first", 0), ("only_middle", K // 2), ("only_last", K - 1)):
        out.append((nm, [int(j == k) for j in range(K)]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every input family of the plan's direct test, as a tuple of cases (read-only arrays)."""
    rng = np.random.default_rng(11)
    out = []
    # K = 1: the rank path with nothing to rank against
    out.append(build_case("k1", 1, [("random", [n], ("k1",)) for n in (0, 1, 63, 64, 65, 1024)], 1))
    # K = 2, merge path: 64 / 65 merged samples straddle L = 1 -> 2 per lane; 2048 = PLAN_LDS
    pairs = [(0, 0), (0, 40), (40, 0), (1, 1), (32, 32), (32, 33), (1, 1024), (1024, 1), (1024, 1024)]
    out.append(build_case("k2_merge", 2, [("random", list(p), ("k2_merge",)) for p in pairs] +
                          [("tie_blocks", [32, 33], ("k2_merge",)), ("ties", [1024, 1024], ("k2_merge",))], 2))
    # K = 2 past the LDS slice: the rank path in global memory
    out.append(build_case("k2_unstaged", 2, [(kind, [1025, 1024], ("k2_unstaged",))
                                             for kind in ("random", "ties", "alternating", "tie_blocks")], 3))
    # interleavings at every K: equal counts (`ties` is then all ties) and ragged counts
    for K in range(1, 9):
        rays = []
        for kind in KINDS:
            rays.append((kind, [33] * K, ("all_ties",) if kind == "ties" else ()))
            rays.append((kind, [int(n) for n in rng.integers(1, 70, K)], ()))
        out.append(build_case(f"inter_k{K}", K, rays, 10 + K))
    # K = 3..8: empty models in every position, rays around the LDS slice
    for K in range(3, 9):
        rays = []
        for nm, mask in _holes(K):
            for kind in ("tie_blocks", "alternating"):
                rays.append((kind, [int(m * n) for m, n in zip(mask, rng.integers(20, 90, K))], (nm,)))
        for tot in (LDS - 1, LDS, LDS + 1):
            for kind in ("tie_blocks", "random"):
                rays.append((kind, _split(tot, K, rng), (f"tot_{tot}",)))
        # past the slice with an empty model and with ties only
        if K >= 4:                       # (two runs hold 2048 at the most)
            ns = _split(LDS + 200, K - 1, rng)
            rays.append(("tie_blocks", ns[:1] + [0] + ns[1:], ("long_empty_middle",)))
        rays.append(("ties", [700] * K, ("long", "all_ties")))
        out.append(build_case(f"multi_k{K}", K, rays, 20 + K))
    out.append(build_case("k8_full", 8, [("random", [1024] * 8, ("full",)),
                                         ("tie_blocks", [1024] * 8, ("full",)),
                                         ("alternating", [5] * 8, ())], 30))
    # empty rays: first and last, a run of five in the middle; no sample at all
    for K in (1, 2, 4):
        rays = [("random", [0] * K, ("empty_ray",))]
        rays += [("tie_blocks", [int(n) for n in rng.integers(0, 60, K)], ()) for _ in range(4)]
        rays += [("random", [0] * K, ("empty_ray",))] * 5
        rays += [("alternating", [int(n) for n in rng.integers(0, 60, K)], ()) for _ in range(4)]
        rays += [("random", [0] * K, ("empty_ray",))] * 2
        out.append(build_case(f"empties_k{K}", K, rays, 40 + K))
    for K in (1, 2, 3):
        out.append(build_case(f"none_k{K}", K, [("random", [0] * K, ("empty_ray",))] * 5, 50 + K))
    # B = 1, 5, 7: the last block of both kernels is ragged (4 and 2 waves a block)
    for K in (1, 2, 3, 8):
        for B in (1, 5, 7):
            rays = [(KINDS[int(rng.integers(len(KINDS)))], [int(n) for n in rng.integers(0, 50, K)],
                     ("ragged_block",)) for _ in range(B)]
            out.append(build_case(f"b{B}_k{K}", K, rays, 60 + 8 * B + K))
    # tiny totals around min_chunk = 16
    for tot in (1, 15, 16, 17):
        for K in (2, 3):
            cnt = np.zeros((7, K), int)
            for _ in range(tot):
                cnt[rng.integers(7), rng.integers(K)] += 1
            out.append(build_case(f"tot{tot}_k{K}", K,
                                  [("tie_blocks", [int(n) for n in row], ("tiny",)) for row in cnt],
                                  70 + 4 * tot + K))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def ray_totals(c):
    return c["counts"].astype(np.int64).sum(0)


def all_ties_rays(c):
    """rays with samples in at least two models whose non-empty runs are all the same run of t
    (K = 1: any ray with samples)"""
    out = []
    for r in range(c["B"]):
        runs = [c["ts"][c["offsets"][k, r]:c["offsets"][k, r] + c["counts"][k, r]]
                for k in range(c["K"]) if c["counts"][k, r]]
        if len(runs) >= min(2, c["K"]) and all(np.array_equal(x, runs[0]) for x in runs):
            out.append(r)
    return out
