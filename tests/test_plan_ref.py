"""CPU: tests/plan_ref.py holds the families its table claims (the GPU file
test_gpu_plan.py runs whatever cases() returns, so a family lost here would be
lost there without a failure), and the restatement of the plan is consistent
with itself: perm a permutation of the valid samples, the chunk rows a
partition of the rays whose per-model counts add up, no chunk larger than the
scratch rows that rn_field_bwd_merged is given."""
import numpy as np
import pytest

import plan_ref as R

CASES = R.cases()


def _by_K(K):
    return [c for c in CASES if c["K"] == K]


def test_case_limits_and_layout():
    assert {c["K"] for c in CASES} == set(range(1, 9))
    for c in CASES:
        K, B = c["K"], c["B"]
        assert 1 <= B <= 64 and c["total"] <= 60000, c["name"]
        assert np.all(c["seg_base"] % R.SEG_ALIGN == 0)
        assert np.array_equal(c["seg_count"], c["counts"].sum(1))
        # (1025: past the march's 1024 samples, reachable through the C ABI only)
        assert c["counts"].max(initial=0) <= (1025 if c["name"] == "k2_unstaged" else 1024)
        # exclusive prefix inside every model's segment, segments disjoint and in order
        assert np.array_equal(c["offsets"], c["seg_base"][:, None] + np.cumsum(c["counts"], 1) - c["counts"])
        assert np.all(c["seg_base"][1:] >= c["seg_base"][:-1] + c["seg_count"][:-1])
        # NaN exactly where no valid sample lies
        valid = np.zeros(len(c["ts"]), bool)
        valid[R.sample_table(c["counts"], c["offsets"])[0]] = True
        assert np.array_equal(np.isfinite(c["ts"]), valid), c["name"]
        assert valid.sum() == c["total"]
        assert sorted(set(sum(c["fam"].values(), []))) == list(range(B))


def test_ts_strictly_increasing_inside_every_run():
    for c in CASES:
        for k in range(c["K"]):
            for r in range(c["B"]):
                run = c["ts"][c["offsets"][k, r]:c["offsets"][k, r] + c["counts"][k, r]]
                assert np.all(np.diff(run) > 0), (c["name"], k, r)


def test_k1_and_k2_families():
    assert sorted(R.ray_totals(R.case("k1")).tolist()) == [0, 1, 63, 64, 65, 1024]
    c = R.case("k2_merge")
    pairs = {tuple(int(v) for v in c["counts"][:, r]) for r in range(c["B"])}
    assert {(0, 0), (1, 1), (32, 32), (32, 33), (1, 1024), (1024, 1), (1024, 1024)} <= pairs
    assert any(a == 0 and b > 0 for a, b in pairs) and any(a > 0 and b == 0 for a, b in pairs)
    assert {64, 65, R.LDS} <= set(R.ray_totals(c).tolist())          # L = 1 -> 2 per lane; the full slice
    assert R.ray_totals(c).max() <= R.LDS                            # all of it on the merge path
    c = R.case("k2_unstaged")
    assert np.all(R.ray_totals(c) == 2049) and {"ties", "random"} <= set(c["fam"])


@pytest.mark.parametrize("K", range(1, 9))
def test_interleavings_at_every_K(K):
    c = R.case(f"inter_k{K}")
    assert set(R.KINDS) <= set(c["fam"])
    assert all(len(c["fam"][kind]) >= 2 for kind in R.KINDS)
    ties = set(R.all_ties_rays(c))
    assert ties and set(c["fam"]["all_ties"]) <= ties
    if K >= 2:
        t = c["ts"]
        r = c["fam"]["disjoint"][0]
        last = [t[c["offsets"][k, r] + c["counts"][k, r] - 1] for k in range(K)]
        first = [t[c["offsets"][k, r]] for k in range(K)]
        assert all(last[k] < first[k + 1] for k in range(K - 1))
        r = c["fam"]["disjoint_rev"][0]
        last = [t[c["offsets"][k, r] + c["counts"][k, r] - 1] for k in range(K)]
        first = [t[c["offsets"][k, r]] for k in range(K)]
        assert all(last[k + 1] < first[k] for k in range(K - 1))
        # blocks of ties between distinct values: t shared by several models, not by all of them
        r = c["fam"]["tie_blocks"][0]
        vals = np.concatenate([t[c["offsets"][k, r]:c["offsets"][k, r] + c["counts"][k, r]]
                               for k in range(K)])
        mult = np.unique(vals, return_counts=True)[1]
        assert (mult > 1).any() and (mult < K).any() and len(mult) > 8


@pytest.mark.parametrize("K", range(3, 9))
def test_multi_families(K):
    c = R.case(f"multi_k{K}")
    cnt, tot = c["counts"], R.ray_totals(c)
    for nm in ("empty_first", "empty_middle", "empty_last", "only_first", "only_middle", "only_last"):
        assert len(c["fam"][nm]) >= 1, nm
    for r in c["fam"]["empty_first"]:
        assert cnt[0, r] == 0 and np.all(cnt[1:, r] > 0)
    for r in c["fam"]["empty_last"]:
        assert cnt[K - 1, r] == 0 and np.all(cnt[:K - 1, r] > 0)
    for r in c["fam"]["empty_middle"]:
        assert (cnt[:, r] == 0).sum() == 1 and cnt[0, r] > 0 and cnt[K - 1, r] > 0
    for nm, k in (("only_first", 0), ("only_middle", K // 2), ("only_last", K - 1)):
        for r in c["fam"][nm]:
            assert cnt[k, r] > 0 and tot[r] == cnt[k, r]
    for t in (R.LDS - 1, R.LDS, R.LDS + 1):
        rays = c["fam"][f"tot_{t}"]
        assert len(rays) >= 2 and np.all(tot[rays] == t) and np.all(cnt[:, rays] > 0)
    assert (tot > R.LDS).sum() >= 3 and (tot == R.LDS).sum() >= 1
    assert any(tot[r] > R.LDS for r in R.all_ties_rays(c))          # ties on the global-memory path
    if K >= 4:
        r = c["fam"]["long_empty_middle"][0]
        assert tot[r] > R.LDS and cnt[1, r] == 0
    if K == 8:
        assert (R.ray_totals(R.case("k8_full")) == 8 * 1024).sum() >= 1


def test_empty_rays_blocks_and_tiny_totals():
    for K in (1, 2, 4):
        tot = R.ray_totals(R.case(f"empties_k{K}"))
        assert tot[0] == 0 and tot[-1] == 0 and tot.sum() > 0
        z = "".join("0" if v == 0 else "1" for v in tot[1:-1])
        assert "1000001" in z                                     # five empty rays in the middle
    assert all(R.case(f"none_k{K}")["total"] == 0 for K in (1, 2, 3))
    for B in (1, 5, 7):                                           # ragged last block: 4 and 2 waves
        assert B % 4 and B % 2
        assert {c["K"] for c in CASES if c["B"] == B} >= {1, 2, 3, 8}
    totals = {c["total"] for c in CASES}
    assert {0, 1, 15, 16, 17} <= totals and sum(2000 <= t <= 9000 for t in totals) >= 3
    for K in range(1, 9):
        assert any(R.all_ties_rays(c) for c in _by_K(K)), K


def test_box_rays_leave_the_box():
    """the prep check's rays: coordinates clamped to exactly 0 and exactly 1, and some inside"""
    for mn, ext in (((-0.5,) * 3, (1.0,) * 3), ((-16.0,) * 3, (32.0,) * 3), ((-0.5, -1.0, -1.5), (1.0, 2.0, 3.0))):
        seen = np.zeros(3, int)
        for c in CASES:
            if not c["total"]:
                continue
            perm, ms = R.merged_order(c["counts"], c["offsets"], c["ts"])
            o, d = R.box_rays(c, mn, ext)
            u = R.prep_rows(perm, R.ray_of_positions(ms), c["ts"], o, d, mn, ext)[:, :3].view(np.float32)
            assert np.all((u >= 0) & (u <= 1))
            seen += [(u == 0).sum(), (u == 1).sum(), ((u > 0) & (u < 1)).sum()]
        assert np.all(seen > 1000), seen


def test_merged_order_is_a_sorted_permutation():
    for c in CASES:
        perm, ms = R.merged_order(c["counts"], c["offsets"], c["ts"])
        smp, ray, mod = R.sample_table(c["counts"], c["offsets"])
        assert len(perm) == c["total"] == ms[-1] and ms[0] == 0
        assert np.array_equal(np.sort(perm), np.sort(smp)), c["name"]
        assert np.array_equal(np.diff(ms), R.ray_totals(c))
        # (ray, t, model) never decreases along perm
        model_of = np.zeros(len(c["ts"]), np.int64)
        model_of[smp] = mod
        ray_of = np.zeros(len(c["ts"]), np.int64)
        ray_of[smp] = ray
        assert np.array_equal(ray_of[perm], R.ray_of_positions(ms))
        t, m, rr = c["ts"][perm], model_of[perm], ray_of[perm]
        same = rr[1:] == rr[:-1]
        assert np.all(t[1:][same] >= t[:-1][same])
        tie = same & (t[1:] == t[:-1])
        assert np.all(m[1:][tie] > m[:-1][tie])


@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_chunk_rows_partition_and_fit(cfg):
    head_n, head, max_chunk, min_chunk, blocks = cfg
    for c in CASES:
        K, B = c["K"], c["B"]
        _, ms = R.merged_order(c["counts"], c["offsets"], c["ts"])
        bounds = R.chunk_bounds(c["total"], head_n, head, max_chunk, min_chunk, blocks)[0]
        n = len(bounds)
        first, rows = R.chunk_rows(ms, c["offsets"], c["seg_base"], c["seg_count"], bounds, n, K)
        assert rows.shape == (n, R.DESC) and len(first) == n + 1 and first[n] == B
        if n:
            # the rays [r0, r1) of the chunks partition [0, B)
            assert first[0] == 0 and np.all(np.diff(first) >= 0)
            assert np.array_equal(rows[:, 0], first[:-1]) and np.array_equal(rows[:, 1], first[1:])
        else:
            assert c["total"] == 0
        assert np.all(rows[:, 2:4] == 0) and np.all(rows[:, 4 + K:12] == 0) and np.all(rows[:, 12 + K:] == 0)
        cnt = rows[:, 12:12 + K]
        assert np.all(cnt >= 0)
        assert np.array_equal(cnt.sum(0), c["seg_count"]), c["name"]
        # every model's chunk ranges are contiguous from its base
        live = rows[:, 0] < B
        for k in range(K):
            a = rows[live, 4 + k].astype(np.int64)
            assert np.array_equal(a, c["seg_base"][k] + np.cumsum(cnt[live, k]) - cnt[live, k])
        # the scratch contract: a chunk's rows <= max_chunk + one ray
        assert cnt.sum(1).max(initial=0) <= max_chunk + R.ray_totals(c).max(), c["name"]
        # a truncated schedule is a prefix of the full one
        for keep in {0, min(1, n), n // 2, max(n - 1, 0)}:
            f2, r2 = R.chunk_rows(ms, c["offsets"], c["seg_base"], c["seg_count"], bounds, keep, K)
            assert np.array_equal(r2, rows[:keep]) and np.array_equal(f2, first[:keep + 1])
