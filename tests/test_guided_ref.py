"""CPU: the rule of error-guided sampling, checked on its numpy restatement
(tests/guided_ref.py) before any kernel is compared with it.

Geometry: 3 images of 37 x 21 with tile 16 -- 3 x 2 cells per image, the
right column 5 wide and the bottom row 5 tall.  The map holds values in
[0.001, 0.2] and one cell at 3.0.

  * the mixture density sums to exactly 1 over all pixels (Fractions);
  * sum p ray_weight = 1 to 1e-6 for uniform_frac 0, 0.5 and 1: the fp32
    weight carries a relative error of 2^-24 = 6e-8, the doubles before it
    1e-16 each, so the p-weighted sum is within 1e-7 of 1 (seen: 1 - 7e-9, 1 + 8e-9, 1 - 1e-16);
  * uniform_frac = 1 is sampler_ref.picks with weight exactly 1, and an
    all-ones map gives weight exactly 1 for any uniform_frac;
  * every pick is in range and cell_idx is the cell of the pick;
  * the hot cell's share of 2^14 rays is within 5 sigma of n p, counted from
    the picks alone (seed 11, step 5, uniform_frac 0.5: 7554 against 7554.2,
    sigma 63.8).
"""
from fractions import Fraction

import numpy as np
import pytest

import guided_ref as GR
import sampler_ref as SR
from radnerf_amd import sampler  # noqa: F401  (the API this restates: GuidedSampler)

N_IMG, W, H, TILE = 3, 37, 21, 16
HOT = 7


@pytest.fixture(scope="module")
def geo():
    assert hasattr(sampler, "GuidedSampler")
    return GR.Geometry(N_IMG, W, H, TILE)


@pytest.fixture(scope="module")
def emap(geo):
    rng = np.random.default_rng(3)
    e = rng.uniform(0.001, 0.2, geo.n_cells).astype(np.float32)
    e[HOT] = 3.0
    e.setflags(write=False)
    return e


def test_geometry(geo):
    assert (geo.tw, geo.th, geo.cpi, geo.n_cells) == (3, 2, 6, 18)
    npx = geo.n_px()
    assert list(npx[:6]) == [256, 256, 80, 80, 80, 25]
    assert int(npx.sum()) == N_IMG * W * H
    # every pixel lies in the cell cell_of names, and each cell gets n_px of them
    img, pix = np.divmod(np.arange(N_IMG * W * H), W * H)
    cells = geo.cell_of(img, pix)
    assert np.array_equal(np.bincount(cells, minlength=geo.n_cells), npx)


def test_weights_and_cdf(geo, emap):
    w, cdf = GR.weights(emap, geo)
    assert w.dtype == np.uint32 and cdf.dtype == np.uint64
    assert int(w[HOT]) == 3 * 65536 and int(w.min()) >= 1
    total = sum(int(a) * int(b) for a, b in zip(w, geo.n_px()))
    assert int(cdf[-1]) == total
    # the clamps: 0 and NaN -> 1, 300 -> 2^24
    e = emap.copy()
    e[0], e[1], e[2] = 0.0, 300.0, np.nan
    w2, _ = GR.weights(e, geo)
    assert (int(w2[0]), int(w2[1]), int(w2[2])) == (1, 1 << 24, 1)


@pytest.mark.parametrize("frac", [0.0, 0.5, 1.0])
def test_density_sums_to_one(geo, emap, frac):
    w, cdf = GR.weights(emap, geo)
    p = GR.density(geo, w, cdf, frac)
    npx = geo.n_px()
    assert sum(pc * int(n) for pc, n in zip(p, npx)) == Fraction(1)
    wgt = GR.ray_weight(frac, w, N_IMG * W * H, cdf[-1])
    assert wgt.dtype == np.float32
    s = sum(float(pc) * int(n) * float(x) for pc, n, x in zip(p, npx, wgt))
    print(f"uniform_frac {frac}: sum p weight - 1 = {s - 1:.2e}")
    assert abs(s - 1) <= 1e-6
    if frac > 0:
        assert float(wgt.max()) <= 1 / frac


def test_all_uniform_is_the_plain_sampler(geo, emap):
    w, cdf = GR.weights(emap, geo)
    img, pix, cell, wgt = GR.sample(11, 5, 0, 4096, geo, w, cdf, 1.0)
    i0, p0 = SR.picks(11, 5, 0, 4096, N_IMG, W * H)
    assert np.array_equal(img, i0) and np.array_equal(pix, p0)
    assert np.array_equal(wgt, np.ones(4096, np.float32))
    assert np.array_equal(cell, geo.cell_of(i0, p0))


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.5, 1.0])
def test_flat_map_weighs_every_ray_one(geo, frac):
    w, cdf = GR.weights(np.ones(geo.n_cells, np.float32), geo)
    assert int(cdf[-1]) == 65536 * N_IMG * W * H
    _, _, _, wgt = GR.sample(2, 9, 1, 2048, geo, w, cdf, frac)
    assert np.array_equal(wgt, np.ones(2048, np.float32))


@pytest.mark.parametrize("frac", [0.0, 0.5])
def test_picks_in_range(geo, emap, frac):
    w, cdf = GR.weights(emap, geo)
    img, pix, cell, wgt = GR.sample(4, 17, 2, 1 << 14, geo, w, cdf, frac)
    assert img.min() >= 0 and img.max() < N_IMG and pix.min() >= 0 and pix.max() < W * H
    assert np.array_equal(cell, geo.cell_of(img, pix)) and cell.dtype == np.int32
    assert np.array_equal(wgt, GR.ray_weight(frac, w[cell], N_IMG * W * H, cdf[-1]))
    # inside a cell every pixel is reached; with a uniform share every cell is,
    # edge cells included (the smallest expects 2^14 * 0.5 * 25 / 2331 = 88 rays)
    if frac > 0:
        assert set(cell.tolist()) == set(range(geo.n_cells))
    hot = pix[cell == HOT]
    assert len(set(hot.tolist())) == int(geo.n_px()[HOT])


def test_hot_cell_frequency(geo, emap):
    """counted from the picks, not through the CDF"""
    n, frac = 1 << 14, 0.5
    w, cdf = GR.weights(emap, geo)
    img, pix, _, _ = GR.sample(11, 5, 0, n, geo, w, cdf, frac)
    count = int((geo.cell_of(img, pix) == HOT).sum())
    npx = int(geo.n_px()[HOT])
    p = frac * npx / (N_IMG * W * H) + (1 - frac) * int(w[HOT]) * npx / int(cdf[-1])
    sigma = (n * p * (1 - p)) ** 0.5
    print(f"hot cell: {count} of {n}, expected {n * p:.1f}, sigma {sigma:.1f}")
    assert abs(count - n * p) <= 5 * sigma


def test_epilogue_and_refresh_rules(geo):
    rng = np.random.default_rng(5)
    n = 500
    rgb = rng.random((n, 3), dtype=np.float32)
    tgt = rng.random((n, 3), dtype=np.float32)
    rgb[3, 1], rgb[4, 0], rgb[5] = np.nan, np.inf, 1e3          # 5: finite, clamps
    cell = rng.integers(0, geo.n_cells, n).astype(np.int32)
    wgt = rng.uniform(0.5, 2.0, n).astype(np.float32)
    acc_sum, acc_cnt = np.zeros(geo.n_cells, np.uint64), np.zeros(geo.n_cells, np.uint32)
    seeds = [rng.standard_normal((n, 3)).astype(np.float32),
             rng.standard_normal(n).astype(np.float32)]
    out = GR.epilogue(rgb, tgt, cell, wgt, acc_sum, acc_cnt, seeds)
    assert int(acc_cnt.sum()) == n - 2
    assert np.array_equal(out[0], seeds[0] * wgt[:, None]) and np.array_equal(out[1], seeds[1] * wgt)
    d = rgb[6].astype(np.float64) - tgt[6]
    only = np.zeros(geo.n_cells, np.uint64)
    GR.epilogue(rgb[6:7], tgt[6:7], cell[6:7], wgt[6:7], only, np.zeros(geo.n_cells, np.uint32), [])
    assert abs(int(only[cell[6]]) - (d * d).sum() * 2 ** 20) <= 2
    only[:] = 0
    GR.epilogue(rgb[5:6], tgt[5:6], cell[5:6], wgt[5:6], only, np.zeros(geo.n_cells, np.uint32), [])
    assert int(only[cell[5]]) == 1 << 24
    emap = np.ones(geo.n_cells, np.float32)
    seen = acc_cnt > 0
    s, c = acc_sum.copy(), acc_cnt.copy()
    new = GR.refresh(emap, acc_sum, acc_cnt, 0.5)
    assert not acc_sum.any() and not acc_cnt.any()
    assert np.array_equal(new[~seen], emap[~seen])
    mean = s[seen] / 2.0 ** 20 / c[seen]
    assert np.allclose(new[seen], 0.5 + 0.5 * mean, rtol=1e-6)
    assert np.array_equal(GR.refresh(new, acc_sum, acc_cnt, 0.5), new)
