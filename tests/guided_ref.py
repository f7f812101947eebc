"""Error-guided sampling restated in numpy and python ints, from the comment
"error-guided pixel sampling" of include/radnerf.h (test code: the package
does not import it).  The random stream is sampler_ref's.

    geometry  tw = ceil(W / tile), th = ceil(H / tile); cell c = (img th + ty)
              tw + tx; edge cells narrower / shorter; pixel index y W + x
    weights   w = clamp(rint(emap * 65536), 1, 2^24) (fp32 product), mass =
              w n_px, cdf = inclusive uint64 sums, total = cdf[-1]
    branch    u = unit(mix((key ^ C_BRANCH) + (i + 1) G)) < uniform_frac: the
              uniform picks of sampler_ref.picks
    guided    t = mulhi64(mix((key ^ C_CELL) + (i + 1) G), total); c = the first
              cell with cdf[c] > t; j = (t - cdf[c - 1]) // w[c]; the pixel is
              (ty tile + j // cw, tx tile + j % cw)
    weight    float32(1 / (f + (((1 - f) w) N_all) / total)) in doubles
    epilogue  e = (d0 d0 + d1 d1) + d2 d2 (fp32); finite: acc_sum[cell] +=
              min(rint(e 2^20), 2^24), acc_cnt[cell] += 1; seeds *= weight
    refresh   cnt > 0: mean = float32((acc_sum 2^-20) / cnt) in doubles,
              emap += alpha (mean - emap) in fp32; accumulators zeroed
"""
import numpy as np

from sampler_ref import _stream, key, picks, unit

C_BRANCH = 0xa0761d6478bd642f
C_CELL = 0xe7037ed1a0b428db
_F = np.float32


class Geometry:
    def __init__(self, n_images, W, H, tile):
        assert 1 <= tile <= 256
        self.n_images, self.W, self.H, self.tile = n_images, W, H, tile
        self.tw, self.th = -(-W // tile), -(-H // tile)
        self.cpi = self.tw * self.th
        self.n_cells = n_images * self.cpi
        assert self.n_cells < 1 << 24
        self.n_pix = W * H

    def cw(self, tx):
        return np.minimum(self.tile, self.W - np.asarray(tx) * self.tile)

    def ch(self, ty):
        return np.minimum(self.tile, self.H - np.asarray(ty) * self.tile)

    def n_px(self):
        """pixels of every cell, int64 (n_cells)"""
        c = np.arange(self.n_cells, dtype=np.int64) % self.cpi
        return (self.cw(c % self.tw) * self.ch(c // self.tw)).astype(np.int64)

    def cell_of(self, img, pix):
        img, pix = np.asarray(img, np.int64), np.asarray(pix, np.int64)
        y, x = pix // self.W, pix % self.W
        return (img * self.th + y // self.tile) * self.tw + x // self.tile


def weights(emap, geo):
    """(w uint32, cdf uint64) of an fp32 map"""
    emap = np.asarray(emap, _F).reshape(-1)
    assert emap.size == geo.n_cells
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(emap * _F(65536.0))
    w = np.where(v >= 1, np.minimum(v, _F(1 << 24)), _F(1)).astype(np.uint32)   # a NaN -> 1
    mass = w.astype(np.uint64) * geo.n_px().astype(np.uint64)
    return w, np.cumsum(mass, dtype=np.uint64)


def ray_weight(f, w_c, n_all, total):
    """the importance weight, fp32; doubles in the stated order"""
    f = float(_F(f))
    w_c = np.asarray(w_c).astype(np.float64)
    return (1.0 / (f + (((1.0 - f) * w_c) * float(n_all)) / float(int(total)))
            ).astype(_F)


def sample(seed, step, rank, n_rays, geo, w, cdf, uniform_frac):
    """(img int64, pix int64, cell int32, weight fp32), (n_rays) each"""
    k = key(seed, step, rank)
    img, pix = picks(seed, step, rank, n_rays, geo.n_images, geo.n_pix)
    u = unit(_stream(k ^ C_BRANCH, n_rays))
    guided = ~(u < _F(uniform_frac))
    z2 = _stream(k ^ C_CELL, n_rays)
    total = int(cdf[-1])
    cdf_i = [int(v) for v in cdf]
    import bisect
    for i in np.nonzero(guided)[0]:
        t = (int(z2[i]) * total) >> 64
        c = bisect.bisect_right(cdf_i, t)           # the first cell with cdf[c] > t
        below = cdf_i[c - 1] if c else 0
        j = (t - below) // int(w[c])
        rem = c % geo.cpi
        ty, tx = rem // geo.tw, rem % geo.tw
        cw = int(geo.cw(tx))
        assert j < cw * int(geo.ch(ty))
        img[i] = c // geo.cpi
        pix[i] = (ty * geo.tile + j // cw) * geo.W + tx * geo.tile + j % cw
    cell = geo.cell_of(img, pix)
    wgt = ray_weight(uniform_frac, w[cell], geo.n_images * geo.n_pix, total)
    return img, pix, cell.astype(np.int32), wgt


def density(geo, w, cdf, uniform_frac):
    """p(pixel) per cell as a Fraction: f / N_all + (1 - f) w / total"""
    from fractions import Fraction
    f = Fraction(float(_F(uniform_frac)))
    n_all, total = geo.n_images * geo.n_pix, int(cdf[-1])
    return [f / n_all + (1 - f) * Fraction(int(wc), total) for wc in w]


def epilogue(rgb, target, cell, wgt, acc_sum, acc_cnt, seeds):
    """Adds to acc_sum (python ints / uint64) and acc_cnt in place; returns the
    seeds times the weights, fp32."""
    rgb, target = np.asarray(rgb, _F), np.asarray(target, _F)
    with np.errstate(invalid="ignore", over="ignore"):
        d = rgb - target
        e = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        q = np.minimum(np.rint(e * _F(1 << 20)), _F(1 << 24))
    ok = np.isfinite(e)
    np.add.at(acc_sum, cell[ok], q[ok].astype(np.uint64))
    np.add.at(acc_cnt, cell[ok], np.uint32(1))
    wgt = np.asarray(wgt, _F)
    with np.errstate(invalid="ignore", over="ignore"):
        return [np.asarray(s, _F) * wgt.reshape((-1,) + (1,) * (np.ndim(s) - 1)) for s in seeds]


def refresh(emap, acc_sum, acc_cnt, alpha):
    """the new map; zeroes the accumulators in place"""
    emap = np.asarray(emap, _F).copy()
    hit = acc_cnt > 0
    mean = ((acc_sum[hit].astype(np.float64) * 2.0 ** -20)
            / acc_cnt[hit].astype(np.float64)).astype(_F)
    emap[hit] = emap[hit] + _F(alpha) * (mean - emap[hit])
    acc_sum[:] = 0
    acc_cnt[:] = 0
    return emap
