"""The batch sampler's random stream restated in numpy, from the comment of
rn_sample_batch in include/radnerf.h (test code: the package does not import
it).  All arithmetic is uint64 and wraps.

    mix(z)    the splitmix64 finaliser
    G         0x9e3779b97f4a7c15
    key       mix(seed * G + (rank << 40 | step))
    pick i    z = mix(key + (i + 1) G); img = (hi32(z) n_images) >> 32,
              pix = (lo32(z) n_pix) >> 32
    jitter    unit(mix((key ^ 0xd1b54a32d192ed03) + (k n_rays + i + 1) G))
    bg        unit(mix((key ^ 0x8cb92ba72f3d8dd7) + (c + 1) G))
    unit(z)   float(z >> 40) * 2^-24
"""
import numpy as np

MASK = (1 << 64) - 1
G = 0x9e3779b97f4a7c15
C_NOISE = 0xd1b54a32d192ed03
C_BG = 0x8cb92ba72f3d8dd7
_U = np.uint64


def mix_int(z):
    """mix on one python int"""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def mix(z):
    """mix on a uint64 array"""
    z = np.asarray(z, dtype=_U)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U(30))) * _U(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U(27))) * _U(0x94d049bb133111eb)
    return z ^ (z >> _U(31))


def key(seed, step, rank=0):
    assert 0 <= step < 1 << 40 and 0 <= rank < 1 << 24
    return mix_int((seed & MASK) * G + ((rank << 40) | step))


def _stream(k, n):
    """mix(k + j G) for j = 1..n"""
    j = np.arange(1, n + 1, dtype=_U)
    with np.errstate(over="ignore"):
        return mix(_U(k) + j * _U(G))


def unit(z):
    return (z >> _U(40)).astype(np.float32) * np.float32(2.0 ** -24)


def picks(seed, step, rank, n_rays, n_images, n_pix):
    """(img_idxs, pix_idxs), int64 (n_rays) each"""
    assert 1 <= n_images < 1 << 32 and 1 <= n_pix < 1 << 32
    z = _stream(key(seed, step, rank), n_rays)
    img = ((z >> _U(32)) * _U(n_images)) >> _U(32)
    pix = ((z & _U(0xffffffff)) * _U(n_pix)) >> _U(32)
    return img.astype(np.int64), pix.astype(np.int64)


def noise(seed, step, rank, n_models, n_rays):
    """the march jitter, fp32 (n_models, n_rays)"""
    z = _stream(key(seed, step, rank) ^ C_NOISE, n_models * n_rays)
    return unit(z).reshape(n_models, n_rays)


def bg(seed, step, rank=0):
    """the random background, fp32 (3)"""
    return unit(_stream(key(seed, step, rank) ^ C_BG, 3))
