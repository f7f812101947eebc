"""numpy restatement of the four validation-image operations (include/radnerf.h,
"validation images"), word for word: fp32 arrays throughout, one rounding per
operation, clip before astype(uint8).  The GPU tests compare bytes with these.
"""
import struct
import zlib

import numpy as np

F = np.float32


def _u8(y):
    """NaN -> 0, clamp to [0, 255], truncate toward zero"""
    y = np.asarray(y, dtype=F)
    y = np.where(np.isnan(y), F(0), y)
    return np.clip(y, F(0), F(255)).astype(np.uint8)


def minmax_finite(x):
    """{min, max} over the finite values, {0, 0} if there is none"""
    x = np.asarray(x, dtype=F)
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return np.zeros(2, dtype=F)
    return np.array([fin.min(), fin.max()], dtype=F)


def quantize_u8(src):
    return _u8(np.asarray(src, dtype=F) * F(255))


def colormap_u8(x, range2, lut, swap_rb=False):
    x = np.asarray(x, dtype=F)
    mn, mx = F(range2[0]), F(range2[1])
    with np.errstate(all="ignore"):
        den = F(mx - mn)
        if not den > 0:
            idx = np.zeros(x.shape, dtype=np.uint8)
        else:
            t = ((x - mn).astype(F) / den).astype(F)
            idx = np.where(np.isfinite(x), _u8(t * F(255)), np.uint8(0))
    out = np.asarray(lut, dtype=np.uint8)[idx]
    return out[..., ::-1].copy() if swap_rb else out


def depth2img(x, lut, swap_rb=False):
    return colormap_u8(x, minmax_finite(x), lut, swap_rb)


def gate_map_u8(gate, palette, hard=False):
    g = np.asarray(gate, dtype=F)
    pal = np.asarray(palette, dtype=np.uint8)
    n, K = g.shape
    if hard:
        arg = np.argmax(np.where(np.isnan(g), -np.inf, g), axis=1)
        return pal[arg]
    p = pal.astype(F)
    with np.errstate(all="ignore"):
        acc = (g[:, 0:1] * p[0][None, :]).astype(F)
        for k in range(1, K):                    # the sequential blend, k ascending
            acc = (acc + (g[:, k:k + 1] * p[k][None, :]).astype(F)).astype(F)
        return _u8(acc + F(0.5))


def read_png(path):
    """A small PNG decoder for what imageout.write_png emits: 8-bit grey or
    RGB, no interlace, filter type 0 on every row; every chunk's CRC is
    checked.  Returns the (H, W) or (H, W, 3) array and the chunk type list."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks, idat, ihdr = 8, [], b"", None
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body), tag
        chunks.append(tag)
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, colour, comp, filt, lace = ihdr
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    C = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + W * C)
    assert not raw[:, 0].any()                   # filter type 0
    img = raw[:, 1:].reshape((H, W, 3) if C == 3 else (H, W)).copy()
    return img, chunks
