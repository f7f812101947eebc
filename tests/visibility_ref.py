"""numpy restatement of rn_mark_invisible_cells, written from the comment in
include/radnerf.h (the package does not import this file).

Two forms of the same arithmetic: dtype=np.float32 follows the stated
operation order (every multiply and add rounded to fp32 on its own), so the
kernel can be compared bit for bit; dtype=np.float64 is the same formula in
double, for judging how many cells sit so close to a frustum plane that the
rounding decides them (edge_band).

Also the camera rig the visibility tests share, and the fp64 erode decay.
"""
import numpy as np

G = 128
G3 = G ** 3

# the rig: image 64 x 48, fx = fy = 100, principal point at the centre
IMG_WH = (64, 48)
INTRINSICS = np.array([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]])


def morton_invert(m):
    """rn_morton3d_invert (raymarching.cu:91-99) of a uint32 array."""
    x = m.astype(np.uint32) & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xc30c30c3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0f00f00f)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xff0000ff)
    x = (x | (x >> np.uint32(16))) & np.uint32(0x0000ffff)
    return x


def morton_coords(m=None):
    """(n, 3) integer coordinates of the Morton cells m (default: all G^3)."""
    if m is None:
        m = np.arange(G3, dtype=np.uint32)
    m = np.asarray(m, dtype=np.uint32)
    return np.stack([morton_invert(m), morton_invert(m >> np.uint32(1)),
                     morton_invert(m >> np.uint32(2))], -1)


def cell_centres(coords, c, scale, dtype):
    """X_a = ((i_a / (G-1)) * 2 - 1) * (sc - hgs), sc = min(2^(c-1), scale)."""
    f = dtype
    sc = f(min(2.0 ** (c - 1), float(np.float32(scale))))
    hgs = f(sc / f(G))
    i = coords.astype(f)
    return ((i / f(G - 1)) * f(2) - f(1)) * f(sc - hgs)


def look_at(eye, target):
    """(3, 4) c2w: columns right, down, front, eye."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    front = target - eye
    front /= np.linalg.norm(front)
    right = np.cross(front, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(front, right)
    return np.stack([right, down, front, eye], 1)


def rig_poses(scale):
    """The six cameras of the tests, (6, 3, 4) fp32: three outside the box
    (scaled by s = 2 max(scale, 0.5)), three inside it (absolute)."""
    s = 2.0 * max(float(scale), 0.5)
    cams = [((0.9 * s, 0.1 * s, 0.2 * s), (0.0, 0.25 * s, 0.0)),
            ((-0.2 * s, -0.95 * s, 0.1 * s), (0.2 * s, 0.0, -0.1 * s)),
            ((0.1 * s, 0.2 * s, 1.1 * s), (-0.15 * s, 0.0, 0.0)),
            ((0.11, 0.052, -0.203), (0.4, 0.3, 0.1)),
            ((-0.23, 0.31, 0.12), (-0.5, -0.2, 0.0)),
            ((0.02, -0.33, 0.27), (0.0, 0.5, -0.4))]
    return np.stack([look_at(e, t) for e, t in cams]).astype(np.float32)


def classify(X, poses, intrinsics, img_wh, near, dtype, band_eps=None):
    """Per cell of X (n, 3): (n_covered, any_too_near[, in_band]).

    in_band (band_eps given): some comparison of some camera has two sides
    closer than band_eps times the summed magnitudes of the terms they were
    formed from (the absolute products of the dot products, carried through
    fx, cx, W ...).  Every comparison counts, reached or not.  On the rig
    this holds 2.8e-4 to 4.1e-4 of the cells."""
    f = dtype
    fx, fy = f(intrinsics[0][0]), f(intrinsics[1][1])
    cx, cy = f(intrinsics[0][2]), f(intrinsics[1][2])
    W, H = f(int(img_wh[0])), f(int(img_wh[1]))
    near = f(np.float32(near))
    X = X.astype(f)
    n_cov = np.zeros(X.shape[0], np.int32)
    too_near = np.zeros(X.shape[0], bool)
    band = np.zeros(X.shape[0], bool)
    for P in np.asarray(poses, np.float32):
        P = P.astype(f)
        d = [X[:, j] - P[j, 3] for j in range(3)]
        cam = [(P[0, col] * d[0] + P[1, col] * d[1]) + P[2, col] * d[2] for col in range(3)]
        xc, yc, zc = cam
        px = fx * xc + cx * zc
        py = fy * yc + cy * zc
        in_image = (zc > 0) & (px >= 0) & (px < W * zc) & (py >= 0) & (py < H * zc)
        n_cov += in_image & (zc >= near)
        too_near |= in_image & (zc < near)
        if band_eps is not None:
            a = [np.abs(d[j]) for j in range(3)]
            mag = [abs(P[0, col]) * a[0] + abs(P[1, col]) * a[1] + abs(P[2, col]) * a[2]
                   for col in range(3)]
            mpx = fx * mag[0] + abs(cx) * mag[2]
            mpy = fy * mag[1] + abs(cy) * mag[2]
            e = f(band_eps)
            band |= np.abs(zc) < e * mag[2]
            band |= np.abs(px) < e * mpx
            band |= np.abs(py) < e * mpy
            band |= np.abs(px - W * zc) < e * (mpx + W * mag[2])
            band |= np.abs(py - H * zc) < e * (mpy + H * mag[2])
            band |= np.abs(zc - near) < e * (mag[2] + near)
    return (n_cov, too_near, band) if band_eps is not None else (n_cov, too_near)


def mark(poses, intrinsics, img_wh, near, cascades, scale, dtype, band_eps=None):
    """The whole grid: dict of count (C, G^3) in dtype's arithmetic (the fp32
    form: the kernel's count_grid bit for bit), n_covered, too_near, valid
    (C, G^3), n_culled (C) and, with band_eps, band (C, G^3)."""
    coords = morton_coords()
    out = {k: [] for k in ("count", "n_covered", "too_near", "valid", "band")}
    n_cams = len(poses)
    for c in range(cascades):
        X = cell_centres(coords, c, scale, dtype)
        r = classify(X, poses, intrinsics, img_wh, near, dtype, band_eps)
        out["n_covered"].append(r[0])
        out["too_near"].append(r[1])
        out["valid"].append((r[0] > 0) & ~r[1])
        out["count"].append(r[0].astype(dtype) / dtype(n_cams))
        out["band"].append(r[2] if band_eps is not None else np.zeros_like(r[1]))
    out = {k: np.stack(v) for k, v in out.items()}
    out["n_culled"] = (~out["valid"]).sum(1).astype(np.int32)
    return out


def apply_mark(grid, bits, valid):
    """What the mark leaves of one sub-NeRF's grid (C, G^3) and bitfield
    (C G^3 / 8 bytes, bit j of byte b = cell 8 b + j)."""
    g = np.where(valid, np.maximum(grid, np.float32(0)), np.float32(-1)).astype(np.float32)
    keep = np.packbits(valid.reshape(-1), bitorder="little")
    return g, bits & keep


def erode_decay(count, decay=0.95):
    """networks.py:398 in fp64: clamp(decay ** (1 / count), 0.1, 0.95)."""
    with np.errstate(divide="ignore"):
        return np.clip(np.float64(decay) ** (1.0 / count.astype(np.float64)), 0.1, 0.95)


_RIG = {}


def rig_mark(scale, near, dtype=np.float32, band_eps=None):
    """mark() of the rig at `scale` (cascades as the model's: 1 at 0.5, 4 at
    4), computed once per process and shared by the tests: do not modify."""
    key = (float(scale), float(near), np.dtype(dtype).name, band_eps)
    if key not in _RIG:
        cascades = max(1 + int(np.ceil(np.log2(2 * float(scale)))), 1)
        _RIG[key] = mark(rig_poses(scale), INTRINSICS, IMG_WH, near, cascades, scale, dtype,
                         band_eps)
    return _RIG[key]
