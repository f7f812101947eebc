"""Numpy restatements of the TSDF fusion rules (include/radnerf.h, "TSDF
fusion"), and the analytic scene the TSDF tests share.

  integrate        rn_tsdf_integrate op for op: fp32 arrays throughout, one
                   rounding per operation, the cameras folded in ascending order
  decisions64      the same update's discrete decisions in fp64 (pixel index,
                   in-image, near, the opacity branch, s > trunc, s >= -trunc)
                   with the distance of each from its boundary
  surface_nets_valid  rn_surface_count_valid / rn_surface_emit_valid, as
                   mesh_ref.surface_nets with the two observation rules
  lattice_colors   rn_lattice_colors
  scene            a sphere of radius 0.3 seen by six small cameras

A volume is a dict of flat fp32 arrays over the lattice points, x fastest:
phi, w, rgb (points, 3), wc.
"""
from types import SimpleNamespace

import numpy as np

import image_out_ref as IR
import mesh_ref as R

F32 = np.float32
NEAR = 0.01                    # rendering.NEAR_DISTANCE

# decision codes of one (camera, point) pair
SKIP, CARVE, HIT, HIT_COLOUR = 0, 1, 2, 3


def fresh(n_pts):
    z = lambda *s: np.zeros(s, F32)
    return dict(phi=z(n_pts), w=z(n_pts), rgb=z(n_pts, 3), wc=z(n_pts))


def points(lo, step, res):
    """x, y, z of every lattice point, flat, x fastest: lo + float32(i) * step"""
    x, y, z = R.lattice_points(lo, step, res)
    return x.ravel(), y.ravel(), z.ravel()


def integrate(vol, sc, cams=None, carve=True, near=NEAR, opacity_min=0.5, colour=True,
              dirs=None, depth=None):
    """Fold the cameras `cams` (indices, ascending; None: all) of the scene
    into vol in place -> code (len(cams), points) int8 and pix (same, int32,
    -1 where the point never reached a pixel): the decisions taken."""
    cams = range(len(sc.poses)) if cams is None else cams
    dirs = sc.dirs if dirs is None else dirs
    depth = sc.depth if depth is None else depth
    X = points(sc.lo, sc.step, sc.res)
    fx, fy, cx, cy = (F32(v) for v in sc.K)
    Wf, Hf = F32(sc.W), F32(sc.H)
    trunc, near, omin = F32(sc.trunc), F32(near), F32(opacity_min)
    phi, w, rgb, wc = vol["phi"], vol["w"], vol["rgb"], vol["wc"]
    codes, pixs = [], []
    with np.errstate(all="ignore"):
        for c in cams:
            P = sc.poses[c].astype(F32)
            d = [X[j] - P[j, 3] for j in range(3)]
            xc = (P[0, 0] * d[0] + P[1, 0] * d[1]) + P[2, 0] * d[2]
            yc = (P[0, 1] * d[0] + P[1, 1] * d[1]) + P[2, 1] * d[2]
            zc = (P[0, 2] * d[0] + P[1, 2] * d[1]) + P[2, 2] * d[2]
            ok = zc >= near
            u = np.floor((fx * xc) / zc + cx)
            v = np.floor((fy * yc) / zc + cy)
            ok &= (u >= 0) & (u < Wf) & (v >= 0) & (v < Hf)
            pix = np.where(ok, v * Wf + u, F32(0)).astype(np.int64)
            o = sc.opacity[c][pix]
            hit = ok & (o >= omin)
            miss = ok & ~(o >= omin)
            dd = depth[c][pix] / o
            e = dirs[pix]
            n2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            tv = ((xc * e[:, 0] + yc * e[:, 1]) + zc * e[:, 2]) / n2
            s = (tv - dd) * np.sqrt(n2)
            hit &= s <= trunc
            obs = np.where(hit, np.fmax(s / trunc, F32(-1)), F32(-1))
            fold = hit | (miss & bool(carve))
            col = hit & (s >= -trunc)
            phi[:] = np.where(fold, (phi * w + obs) / (w + F32(1)), phi)
            w[:] = np.where(fold, w + F32(1), w)
            if colour:
                q = sc.rgb[c][pix]
                rgb[:] = np.where(col[:, None], (rgb * wc[:, None] + q) / (wc + F32(1))[:, None],
                                  rgb)
                wc[:] = np.where(col, wc + F32(1), wc)
            code = np.where(col, HIT_COLOUR, np.where(hit, HIT, np.where(fold, CARVE, SKIP)))
            codes.append(code.astype(np.int8))
            pixs.append(np.where(ok, pix, -1).astype(np.int32))
    return np.stack(codes), np.stack(pixs)


def decisions64(sc, carve=True, near=NEAR, opacity_min=0.5, dirs=None, depth=None):
    """The discrete decisions of integrate() in fp64 from the same fp32 inputs
    -> code, pix (n_cams, points) as integrate returns them, and marginal
    (points) bool: some camera's decision for the point lies closer to its
    boundary than the exclusion rule's margin -- px or py within 1e-4 of an
    integer (where the point is at or beyond near and within 1e-4 px of the
    image), zc within 1e-5 of near, s within 1e-4 trunc of +-trunc."""
    dirs = (sc.dirs if dirs is None else dirs).astype(np.float64)
    depth = (sc.depth if depth is None else depth).astype(np.float64)
    lo, step = sc.lo.astype(np.float64), sc.step.astype(np.float64)
    ax = [lo[d] + np.arange(sc.res[d] + 1, dtype=np.float64) * step[d] for d in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    X = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    fx, fy, cx, cy = (float(F32(v)) for v in sc.K)
    trunc, near, omin = float(F32(sc.trunc)), float(F32(near)), float(F32(opacity_min))
    codes, pixs = [], []
    marginal = np.zeros(len(X), bool)
    with np.errstate(all="ignore"):
        for c in range(len(sc.poses)):
            P = sc.poses[c].astype(np.float64)
            pc = (X - P[:, 3]) @ P[:, :3]
            zc = pc[:, 2]
            px, py = fx * pc[:, 0] / zc + cx, fy * pc[:, 1] / zc + cy
            front = zc >= near
            marginal |= np.abs(zc - near) < 1e-5
            close = front & (px > -1e-4) & (px < sc.W + 1e-4) & (py > -1e-4) & (py < sc.H + 1e-4)
            marginal |= close & ((np.abs(px - np.rint(px)) < 1e-4)
                                 | (np.abs(py - np.rint(py)) < 1e-4))
            u, v = np.floor(px), np.floor(py)
            ok = front & (u >= 0) & (u < sc.W) & (v >= 0) & (v < sc.H)
            pix = np.where(ok, v * sc.W + u, 0).astype(np.int64)
            o = sc.opacity[c].astype(np.float64)[pix]
            hit = ok & (o >= omin)
            miss = ok & ~(o >= omin)
            e = dirs[pix]
            n2 = (e * e).sum(1)
            s = ((pc * e).sum(1) / n2 - depth[c][pix] / o) * np.sqrt(n2)
            marginal |= hit & ((np.abs(s - trunc) < 1e-4 * trunc)
                               | (np.abs(s + trunc) < 1e-4 * trunc))
            hit &= s <= trunc
            fold = hit | (miss & bool(carve))
            col = hit & (s >= -trunc)
            code = np.where(col, HIT_COLOUR, np.where(hit, HIT, np.where(fold, CARVE, SKIP)))
            codes.append(code.astype(np.int8))
            pixs.append(np.where(ok, pix, -1).astype(np.int32))
    return np.stack(codes), np.stack(pixs), marginal


def _lattice(a, res):
    return np.asarray(a, F32).reshape(res[2] + 1, res[1] + 1, res[0] + 1)


def surface_nets_valid(phi, w, iso, lo, step):
    """mesh_ref.surface_nets with the observation rules: the vertices of cells
    whose 8 corners all have w > 0, renumbered in their order, and the quads
    whose four cells are all such cells.  A vertex's position and normal depend
    on its own cell's corners alone, so they are mesh_ref's."""
    phi, w = np.ascontiguousarray(phi, F32), np.ascontiguousarray(w, F32)
    v, f, nr = R.surface_nets(phi, iso, lo, step)
    pz, py, px = phi.shape
    nz, ny, nx = pz - 1, py - 1, px - 1
    off = [(q & 1, q >> 1 & 1, q >> 2 & 1) for q in range(8)]
    with np.errstate(all="ignore"):
        inside, seen = phi >= F32(iso), w > 0
    corner = lambda a: np.stack([a[dz:dz + nz, dy:dy + ny, dx:dx + nx] for dx, dy, dz in off], -1)
    cin = corner(inside)
    active = cin.any(-1) & ~cin.all(-1)
    keep_v = corner(seen).all(-1)[active]                  # per vertex, ascending c
    assert len(keep_v) == len(v)
    new_id = np.cumsum(keep_v) - 1
    quads = f.reshape(-1, 6)
    keep_q = keep_v[quads].all(1) if len(quads) else np.zeros(0, bool)
    faces = new_id[quads[keep_q]].reshape(-1, 3).astype(np.int32)
    return v[keep_v], faces, nr[keep_v]


def lattice_colors(vertices, res, lo, step, rgb, wc):
    """rn_lattice_colors: (V, 3) uint8"""
    v = np.asarray(vertices, F32)
    lo, step = np.asarray(lo, F32), np.asarray(step, F32)
    rgb = np.asarray(rgb, F32).reshape(res[2] + 1, res[1] + 1, res[0] + 1, 3)
    wc = _lattice(wc, res)
    with np.errstate(all="ignore"):
        g = (v - lo[None, :]) / step[None, :]
        top = np.asarray(res, F32)[None, :] - F32(1)
        cf = np.fmin(np.fmax(np.floor(g), F32(0)), top)
        cf = np.where(np.isnan(cf), F32(0), cf)
        f = np.fmin(np.fmax(g - cf, F32(0)), F32(1))
        f = np.where(np.isnan(f), F32(0), f)
        c = cf.astype(np.int64)
        sw = np.zeros(len(v), F32)
        acc = np.zeros((len(v), 3), F32)
        for q in range(8):
            o = (q & 1, q >> 1 & 1, q >> 2 & 1)
            wt = [f[:, a] if o[a] else F32(1) - f[:, a] for a in range(3)]
            t = (wt[0] * wt[1]) * wt[2]
            at = (c[:, 2] + o[2], c[:, 1] + o[1], c[:, 0] + o[0])
            on = wc[at] > 0
            sw = np.where(on, sw + t, sw)
            acc = np.where(on[:, None], acc + t[:, None] * rgb[at], acc)
        val = np.where((sw > 0)[:, None], acc / sw[:, None], F32(0)).astype(F32)
    return IR.quantize_u8(val)


# ---- the scene ------------------------------------------------------------------------
RADIUS = 0.3
RES = (24, 20, 16)
W, H = 40, 32
PINHOLE = (30.0, 30.0, 19.37, 15.71)          # fx, fy, cx, cy: no centred principal point
TRUNC = 0.25                                   # TSDFVolume's default: 4 of the largest step.
SOFT_CAM, SOFT = 2, 0.7                        # one camera's hits have opacity 0.7


def look_at(eye, target, up):
    """c2w (3, 4), columns right / down / front / eye"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    front = target - eye
    front /= np.linalg.norm(front)
    right = np.cross(front, up)
    right /= np.linalg.norm(right)
    down = np.cross(front, right)
    return np.stack([right, down, front, eye], 1)


def _cameras():
    # the ring's axis lies near a diagonal of the box, so that the sixth
    # camera, inside the box on the far side, sees the cap the ring cannot
    axis = np.array([0.55, 0.6, 0.58])
    axis /= np.linalg.norm(axis)
    e1 = np.cross(axis, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    up = np.array([0.13, -0.21, 0.97])
    poses = []
    for i in range(5):
        a = 0.4 + 2 * np.pi * i / 5
        eye = 1.2 * (np.cos(0.35) * (np.cos(a) * e1 + np.sin(a) * e2) + np.sin(0.35) * axis)
        target = np.array([0.013, -0.021, 0.017]) * (1 + i)
        poses.append(look_at(eye, target, up))
    poses.append(look_at(-0.78 * axis, (0.011, 0.019, -0.014), up))
    return np.stack(poses).astype(F32)


def directions(normalised=False):
    """ray_utils.py's directions for the pinhole: pixel centres at +0.5"""
    fx, fy, cx, cy = PINHOLE
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64),
                       indexing="ij")
    d = np.stack([(i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, np.ones_like(i)], -1).reshape(-1, 3)
    if normalised:
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(d, F32)


def render(poses, dirs):
    """fp64 ray-sphere distances along each pixel's directions row (in units
    of that row's length, as the renderer's t), cast to fp32 -> depth, opacity
    (n, H*W), rgb (n, H*W, 3): the colour is a function of the hit point"""
    depth, opac, rgb = [], [], []
    d64 = dirs.astype(np.float64)
    for P in poses.astype(np.float64):
        o, dw = P[:, 3], d64 @ P[:, :3].T
        a, b = (dw * dw).sum(1), (dw @ o)
        disc = b * b - a * (o @ o - RADIUS * RADIUS)
        hit = disc > 0
        t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / a, 0.0)
        hit &= t > 0
        x = o[None, :] + t[:, None] * dw
        depth.append(np.where(hit, t, 0.0))
        opac.append(hit.astype(np.float64))
        rgb.append(np.where(hit[:, None], 0.5 + 0.5 * x / RADIUS, 0.0))
    f = lambda a: np.ascontiguousarray(np.stack(a), F32)
    return f(depth), f(opac), f(rgb)


_scenes = {}


def scene(normalised=False):
    """The shared scene (built once per kind and left unchanged): the sphere
    in [-0.5, 0.5]^3 on 24 x 20 x 16 cells, five cameras of 40 x 32 pixels on
    a tilted ring of radius 1.2 and one inside the box, look-at targets off
    the origin and an up vector off the axes; camera SOFT_CAM's hits have
    opacity 0.7 and a depth scaled by it."""
    if normalised not in _scenes:
        lo, step = R.box_step((-0.5,) * 3, (0.5,) * 3, RES)
        poses = _cameras()
        dirs = directions(normalised)
        depth, opac, rgb = render(poses, dirs)
        opac[SOFT_CAM] = opac[SOFT_CAM] * F32(SOFT)
        depth[SOFT_CAM] = depth[SOFT_CAM] * F32(SOFT)
        n_pts = (RES[0] + 1) * (RES[1] + 1) * (RES[2] + 1)
        _scenes[normalised] = SimpleNamespace(
            res=RES, lo=lo, step=step, hi=np.full(3, 0.5, F32), n_pts=n_pts, trunc=TRUNC,
            poses=poses, K=PINHOLE, W=W, H=H, dirs=dirs, depth=depth, opacity=opac, rgb=rgb)
    return _scenes[normalised]


def intrinsics():
    fx, fy, cx, cy = PINHOLE
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


_fused = {}


def fused(normalised=False, carve=True):
    """The scene's six cameras folded into a fresh volume by integrate() ->
    (vol, code, pix), computed once per kind and left unchanged."""
    key = (normalised, carve)
    if key not in _fused:
        sc = scene(normalised)
        vol = fresh(sc.n_pts)
        code, pix = integrate(vol, sc, carve=carve)
        _fused[key] = (vol, code, pix)
    return _fused[key]
