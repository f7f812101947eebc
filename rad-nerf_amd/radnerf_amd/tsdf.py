"""Mesh export by TSDF fusion: the geometry a model renders, as a mesh.

    TSDFVolume   a truncated signed distance volume on a lattice:
                 .integrate  a batch of rendered depth images in one launch
                             (rn_tsdf_integrate), no host synchronisation
                 .extract    surface nets at level 0 that leave unobserved
                             points alone (rn_surface_count_valid /
                             rn_surface_emit_valid), colours from the volume
                             (rn_lattice_colors)
    fuse_mesh    render every pose with one ImageEvaluator, integrate every
                 `batch` images, extract, optionally filter_components

mesh.extract_mesh meshes a density the model never defines for K > 1 (the
gate has no value at a point in space); what training constrains is the
gate-weighted depth along camera rays.  Fusing those depth maps carves every
point in front of a rendered surface as free space by every camera that sees
through it, leaves points nobody observed without a surface, and needs no
density level: the surface is phi = 0 by construction.  phi is the mean of the
observed signed distances, positive INSIDE, in units of trunc, so
mesh.surface_nets' conventions hold at iso = 0 (inside is value >= iso, normals
point from dense to empty).  include/radnerf.h states every operation.
"""
import math

import numpy as np
import torch

from ._lib import lib
from .mesh import (_LIMIT, Mesh, _box, _criteria, _model_box, _ptr, _resolution,
                   filter_components, surface_work_bytes)
from .networks import _stream
from .rendering import NEAR_DISTANCE

# trunc=None: this many times the largest lattice step (a choice: wide enough
# that a surface seen at a grazing angle still has both signs on its cells'
# corners, narrow enough that thin parts keep two sides)
DEFAULT_TRUNC_STEPS = 4.0


def _intrinsics(fn, K):
    Kh = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    if Kh.shape != (3, 3):
        raise ValueError(f"{fn}: intrinsics must be a 3x3 pinhole matrix, got shape {Kh.shape}")
    fx, fy, cx, cy = (float(Kh[0, 0]), float(Kh[1, 1]), float(Kh[0, 2]), float(Kh[1, 2]))
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        raise ValueError(f"{fn}: intrinsics need finite fx, fy > 0 and cx, cy, got "
                         f"{(fx, fy, cx, cy)}")
    return fx, fy, cx, cy


def _img_wh(fn, img_wh):
    try:
        W, H = (int(v) for v in img_wh)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: img_wh must be (W, H), got {img_wh!r}") from None
    if W < 1 or H < 1 or W * H >= _LIMIT:
        raise ValueError(f"{fn}: img_wh must be positive with fewer than 2^31 pixels, got "
                         f"{W} x {H}")
    return W, H


def _poses(fn, poses):
    if not torch.is_tensor(poses) or poses.ndim != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"{fn}: poses must be a (N, 3, 4) camera-to-world tensor, got "
                         f"{tuple(getattr(poses, 'shape', ()))}")
    if poses.dtype != torch.float32:
        raise ValueError(f"{fn}: poses must be float32, got {poses.dtype}")


def _observation(fn, near, opacity_min):
    near, opacity_min = float(near), float(opacity_min)
    if not (math.isfinite(near) and near >= 0.0):
        raise ValueError(f"{fn}: near must be finite and >= 0, got {near!r}")
    if not 0.0 < opacity_min <= 1.0:
        raise ValueError(f"{fn}: opacity_min must lie in (0, 1], got {opacity_min!r}")
    return near, opacity_min


def _lattice(fn, resolution, aabb, trunc):
    """-> res, lo, step, hi, trunc, checked; nothing is allocated"""
    res = _resolution(fn, resolution)
    lo, step = _box(fn, aabb, res)
    hi = np.asarray(aabb[1], np.float32).reshape(3).copy()
    big = float(step.max())
    if trunc is None:
        trunc = DEFAULT_TRUNC_STEPS * big
    try:
        trunc = float(np.float32(trunc))
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: trunc must be a number or None, got {trunc!r}") from None
    if not (math.isfinite(trunc) and trunc >= math.sqrt(3.0) * big):
        raise ValueError(f"{fn}: trunc {trunc!r} is below sqrt(3) lattice steps "
                         f"({math.sqrt(3.0) * big:.6g}, a cell's diagonal)")
    return res, lo, step, hi, trunc


class TSDFVolume:
    """A TSDF volume of resolution (an int or (nx, ny, nz) cells) over aabb =
    (lo, hi): phi and w (nz + 1, ny + 1, nx + 1) fp32, x fastest, and with
    colors=True rgb (..., 3) and wc, all zeros when fresh (w == 0: never
    observed).  Point i of an axis lies at lo + float32(i) * step, step =
    (hi - lo) / n in fp32, as mesh.density_lattice has it.

    trunc: the truncation distance in world units; None means
    DEFAULT_TRUNC_STEPS = 4 times the largest lattice step, which is a choice,
    not a property of the model.  ValueError, before anything is allocated,
    for a trunc below sqrt(3) of the largest step (a cell's diagonal: a
    thinner band can miss every lattice point next to the surface) and for a
    lattice of 2^31 points or more."""

    def __init__(self, resolution, aabb, trunc=None, colors=True, device="cuda"):
        fn = "TSDFVolume"
        self.res, self.lo, self.step, self.hi, self.trunc = _lattice(fn, resolution, aabb, trunc)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{fn}: the volume lives on the GPU, got device {self.device}")
        shape = (self.res[2] + 1, self.res[1] + 1, self.res[0] + 1)
        f32 = dict(device=self.device, dtype=torch.float32)
        self.phi, self.w = torch.zeros(shape, **f32), torch.zeros(shape, **f32)
        self.rgb = torch.zeros(shape + (3,), **f32) if colors else None
        self.wc = torch.zeros(shape, **f32) if colors else None
        self.device = self.phi.device                      # "cuda" -> the device it names

    @property
    def aabb(self):
        return self.lo, self.hi

    def reset(self):
        """A fresh volume again: all zeros."""
        for t in (self.phi, self.w, self.rgb, self.wc):
            if t is not None:
                t.zero_()

    @torch.no_grad()
    def integrate(self, depth, opacity, poses, intrinsics, directions, img_wh, rgb=None,
                  near=NEAR_DISTANCE, opacity_min=0.5, carve=True):
        """Fold n images of one pinhole camera model into the volume: one
        launch, no host synchronisation, the volume read and written once
        however large n is.  depth, opacity (n, H*W) fp32 as
        ImageEvaluator.render_image returns them (depth is sum w t: it is
        divided by the opacity here); poses (n, 3, 4) c2w, axes right / down /
        front; intrinsics the 3x3 pinhole matrix and directions (H*W, 3) the
        buffer the images were rendered with; rgb (n, H*W, 3) or None (the
        colour lattice is then left alone).

        A point is observed by a camera when it projects into the image at
        depth zc >= near.  Where the pixel's opacity is below opacity_min the
        ray hit nothing: with carve the point is free space (-1), without it
        the camera says nothing.  Otherwise s, the distance along the pixel's
        ray behind the rendered depth, gives clamp(s / trunc, -1, .); a point
        more than trunc behind the surface is hidden and not observed.
        opacity_min = 0.5 and carve = True are choices: a lower opacity_min
        trusts the depth of half-transparent pixels, carve = False keeps the
        background of masked renders from erasing what other cameras saw.
        Every observation has weight 1; the cameras fold in their order, and
        any split of them into consecutive calls gives the same bits."""
        fn = "TSDFVolume.integrate"
        W, H = _img_wh(fn, img_wh)
        fx, fy, cx, cy = _intrinsics(fn, intrinsics)
        near, opacity_min = _observation(fn, near, opacity_min)
        _poses(fn, poses)
        n, N = poses.shape[0], W * H
        want = {"depth": (depth, (n, N)), "opacity": (opacity, (n, N)),
                "directions": (directions, (N, 3))}
        if rgb is not None:
            if self.rgb is None:
                raise ValueError(f"{fn}: rgb images given to a volume built with colors=False")
            want["rgb"] = (rgb, (n, N, 3))
        for name, (t, shape) in want.items():
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"{fn}: {name} must be a {shape} tensor ({n} poses, img_wh "
                                 f"{W} x {H}), got {tuple(getattr(t, 'shape', ()))}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{fn}: {name} must be contiguous float32")
        for name, t in [("poses", poses)] + [(k, v[0]) for k, v in want.items()]:
            if t.device != self.device:
                raise ValueError(f"{fn}: {name} is on {t.device}, the volume on {self.device}")
        poses = poses.contiguous()
        ptr = lambda t: None if t is None else t.data_ptr()
        lib().tsdf_integrate(*self.res, _ptr(self.lo), _ptr(self.step), poses.data_ptr(), n, fx,
                             fy, cx, cy, W, H, directions.data_ptr(), depth.data_ptr(),
                             opacity.data_ptr(), ptr(rgb), self.trunc, near, opacity_min,
                             int(bool(carve)), self.phi.data_ptr(), self.w.data_ptr(),
                             ptr(self.rgb), ptr(self.wc), _stream(self.device))
        return self

    @torch.no_grad()
    def extract(self, normals=True):
        """The surface phi = 0 -> Mesh on the device, by surface nets that
        respect unobserved points: a cell with a corner nobody observed holds
        no vertex and an edge next to such a cell no quad, so the mesh stays
        open where the cameras saw nothing instead of growing a false shell one
        truncation distance behind every surface.  Inside is phi >= 0, normals
        point outwards, orders come from scans (mesh.surface_nets); with
        colours the vertices take the trilinear mean of the colour lattice over
        their cell's observed corners.  One host read, to size the outputs."""
        fn = "TSDFVolume.extract"
        dev, st, L = self.device, _stream(self.device), lib()
        work = torch.empty(surface_work_bytes(self.res), dtype=torch.uint8, device=dev)
        L.surface_count_valid(self.phi.data_ptr(), self.w.data_ptr(), *self.res, 0.0,
                              work.data_ptr(), st)
        n_v, n_q = work[:16].view(torch.int64).tolist()    # the call's one synchronisation
        if n_v >= _LIMIT or 2 * n_q >= _LIMIT:
            raise ValueError(f"{fn}: {n_v} vertices and {2 * n_q} triangles; int32 faces hold "
                             f"fewer than 2^31 of each")
        v = torch.empty(n_v, 3, device=dev)
        nr = torch.empty(n_v, 3, device=dev) if normals else None
        f = torch.empty(2 * n_q, 3, dtype=torch.int32, device=dev)
        L.surface_emit_valid(self.phi.data_ptr(), self.w.data_ptr(), *self.res, 0.0,
                             _ptr(self.lo), _ptr(self.step), work.data_ptr(), n_v, n_q,
                             v.data_ptr() if n_v else None,
                             nr.data_ptr() if normals and n_v else None,
                             f.data_ptr() if n_q else None, st)
        col = None
        if self.rgb is not None:
            col = torch.empty(n_v, 3, dtype=torch.uint8, device=dev)
            L.lattice_colors(v.data_ptr() if n_v else None, n_v, *self.res, _ptr(self.lo),
                             _ptr(self.step), self.rgb.data_ptr(), self.wc.data_ptr(),
                             col.data_ptr() if n_v else None, st)
        return Mesh(v, f, nr, col)


@torch.no_grad()
def fuse_mesh(model, gating_net, poses, directions, img_wh, intrinsics, resolution=256, aabb=None,
              trunc=None, colors=True, batch=8, keep_largest=None, min_vertices=None,
              min_fraction=None, gate_min=0.0, gate_topk=None, renormalize=False,
              near=NEAR_DISTANCE, opacity_min=0.5, carve=True, normals=True,
              exp_step_factor=None, **render_kw):
    """The mesh of what `model` renders from `poses`: every pose is rendered
    with one ImageEvaluator (gate_min / gate_topk / renormalize and render_kw,
    e.g. T_threshold, as render_image takes them -- a routed model comes out as
    it renders), depth / opacity / rgb are copied device-to-device into the
    slot of a batch of `batch` images, every full batch (and the rest) is one
    TSDFVolume.integrate; the loop does not synchronise with the host.  Then
    TSDFVolume.extract and, if keep_largest, min_vertices or min_fraction is
    given, mesh.filter_components.  aabb=None is the model's box; resolution,
    trunc, colors as TSDFVolume; near, opacity_min, carve as integrate.  The
    result does not depend on `batch`."""
    from .evaluate import ImageEvaluator
    fn = "fuse_mesh"
    clean = not (keep_largest is None and min_vertices is None and min_fraction is None)
    if clean:
        _criteria(fn, keep_largest, min_vertices, min_fraction)
    W, H = _img_wh(fn, img_wh)
    _intrinsics(fn, intrinsics)
    _observation(fn, near, opacity_min)
    _poses(fn, poses)
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"{fn}: batch must be an int >= 1, got {batch!r}")
    box = _model_box(model) if aabb is None else aabb
    res = _lattice(fn, resolution, box, trunc)[0]
    ev = ImageEvaluator(model, gating_net, directions, (W, H), exp_step_factor=exp_step_factor)
    dev = ev.device
    vol = TSDFVolume(res, box, trunc=trunc, colors=colors, device=dev)
    poses = poses.detach().to(dev).contiguous()
    n, N = poses.shape[0], W * H
    B = min(int(batch), max(n, 1))
    depth, opacity = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    rgb = torch.empty(B, N, 3, device=dev) if colors else None
    for i0 in range(0, n, B):
        m = min(B, n - i0)
        for j in range(m):
            out = ev.render_image(poses[i0 + j], gate_min=gate_min, gate_topk=gate_topk,
                                  renormalize=renormalize, **render_kw)
            depth[j].copy_(out["depth"])
            opacity[j].copy_(out["opacity"])
            if colors:
                rgb[j].copy_(out["rgb"])
        vol.integrate(depth[:m], opacity[:m], poses[i0:i0 + m], intrinsics, ev.directions,
                      (W, H), rgb=rgb[:m] if colors else None, near=near,
                      opacity_min=opacity_min, carve=carve)
    mesh = vol.extract(normals=normals)
    if clean:
        mesh = filter_components(mesh, keep_largest, min_vertices, min_fraction)
    return mesh
