"""Mesh export: the geometry of a trained model as a triangle mesh.

    density_lattice   sigma on a regular lattice of points (rn_density_lattice)
    surface_nets      the iso-surface of such a lattice (rn_surface_count /
                      rn_surface_emit): naive surface nets, one vertex per
                      sign-changing cell, one quad per sign-changing interior
                      lattice edge; the rules are in include/radnerf.h
    extract_mesh      both, plus per-vertex colours from the model's forward
    Mesh.save         binary little-endian PLY or OBJ (standard library + numpy)
    load_ply/load_obj read back what save wrote

What the lattice holds for K > 1: the ray gate has no value at a point in
space -- every sub-NeRF is a whole model of the scene and the image is the
gate-weighted sum of their renders -- so the lattice is a weighted sum of the
sub-NeRFs' densities, by default their mean (a consensus).  A one-hot `weights`
gives one sub-NeRF's own surface.  A model trained with routing may hold
floaters in sub-NeRFs that never saw a region; they are exported as they are.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import lib
from .networks import _stream, field_ptrs

# the training density threshold (trainer.py: 0.01 * MAX_SAMPLES / 3 ** 0.5),
# extract_mesh's default level: a choice, not a property of the model
DEFAULT_ISO = 0.01 * 1024 / 3 ** 0.5
_LIMIT = 1 << 31


@dataclass
class Mesh:
    """vertices (V, 3) fp32, faces (F, 3) int32, normals (V, 3) fp32 or None,
    colors (V, 3) uint8 or None; on the device after an extraction, on the CPU
    after a load."""
    vertices: torch.Tensor
    faces: torch.Tensor
    normals: Optional[torch.Tensor] = None
    colors: Optional[torch.Tensor] = None

    def _numpy(self):
        f = lambda t: None if t is None else t.detach().cpu().numpy()
        return f(self.vertices), f(self.faces), f(self.normals), f(self.colors)

    def save(self, path):
        """Write `path`: .ply (binary little-endian: x y z, then nx ny nz and
        red green blue where present, faces as vertex_indices lists) or .obj."""
        p = str(path).lower()
        if p.endswith(".ply"):
            _write_ply(path, *self._numpy())
        elif p.endswith(".obj"):
            _write_obj(path, *self._numpy())
        else:
            raise ValueError(f"Mesh.save: {path}: the file name must end in .ply or .obj")
        return path


# ---- files --------------------------------------------------------------------------
def _vertex_dtype(normals, colors):
    fields = [(n, "<f4") for n in ("x", "y", "z")]
    if normals:
        fields += [(n, "<f4") for n in ("nx", "ny", "nz")]
    if colors:
        fields += [(n, "u1") for n in ("red", "green", "blue")]
    return np.dtype(fields)


_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _write_ply(path, v, f, n, c):
    vt = _vertex_dtype(n is not None, c is not None)
    rec = np.empty(len(v), vt)
    for i, name in enumerate(("x", "y", "z")):
        rec[name] = v[:, i]
    if n is not None:
        for i, name in enumerate(("nx", "ny", "nz")):
            rec[name] = n[:, i]
    if c is not None:
        for i, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, i]
    fr = np.empty(len(f), _FACE_DTYPE)
    fr["n"] = 3
    fr["v"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'uchar' if vt[name] == np.uint8 else 'float'} {name}" for name in vt.names]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(fr.tobytes())


def load_ply(path):
    """Read a PLY written by Mesh.save -> Mesh on the CPU."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"load_ply: {path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"load_ply: {path}: only binary_little_endian 1.0 is read")
    counts, props, cur = {}, {"vertex": [], "face": []}, None
    for ln in lines:
        t = ln.split()
        if t[:1] == ["element"]:
            cur = t[1]
            counts[cur] = int(t[2])
            props.setdefault(cur, [])
        elif t[:1] == ["property"]:
            props[cur].append(t[1:])
    names = [p[-1] for p in props["vertex"]]
    normals, colors = "nx" in names, "red" in names
    vt = _vertex_dtype(normals, colors)
    if list(vt.names) != names or props["face"] != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError(f"load_ply: {path}: not the layout Mesh.save writes")
    nv, nf = counts.get("vertex", 0), counts.get("face", 0)
    body = end + len(b"end_header\n")
    if len(data) != body + nv * vt.itemsize + nf * _FACE_DTYPE.itemsize:
        raise ValueError(f"load_ply: {path}: truncated or trailing data")
    rec = np.frombuffer(data, vt, nv, body)
    fr = np.frombuffer(data, _FACE_DTYPE, nf, body + nv * vt.itemsize)
    if nf and (fr["n"] != 3).any():
        raise ValueError(f"load_ply: {path}: a face is not a triangle")
    col = lambda ns, dt: torch.from_numpy(np.stack([rec[k] for k in ns], 1).astype(dt))
    return Mesh(col(("x", "y", "z"), np.float32), torch.from_numpy(fr["v"].astype(np.int32)),
                col(("nx", "ny", "nz"), np.float32) if normals else None,
                col(("red", "green", "blue"), np.uint8) if colors else None)


def _write_obj(path, v, f, n, c):
    g = lambda x: "%.9g" % x                       # 9 digits: fp32 round-trips
    with open(path, "w") as fh:
        for i in range(len(v)):
            row = [g(x) for x in v[i]]
            if c is not None:
                row += [g(np.float32(x) / np.float32(255)) for x in c[i]]
            fh.write("v " + " ".join(row) + "\n")
        if n is not None:
            for i in range(len(n)):
                fh.write("vn " + " ".join(g(x) for x in n[i]) + "\n")
        tag = (lambda i: f"{i}//{i}") if n is not None else str
        for a, b, cc in (f + 1).tolist():
            fh.write(f"f {tag(a)} {tag(b)} {tag(cc)}\n")


def load_obj(path):
    """Read an OBJ written by Mesh.save -> Mesh on the CPU."""
    v, n, f = [], [], []
    with open(path) as fh:
        for ln in fh:
            t = ln.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:]])
            elif t[0] == "vn":
                n.append([float(x) for x in t[1:]])
            elif t[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in t[1:]])
    v = np.asarray(v, np.float32).reshape(len(v), -1)
    colors = None
    if v.shape[1] == 6:
        colors = torch.from_numpy(np.rint(v[:, 3:] * np.float32(255)).astype(np.uint8))
    return Mesh(torch.from_numpy(np.ascontiguousarray(v[:, :3])),
                torch.from_numpy(np.asarray(f, np.int32).reshape(len(f), 3)),
                torch.from_numpy(np.asarray(n, np.float32).reshape(len(n), 3)) if n else None,
                colors)


# ---- arguments ------------------------------------------------------------------------
def _resolution(fn, resolution):
    if isinstance(resolution, (int, np.integer)):
        r = (resolution,) * 3
    else:
        try:
            r = tuple(resolution)
        except TypeError:
            r = ()
    if len(r) != 3 or any(not isinstance(v, (int, np.integer)) or v < 1 for v in r):
        raise ValueError(f"{fn}: resolution must be an int or (nx, ny, nz), each >= 1, got "
                         f"{resolution!r}")
    r = tuple(int(v) for v in r)
    pts = (r[0] + 1) * (r[1] + 1) * (r[2] + 1)
    if pts >= _LIMIT:
        raise ValueError(f"{fn}: a lattice of {pts} points (resolution {r}); the limit is below "
                         f"2^31")
    return r


def _box(fn, aabb, res):
    """(lo, hi) -> lo, step as fp32 host arrays; step = (hi - lo) / n in fp32"""
    try:
        lo, hi = (np.asarray(v, np.float32).reshape(3) for v in aabb)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: aabb must be (lo, hi) of 3 numbers each, got {aabb!r}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError(f"{fn}: aabb needs finite lo < hi on every axis, got {aabb!r}")
    step = ((hi - lo) / np.asarray(res, np.float32)).astype(np.float32)
    return np.ascontiguousarray(lo), np.ascontiguousarray(step)


def _model_box(model):
    return model._h_min, (model._h_min + model._h_ext).astype(np.float32)


def _weights(fn, model, weights):
    K = model.size
    if weights is None:
        return np.full(K, np.float32(1) / np.float32(K), np.float32)
    w = weights.detach().cpu().numpy() if torch.is_tensor(weights) else np.asarray(weights)
    if w.shape != (K,):
        raise ValueError(f"{fn}: weights must be ({K},), one per sub-NeRF, got {tuple(w.shape)}")
    w = np.ascontiguousarray(w, np.float32)
    if not np.isfinite(w).all():
        raise ValueError(f"{fn}: weights must be finite")
    return w


def _ptr(a):
    return a.ctypes.data


# ---- the lattice ------------------------------------------------------------------------
@torch.no_grad()
def density_lattice(model, resolution, aabb=None, weights=None):
    """sigma of `model` (an MNGP or NGP on the GPU) on a regular lattice ->
    (nz + 1, ny + 1, nx + 1) fp32 on the model's device, x fastest.

    resolution: cells per axis, an int or (nx, ny, nz).  aabb = (lo, hi), by
    default the model's box, and inside it.  Point i of an axis lies at
    lo + float32(i) * step with step = (hi - lo) / n in fp32.  weights: (K,)
    fp32, by default 1 / K each; the value is w_0 sigma_0 + w_1 sigma_1 + ...
    added in that order over the sub-NeRFs with a non-zero weight, sigma_k
    being exactly MNGP.density(x, k).  One launch, no xyz buffer."""
    fn = "density_lattice"
    res = _resolution(fn, resolution)
    mlo, mhi = _model_box(model)
    lo, step = _box(fn, (mlo, mhi) if aabb is None else aabb, res)
    if aabb is not None:
        hi = np.asarray(aabb[1], np.float32).reshape(3)
        if (lo < mlo).any() or (hi > mhi).any():
            raise ValueError(f"{fn}: aabb {aabb!r} leaves the model's box "
                             f"({mlo.tolist()}, {mhi.tolist()})")
    w = _weights(fn, model, weights)
    dev = model.mlp_params.device
    if dev.type != "cuda":
        raise ValueError(f"{fn}: the model must be on the GPU, got {dev}")
    out = torch.empty(res[2] + 1, res[1] + 1, res[0] + 1, device=dev)
    lib().density_lattice(res[0], res[1], res[2], _ptr(lo), _ptr(step), _ptr(w), model.size,
                          *field_ptrs(model), out.data_ptr(), _stream(dev))
    return out


# ---- the surface ------------------------------------------------------------------------
def surface_work_bytes(resolution):
    """bytes of device scratch an extraction at `resolution` takes"""
    res = _resolution("surface_work_bytes", resolution)
    n = ctypes.c_int64(0)
    lib().surface_work_bytes(res[0], res[1], res[2], ctypes.byref(n))
    return n.value


@torch.no_grad()
def surface_nets(sigma, iso, aabb, normals=True):
    """The iso-surface of a device lattice sigma (nz + 1, ny + 1, nx + 1) at
    the level iso, over the box aabb = (lo, hi) -> Mesh on the device.  Inside
    is sigma >= iso; normals point from dense to empty and triangles are
    counter-clockwise seen from the empty side.  A surface that reaches the
    lattice's boundary stays open there.  The same lattice gives the same
    bits on every call; the call synchronises once, to size the outputs."""
    fn = "surface_nets"
    if not torch.is_tensor(sigma) or sigma.dtype != torch.float32 or sigma.dim() != 3:
        raise ValueError(f"{fn}: sigma must be a (nz + 1, ny + 1, nx + 1) float32 tensor")
    if not sigma.is_contiguous():
        raise ValueError(f"{fn}: sigma must be contiguous")
    res = _resolution(fn, tuple(int(s) - 1 for s in reversed(sigma.shape)))
    lo, step = _box(fn, aabb, res)
    if not sigma.is_cuda:
        raise ValueError(f"{fn}: sigma must be on the GPU, got {sigma.device}")
    dev, st = sigma.device, _stream(sigma.device)
    iso = float(np.float32(iso))
    work = torch.empty(surface_work_bytes(res), dtype=torch.uint8, device=dev)
    L = lib()
    L.surface_count(sigma.data_ptr(), *res, iso, work.data_ptr(), st)
    n_v, n_q = work[:16].view(torch.int64).tolist()        # the call's one synchronisation
    if n_v >= _LIMIT or 2 * n_q >= _LIMIT:
        raise ValueError(f"{fn}: {n_v} vertices and {2 * n_q} triangles; int32 faces hold "
                         f"fewer than 2^31 of each")
    v = torch.empty(n_v, 3, device=dev)
    nr = torch.empty(n_v, 3, device=dev) if normals else None
    f = torch.empty(2 * n_q, 3, dtype=torch.int32, device=dev)
    L.surface_emit(sigma.data_ptr(), *res, iso, _ptr(lo), _ptr(step), work.data_ptr(), n_v, n_q,
                   v.data_ptr() if n_v else None, nr.data_ptr() if normals and n_v else None,
                   f.data_ptr() if n_q else None, st)
    return Mesh(v, f, nr)


@torch.no_grad()
def vertex_colors(model, vertices, normals, weights=None):
    """(V, 3) uint8: every live sub-NeRF's forward at the vertices, seen
    against the normal (d = -normal), mixed as sum w_k rgb_k / sum w_k and
    quantised by imageout.to_uint8."""
    from .imageout import to_uint8
    w = _weights("vertex_colors", model, weights)
    live = [k for k in range(model.size) if w[k] != 0]
    if not live:
        raise ValueError("vertex_colors: every weight is zero")
    d = (-normals).contiguous()
    acc, total = None, np.float32(0)
    for k in live:
        _, rgb = model(vertices, d, k)
        acc = float(w[k]) * rgb if acc is None else acc + float(w[k]) * rgb
        total = np.float32(total + w[k])
    return to_uint8((acc / float(total)).contiguous())


@torch.no_grad()
def extract_mesh(model, resolution=256, iso=None, aabb=None, weights=None, normals=True,
                 colors=False):
    """density_lattice, then surface_nets at the level iso (by default the
    training density threshold DEFAULT_ISO, a choice), then with colors=True
    vertex_colors (which takes the normals: they are computed either way)."""
    sigma = density_lattice(model, resolution, aabb, weights)          # checks the arguments
    mesh = surface_nets(sigma, DEFAULT_ISO if iso is None else iso,
                        _model_box(model) if aabb is None else aabb,
                        normals=normals or colors)
    if colors and mesh.vertices.shape[0]:
        mesh.colors = vertex_colors(model, mesh.vertices, mesh.normals, weights)
    elif colors:
        mesh.colors = torch.empty(0, 3, dtype=torch.uint8, device=mesh.vertices.device)
    if not normals:
        mesh.normals = None
    return mesh
