"""Mesh export: the geometry of a trained model as a triangle mesh.

    density_lattice   sigma on a regular lattice of points (rn_density_lattice)
    surface_nets      the iso-surface of such a lattice (rn_surface_count /
                      rn_surface_emit): naive surface nets, one vertex per
                      sign-changing cell, one quad per sign-changing interior
                      lattice edge; the rules are in include/radnerf.h
    components        the connected components of a mesh (rn_mesh_label /
                      rn_mesh_components)
    filter_components keep the largest components, or those above a size
                      (rn_mesh_compact_count / rn_mesh_compact_emit)
    extract_mesh      lattice, surface, optionally the filter, plus per-vertex
                      colours from the model's forward
    Mesh.save         binary little-endian PLY or OBJ (standard library + numpy)
    load_ply/load_obj read back what save wrote

What the lattice holds for K > 1: the ray gate has no value at a point in
space -- every sub-NeRF is a whole model of the scene and the image is the
gate-weighted sum of their renders -- so the lattice is a weighted sum of the
sub-NeRFs' densities, by default their mean (a consensus).  A one-hot `weights`
gives one sub-NeRF's own surface.  A model trained with routing may hold
floaters in sub-NeRFs that never saw a region: density above the level where
no ray ever constrained the field.  density_lattice(occupancy=True) drops what
lies in cells the occupancy grid calls empty, filter_components drops whole
components by size (surfaces inside the object included, which no occupancy
test can see).
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import lib
from .networks import _stream, field_ptrs, model_bitfields

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


def _bitfields(fn, model):
    """the sub-NeRFs' occupancy bitfields, checked: occupancy=True needs them"""
    try:
        bits = model_bitfields(model)
        C, G = int(model.cascades), int(model.grid_size)
        float(model.scale)
    except (AttributeError, TypeError):
        raise ValueError(f"{fn}: occupancy=True needs a model with density_bitfield_k buffers, "
                         f"cascades, grid_size and scale; {type(model).__name__} has none")
    for k, b in enumerate(bits):
        if (not torch.is_tensor(b) or b.dtype != torch.uint8 or b.numel() != C * G ** 3 // 8
                or not b.is_contiguous()):
            raise ValueError(f"{fn}: density_bitfield_{k} must be {C * G ** 3 // 8} contiguous "
                             f"uint8 (cascades {C}, grid_size {G})")
    return bits


# ---- the lattice ------------------------------------------------------------------------
@torch.no_grad()
def density_lattice(model, resolution, aabb=None, weights=None, occupancy=False):
    """sigma of `model` (an MNGP or NGP on the GPU) on a regular lattice ->
    (nz + 1, ny + 1, nx + 1) fp32 on the model's device, x fastest.

    resolution: cells per axis, an int or (nx, ny, nz).  aabb = (lo, hi), by
    default the model's box, and inside it.  Point i of an axis lies at
    lo + float32(i) * step with step = (hi - lo) / n in fp32.  weights: (K,)
    fp32, by default 1 / K each; the value is w_0 sigma_0 + w_1 sigma_1 + ...
    added in that order over the sub-NeRFs with a non-zero weight, sigma_k
    being exactly MNGP.density(x, k).  One launch, no xyz buffer.

    occupancy=True: sigma_k counts as exactly 0 where the point's cell in
    sub-NeRF k's own density_bitfield is clear -- the cell the march would
    query for that position (rn_density_lattice_masked) -- and a tile of 32
    points that is dead for every live sub-NeRF is neither encoded nor run
    through the MLP.  A live point keeps the bits the unmasked lattice gives
    it.  Caveat: the bitfield is a thresholded, max-pooled, decayed copy of the
    density, not the density; where the field and the grid disagree the mask
    cuts a surface at a cell face."""
    fn = "density_lattice"
    res = _resolution(fn, resolution)
    bits = _bitfields(fn, model) if occupancy else None
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
    if bits is None:
        lib().density_lattice(res[0], res[1], res[2], _ptr(lo), _ptr(step), _ptr(w), model.size,
                              *field_ptrs(model), out.data_ptr(), _stream(dev))
        return out
    if any(b.device != dev for b in bits):
        raise ValueError(f"{fn}: the bitfields must be on the model's device {dev}")
    ptrs = (ctypes.c_void_p * model.size)(*[b.data_ptr() for b in bits])
    lib().density_lattice_masked(res[0], res[1], res[2], _ptr(lo), _ptr(step), _ptr(w),
                                 model.size, *field_ptrs(model), ptrs, int(model.cascades),
                                 int(model.grid_size), float(model.scale), out.data_ptr(),
                                 _stream(dev))
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


# ---- clean-up ---------------------------------------------------------------------------
@dataclass
class Components:
    """label (V,) int32: the component of every vertex; n_vertices, n_faces
    (C,) int64: the components' sizes.  Components are numbered in ascending
    order of their lowest vertex index."""
    label: torch.Tensor
    n_vertices: torch.Tensor
    n_faces: torch.Tensor


# Rounds of the labelling per batch, and the batches a call may take.  The
# numpy model of the scheme (tests/mesh_clean_ref.py: label_rounds) needs 5 to
# 12 rounds on the test meshes, a 4,000-quad strip with permuted indices
# included, so one batch is the usual case; 16 batches are 192 rounds.
LABEL_ROUNDS = 12
LABEL_BATCHES = 16


def _faces_arg(fn, faces):
    if (not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2
            or faces.shape[1] != 3):
        raise ValueError(f"{fn}: faces must be an (F, 3) int32 tensor")
    if not faces.is_contiguous():
        raise ValueError(f"{fn}: faces must be contiguous")
    if faces.shape[0] >= _LIMIT:
        raise ValueError(f"{fn}: {faces.shape[0]} faces; the limit is below 2^31")


def _mesh_arg(fn, mesh):
    v = getattr(mesh, "vertices", None)
    if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"{fn}: mesh.vertices must be a (V, 3) float32 tensor")
    _faces_arg(fn, mesh.faces)
    V = v.shape[0]
    if V >= _LIMIT:
        raise ValueError(f"{fn}: {V} vertices; the limit is below 2^31")
    for name, dt in (("normals", torch.float32), ("colors", torch.uint8)):
        t = getattr(mesh, name)
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (V, 3)):
            raise ValueError(f"{fn}: mesh.{name} must be ({V}, 3) {dt} or None")
    for t in (v, mesh.faces, mesh.normals, mesh.colors):
        if t is not None and (t.device != v.device or not t.is_contiguous()):
            raise ValueError(f"{fn}: the mesh's tensors must be contiguous and on one device")
    if not v.is_cuda:
        raise ValueError(f"{fn}: the mesh must be on the GPU, got {v.device}")
    return V, mesh.faces.shape[0]


def _mesh_work(V, F, dev):
    n = ctypes.c_int64(0)
    lib().mesh_work_bytes(V, F, ctypes.byref(n))
    return torch.empty(n.value, dtype=torch.uint8, device=dev)


def _label(fn, faces, V, work, rounds=LABEL_ROUNDS, batches=LABEL_BATCHES):
    """root (V,) int32 = the lowest vertex index of every vertex's component
    -> root, C, batches taken.  One host read per batch."""
    dev, F = faces.device, faces.shape[0]
    root = torch.empty(V, dtype=torch.int32, device=dev)
    for b in range(batches):
        lib().mesh_label(faces.data_ptr() if F else None, F, V, root.data_ptr(), work.data_ptr(),
                         rounds, int(b == 0), _stream(dev))
        bad, still, C = work[:24].view(torch.int64).tolist()      # the batch's synchronisation
        if bad:
            raise ValueError(f"{fn}: a face holds a vertex index outside [0, {V})")
        if not still:
            return root, C, b + 1
    raise RuntimeError(f"{fn}: the labelling has not converged after {batches} batches of "
                       f"{rounds} rounds")


def _components(fn, mesh):
    V, F = _mesh_arg(fn, mesh)
    dev = mesh.vertices.device
    if V == 0:
        if F:
            raise ValueError(f"{fn}: a face holds a vertex index outside [0, 0)")
        z = lambda dt: torch.empty(0, dtype=dt, device=dev)
        return Components(z(torch.int32), z(torch.int64), z(torch.int64)), None
    work = _mesh_work(V, F, dev)
    root, C, _ = _label(fn, mesh.faces, V, work)
    label = torch.empty(V, dtype=torch.int32, device=dev)
    nv = torch.empty(C, dtype=torch.int64, device=dev)
    nf = torch.empty(C, dtype=torch.int64, device=dev)
    lib().mesh_components(mesh.faces.data_ptr() if F else None, F, V, root.data_ptr(),
                          work.data_ptr(), C, label.data_ptr(), nv.data_ptr(), nf.data_ptr(),
                          _stream(dev))
    return Components(label, nv, nf), work


@torch.no_grad()
def components(mesh):
    """The connected components of a device Mesh -> Components.  Two vertices
    are connected when some face holds both; a vertex in no face is a
    component of its own; components are numbered in ascending order of their
    lowest vertex index (include/radnerf.h, rn_mesh_*).  The labelling runs in
    batches of LABEL_ROUNDS rounds of min-label hooking and pointer jumping and
    the host reads one flag per batch: usually one synchronisation per call,
    at most LABEL_BATCHES, then RuntimeError.  A face index outside [0, V) is
    a ValueError (it is never dereferenced).  The same mesh gives the same
    bits on every call, whatever the order of its face rows."""
    return _components("components", mesh)[0]


def _criteria(fn, keep_largest, min_vertices, min_fraction):
    if keep_largest is None and min_vertices is None and min_fraction is None:
        raise ValueError(f"{fn}: give keep_largest, min_vertices or min_fraction")
    if keep_largest is not None and (not isinstance(keep_largest, (int, np.integer))
                                     or isinstance(keep_largest, bool) or keep_largest < 1):
        raise ValueError(f"{fn}: keep_largest must be an int >= 1, got {keep_largest!r}")
    if min_vertices is not None and (not isinstance(min_vertices, (int, np.integer))
                                     or isinstance(min_vertices, bool) or min_vertices < 0):
        raise ValueError(f"{fn}: min_vertices must be an int >= 0, got {min_vertices!r}")
    if min_fraction is not None:
        try:
            ok = 0.0 <= float(min_fraction) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{fn}: min_fraction must lie in [0, 1], got {min_fraction!r}")


def _keep(comp, V, keep_largest, min_vertices, min_fraction):
    """(C,) uint8 on the device: 1 where every given criterion holds"""
    nv = comp.n_vertices
    keep = torch.ones_like(nv, dtype=torch.bool)
    if min_vertices is not None:
        keep &= nv >= int(min_vertices)
    if min_fraction is not None:
        keep &= nv >= int(math.ceil(float(min_fraction) * V))
    if keep_largest is not None:
        # rank by vertex count descending, ties to the lower id: a stable sort
        order = torch.sort(nv, descending=True, stable=True).indices
        top = torch.zeros_like(keep)
        top[order[:int(keep_largest)]] = True
        keep &= top
    return keep.to(torch.uint8).contiguous()


@torch.no_grad()
def filter_components(mesh, keep_largest=None, min_vertices=None, min_fraction=None):
    """The Mesh of the components of `mesh` that meet every given criterion:
    n_vertices[c] >= min_vertices; n_vertices[c] >= ceil(min_fraction * V);
    rank below keep_largest, ranking by vertex count descending with ties to
    the lower component id.  Kept vertices and faces keep their relative
    order, face indices are remapped, normals and colors travel with their
    vertices.  Labelling, counting and compaction run on the device; the call
    synchronises twice in the usual case (components' flag read, then the kept
    counts that size the outputs)."""
    fn = "filter_components"
    _criteria(fn, keep_largest, min_vertices, min_fraction)
    comp, work = _components(fn, mesh)
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    dev = mesh.vertices.device
    if V == 0:
        return Mesh(mesh.vertices.clone(), mesh.faces.clone(),
                    None if mesh.normals is None else mesh.normals.clone(),
                    None if mesh.colors is None else mesh.colors.clone())
    keep = _keep(comp, V, keep_largest, min_vertices, min_fraction)
    C = keep.shape[0]
    L, st = lib(), _stream(dev)
    fp = mesh.faces.data_ptr() if F else None
    L.mesh_compact_count(fp, F, V, comp.label.data_ptr(), keep.data_ptr(), C, work.data_ptr(), st)
    n_v, n_f = work[24:40].view(torch.int64).tolist()              # sizes the outputs
    v = torch.empty(n_v, 3, device=dev)
    f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    nr = None if mesh.normals is None else torch.empty(n_v, 3, device=dev)
    col = None if mesh.colors is None else torch.empty(n_v, 3, dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    L.mesh_compact_emit(fp, F, V, work.data_ptr(), mesh.vertices.data_ptr(), ptr(mesh.normals),
                        ptr(mesh.colors), n_v, n_f, ptr(v), ptr(nr), ptr(col), ptr(f), st)
    return Mesh(v, f, nr, col)


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
                 colors=False, occupancy=False, keep_largest=None, min_vertices=None,
                 min_fraction=None):
    """density_lattice (with occupancy=True masked by the occupancy bitfields:
    see its caveat), then surface_nets at the level iso (by default the
    training density threshold DEFAULT_ISO, a choice), then, if keep_largest,
    min_vertices or min_fraction is given, filter_components, then with
    colors=True vertex_colors on the vertices that are left (it takes the
    normals: they are computed either way)."""
    clean = not (keep_largest is None and min_vertices is None and min_fraction is None)
    if clean:
        _criteria("extract_mesh", keep_largest, min_vertices, min_fraction)
    sigma = density_lattice(model, resolution, aabb, weights, occupancy=occupancy)
    mesh = surface_nets(sigma, DEFAULT_ISO if iso is None else iso,
                        _model_box(model) if aabb is None else aabb,
                        normals=normals or colors)
    if clean:
        mesh = filter_components(mesh, keep_largest, min_vertices, min_fraction)
    if colors and mesh.vertices.shape[0]:
        mesh.colors = vertex_colors(model, mesh.vertices, mesh.normals, weights)
    elif colors:
        mesh.colors = torch.empty(0, 3, dtype=torch.uint8, device=mesh.vertices.device)
    if not normals:
        mesh.normals = None
    return mesh
