"""GPU: the mesh export against its references.

  * mesh.surface_nets against tests/mesh_ref.py, index for index: equal counts
    and faces, vertices within 2^-22 max|box coordinate| (bit equality is the
    aim; the bound allows an ulp in the last two operations), normals within
    1e-6, and the same bits on a second call;
  * mesh.density_lattice against the composition it replaces -- a torch-made
    xyz buffer, model.density per sub-NeRF, a torch weighted sum in the order
    w_0 s_0 + w_1 s_1 + ... over the non-zero weights -- bit for bit;
  * mesh.extract_mesh end to end, with colours within one 8-bit level;
  * Trainer.export_mesh: the file reads back equal, the training state is
    untouched.
"""
import numpy as np
import pytest
import torch

import image_out_ref as IR
import mesh_ref as R
from radnerf_amd import mesh
from radnerf_amd import synthetic as S
from radnerf_amd.networks import NGP

pytestmark = pytest.mark.gpu

LATTICES = {
    "sphere24": lambda: R.sphere(24) + (R.SPHERE_ISO,),
    "torus": lambda: R.torus() + (0.0,),
    "one_point": lambda: R.one_point() + (0.5,),
    "empty": lambda: R.empty() + (0.5,),
    "half_space": lambda: R.half_space() + (0.0,),
    "noise": lambda: R.noise() + (R.NOISE_ISO,),
    "smooth": lambda: R.smooth() + (0.0,),             # 64 x 60 x 40 cells: 159 counting blocks
}


def _compare(got, v, f, nr, box_max):
    assert got.vertices.shape == (len(v), 3) and got.faces.shape == (len(f), 3)
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
    assert torch.equal(got.faces.cpu(), torch.from_numpy(f))
    dv = np.abs(got.vertices.cpu().numpy() - v).max() if len(v) else 0.0
    dn = np.abs(got.normals.cpu().numpy() - nr).max() if len(v) else 0.0
    print(f"V {len(v)} F {len(f)} max|dv| {dv:.3e} (bound {2.0 ** -22 * box_max:.3e}) "
          f"max|dn| {dn:.3e}")
    assert dv <= 2.0 ** -22 * box_max
    assert dn <= 1e-6


@pytest.mark.parametrize("name", list(LATTICES))
def test_surface_nets_matches_reference(cuda, name):
    s, lo, step, hi, iso = LATTICES[name]()
    v, f, nr = R.surface_nets(s, iso, lo, step)
    sig = torch.from_numpy(s).to(cuda)
    got = mesh.surface_nets(sig, iso, (lo, hi))
    if name == "smooth":
        assert len(v) > 8 * 1024                          # many blocks, a real scan
    _compare(got, v, f, nr, float(np.abs(np.stack([lo, hi])).max()))
    again = mesh.surface_nets(sig, iso, (lo, hi))
    assert torch.equal(again.vertices.view(torch.int32), got.vertices.view(torch.int32))
    assert torch.equal(again.normals.view(torch.int32), got.normals.view(torch.int32))
    assert torch.equal(again.faces, got.faces)
    bare = mesh.surface_nets(sig, iso, (lo, hi), normals=False)
    assert bare.normals is None and torch.equal(bare.faces, got.faces)
    assert torch.equal(bare.vertices.view(torch.int32), got.vertices.view(torch.int32))


# ---- the lattice ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(cuda):
    ngp = NGP(0.5, seed=3)
    with torch.no_grad():
        ngp.xyz_encoder.params.copy_(
            torch.from_numpy(S.grid_params(ngp.xyz_encoder.n_entries)).view(-1))
    return {"K2": S.parity_scene(2, device=cuda).m, "K3": S.parity_scene(3, device=cuda).m,
            "NGP": ngp.to(cuda), "K9": S.parity_scene(9, device=cuda).m}


# points per axis -> (resolution, aabb): a sub-box, and the whole box
SHAPES = {"9x7x5": ((8, 6, 4), ((-0.3, -0.45, 0.05), (0.41, 0.2, 0.5))),
          "40x33x21": ((39, 32, 20), None),               # 27,720 points: no multiple of 32
          "104x102x103": ((103, 101, 102), None)}         # > 8192 x 4 tiles: the stride loop
_sigmas = {}


def _sub_sigmas(model, key, shape):
    """sigma_k of every sub-NeRF on the lattice, by the composition: computed
    once per (model, shape) and left unchanged"""
    if (key, shape) not in _sigmas:
        res, aabb = SHAPES[shape]
        lo, hi = aabb if aabb is not None else (model._h_min, model._h_min + model._h_ext)
        lo, step = R.box_step(lo, hi, res)
        dev = model.mlp_params.device
        ax = [torch.arange(res[d] + 1, device=dev, dtype=torch.float32) * float(step[d])
              + float(lo[d]) for d in range(3)]
        z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        xyz = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
        with torch.no_grad():
            _sigmas[(key, shape)] = [model.density(xyz, ind=k).reshape(x.shape).clone()
                                     for k in range(model.size)]
    return _sigmas[(key, shape)]


def _compose(sig, w):
    acc = None
    for k, s in enumerate(sig):
        if w[k] != 0:
            acc = float(w[k]) * s if acc is None else acc + float(w[k]) * s
    return torch.zeros_like(sig[0]) if acc is None else acc


def _weights(K, kind):
    if kind == "uniform":
        return None
    if kind == "nonuniform":
        w = np.linspace(0.2, 1.3, K)
    elif kind == "zero":
        w = np.linspace(0.7, 0.1, K)
        w[0] = 0.0
    else:
        w = np.zeros(K)
        w[K - 1] = 1.0
    return w.astype(np.float32)


@pytest.mark.parametrize("kind", ["nonuniform", "zero", "onehot"])
@pytest.mark.parametrize("shape", ["9x7x5", "40x33x21"])
@pytest.mark.parametrize("key", ["K2", "K3", "NGP"])
def test_density_lattice_equals_composition(models, key, shape, kind):
    m = models[key]
    res, aabb = SHAPES[shape]
    w = _weights(m.size, kind)
    got = mesh.density_lattice(m, res, aabb=aabb, weights=w)
    assert got.shape == (res[2] + 1, res[1] + 1, res[0] + 1) and got.dtype == torch.float32
    want = _compose(_sub_sigmas(m, key, shape), w)
    assert torch.isfinite(got).all() and (got.max() > 0 or kind == "zero")
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("key,shape", [("K2", "104x102x103"), ("K9", "9x7x5"),
                                       ("K9", "40x33x21")])
def test_density_lattice_other_paths(models, key, shape):
    """default weights (1 / K each); a lattice of more tiles than one pass of
    the launch takes; 9 sub-NeRFs: wide blocks, and a second group of
    fragments that continues from the stored sum"""
    m = models[key]
    res, aabb = SHAPES[shape]
    got = mesh.density_lattice(m, res, aabb=aabb)
    w = np.full(m.size, np.float32(1) / np.float32(m.size), np.float32)
    assert torch.equal(got, _compose(_sub_sigmas(m, key, shape), w))
    if key == "K9":
        w = _weights(9, "zero")
        got = mesh.density_lattice(m, res, aabb=aabb, weights=torch.from_numpy(w))
        assert torch.equal(got, _compose(_sub_sigmas(m, key, shape), w))


# ---- end to end -------------------------------------------------------------------------
def test_extract_mesh_end_to_end(models):
    m = models["K2"]
    res = (32, 32, 32)
    lo, hi = m._h_min, (m._h_min + m._h_ext).astype(np.float32)
    lo, step = R.box_step(lo, hi, res)
    dev = m.mlp_params.device
    ax = [torch.arange(33, device=dev, dtype=torch.float32) * float(step[d]) + float(lo[d])
          for d in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    xyz = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
    w = np.float32(0.5)
    with torch.no_grad():
        sig = float(w) * m.density(xyz, ind=0) + float(w) * m.density(xyz, ind=1)
    sig = sig.reshape(33, 33, 33)
    iso = float(sig.median())
    v, f, nr = R.surface_nets(sig.cpu().numpy(), iso, lo, step)
    assert len(v) > 1000 and len(f) > 1000                # both signs occur
    got = mesh.extract_mesh(m, resolution=32, iso=iso, colors=True)
    _compare(got, v, f, nr, float(np.abs(np.stack([lo, hi])).max()))
    # colours: the same forward at the reference's vertices and normals
    with torch.no_grad():
        tv, td = torch.from_numpy(v).to(dev), torch.from_numpy(-nr).to(dev)
        rgb = [m(tv, td, k)[1].cpu().numpy() for k in range(2)]
    mix = (w * rgb[0] + w * rgb[1]) / np.float32(w + w)
    want = IR.quantize_u8(mix)
    assert got.colors.dtype == torch.uint8 and got.colors.shape == (len(v), 3)
    d = np.abs(got.colors.cpu().numpy().astype(np.int32) - want.astype(np.int32))
    print("colour levels off:", np.bincount(d.ravel()))
    assert d.max() <= 1
    assert want.std() > 0                                  # not one flat colour
    plain = mesh.extract_mesh(m, resolution=32, iso=iso, normals=False)
    assert plain.normals is None and plain.colors is None
    assert torch.equal(plain.faces, got.faces)


def test_trainer_export_mesh(models, cuda, tmp_path):
    from radnerf_amd.trainer import Trainer
    sc = S.parity_scene(2, device=cuda)
    tr = Trainer(sc.m, sc.g, 256)
    with torch.no_grad():
        sig = mesh.density_lattice(sc.m, 16)
    iso = float(sig.median())

    def snapshot():
        d = {"m." + k: v.clone() for k, v in sc.m.state_dict().items()}
        d.update({"g." + k: v.clone() for k, v in sc.g.state_dict().items()})
        # (the trainer owns gradient buffers from the start: they stay as they are)
        for i, q in enumerate(list(sc.m.parameters()) + list(sc.g.parameters())):
            if q.grad is not None:
                d[f"grad.{i}"] = q.grad.clone()
        return d, tr.global_step

    before, step = snapshot()
    p = str(tmp_path / "model.ply")
    out = tr.export_mesh(p, resolution=16, iso=iso, colors=True)
    assert out.vertices.shape[0] > 100 and out.vertices.is_cuda
    back = mesh.load_ply(p)
    assert torch.equal(back.vertices, out.vertices.cpu())
    assert torch.equal(back.faces, out.faces.cpu())
    assert torch.equal(back.normals, out.normals.cpu())
    assert torch.equal(back.colors, out.colors.cpu())
    after, step2 = snapshot()
    assert step2 == step and set(after) == set(before)
    for k in before:
        assert torch.equal(before[k], after[k]), k
