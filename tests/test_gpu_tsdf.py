"""GPU: the TSDF export against its references (tests/tsdf_ref.py).

  * TSDFVolume.integrate against the fp32 restatement on the sphere scene: w
    and wc equal, phi and rgb the same bits, on every point the exclusion rule
    keeps (a point is left out only where the fp64 restatement puts one of its
    discrete decisions within 1e-4 px / 1e-4 trunc of its boundary; the CPU
    test holds the scene to at most 1 % of such points);
  * any split of the cameras into launches, and a second run, give the same
    bits on every point;
  * extract() against the reference index for index, colours within one level;
  * with w all ones rn_surface_*_valid is mesh.surface_nets bit for bit;
  * launches that observe nothing leave the volume's bits alone;
  * fuse_mesh equals its hand composition and does not depend on `batch`;
  * Trainer.export_mesh(method="tsdf"): the file reads back equal, the
    training state is untouched.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_ref as R
import tsdf_ref as T
from radnerf_amd import mesh, tsdf
from radnerf_amd import synthetic as S
from radnerf_amd._lib import lib
from test_gpu_mesh import LATTICES, _compare

pytestmark = pytest.mark.gpu

BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
KEYS = ("phi", "w", "rgb", "wc")


def _dev(sc, cuda, cams=slice(None)):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[cams])).to(cuda)
    return dict(depth=t(sc.depth), opacity=t(sc.opacity), rgb=t(sc.rgb), poses=t(sc.poses),
                directions=torch.from_numpy(sc.dirs).to(cuda), intrinsics=T.intrinsics(),
                img_wh=(sc.W, sc.H))


def _state(vol):
    return {k: getattr(vol, k).detach().cpu().numpy().reshape(-1, *([3] if k == "rgb" else []))
            for k in KEYS}


def _same_bits(a, b, where=None):
    for k in KEYS:
        x, y = a[k].view(np.int32), b[k].view(np.int32)
        if where is not None:
            x, y = x[where], y[where]
        assert np.array_equal(x, y), (k, int((x != y).sum()))


@pytest.mark.parametrize("normalised,carve", [(False, True), (True, True), (False, False)])
def test_integrate_matches_reference(cuda, normalised, carve):
    sc = T.scene(normalised)
    want = T.fused(normalised, carve)[0]
    keep = ~T.decisions64(sc, carve=carve)[2]
    vol = tsdf.TSDFVolume(sc.res, BOX, trunc=sc.trunc, device=cuda)
    assert vol.trunc == sc.trunc and np.array_equal(vol.lo, sc.lo) and np.array_equal(vol.step, sc.step)
    vol.integrate(carve=carve, **_dev(sc, cuda))
    got = _state(vol)
    diff = {k: int((got[k].view(np.int32) != want[k].view(np.int32)).sum()) for k in KEYS}
    print(f"excluded {int((~keep).sum())} of {sc.n_pts}; differing words anywhere: {diff}")
    assert keep.mean() >= 0.99
    assert np.array_equal(got["w"][keep], want["w"][keep])
    assert np.array_equal(got["wc"][keep], want["wc"][keep])
    _same_bits(got, want, keep)
    assert (want["w"] > 0).sum() > 0.9 * sc.n_pts or not carve


def test_batching_and_reruns_give_the_same_bits(cuda):
    sc = T.scene()
    runs = []
    for split in ([6], [2, 4], [1] * 6, [6]):
        vol = tsdf.TSDFVolume(sc.res, BOX, trunc=sc.trunc, device=cuda)
        c0 = 0
        for n in split:
            vol.integrate(**_dev(sc, cuda, slice(c0, c0 + n)))
            c0 += n
        runs.append(_state(vol))
    for other in runs[1:]:
        _same_bits(runs[0], other)
    # geometry alone: the colour lattice is left alone, phi and w are the same
    vol = tsdf.TSDFVolume(sc.res, BOX, trunc=sc.trunc, device=cuda)
    a = _dev(sc, cuda)
    a.pop("rgb")
    vol.integrate(**a)
    bare = _state(vol)
    assert not bare["rgb"].any() and not bare["wc"].any()
    assert np.array_equal(bare["phi"].view(np.int32), runs[0]["phi"].view(np.int32))
    assert np.array_equal(bare["w"], runs[0]["w"])
    plain = tsdf.TSDFVolume(sc.res, BOX, trunc=sc.trunc, colors=False, device=cuda)
    plain.integrate(**a)
    assert plain.rgb is None and torch.equal(plain.phi, vol.phi) and torch.equal(plain.w, vol.w)
    vol.reset()
    assert not any(v.any() for v in _state(vol).values())


def test_extract_matches_reference(cuda):
    sc = T.scene()
    want = T.fused()[0]
    keep = ~T.decisions64(sc)[2]
    vol = tsdf.TSDFVolume(sc.res, BOX, trunc=sc.trunc, device=cuda)
    vol.integrate(**_dev(sc, cuda))
    _same_bits(_state(vol), want, keep)
    # the excluded points take the reference's values: the meshes are then
    # those of one volume, index for index
    for k in KEYS:
        t = getattr(vol, k).view(-1, *([3] if k == "rgb" else []))
        t[torch.from_numpy(~keep).to(cuda)] = torch.from_numpy(want[k][~keep]).to(cuda)
    lat = lambda a: a.reshape(sc.res[2] + 1, sc.res[1] + 1, sc.res[0] + 1)
    v, f, nr = T.surface_nets_valid(lat(want["phi"]), lat(want["w"]), 0.0, sc.lo, sc.step)
    got = vol.extract()
    assert len(v) > 500
    _compare(got, v, f, nr, 0.5)
    col = T.lattice_colors(v, sc.res, sc.lo, sc.step, want["rgb"], want["wc"])
    assert got.colors.dtype == torch.uint8 and got.colors.shape == (len(v), 3)
    d = np.abs(got.colors.cpu().numpy().astype(np.int32) - col.astype(np.int32))
    print("colour levels off:", np.bincount(d.ravel()))
    assert d.max() <= 1 and col.std() > 0
    again = vol.extract()
    assert torch.equal(again.faces, got.faces) and torch.equal(again.colors, got.colors)
    assert torch.equal(again.vertices.view(torch.int32), got.vertices.view(torch.int32))
    bare = vol.extract(normals=False)
    assert bare.normals is None and torch.equal(bare.faces, got.faces)


def _valid_nets(sig, w, iso, lo, hi):
    """rn_surface_count_valid / rn_surface_emit_valid at a level, as
    mesh.surface_nets calls rn_surface_*"""
    res = tuple(int(s) - 1 for s in reversed(sig.shape))
    lo, step = mesh._box("t", (lo, hi), res)
    dev, st, L = sig.device, torch.cuda.current_stream(sig.device).cuda_stream, lib()
    work = torch.empty(mesh.surface_work_bytes(res), dtype=torch.uint8, device=dev)
    iso = float(np.float32(iso))
    L.surface_count_valid(sig.data_ptr(), w.data_ptr(), *res, iso, work.data_ptr(), st)
    n_v, n_q = work[:16].view(torch.int64).tolist()
    v, nr = torch.empty(n_v, 3, device=dev), torch.empty(n_v, 3, device=dev)
    f = torch.empty(2 * n_q, 3, dtype=torch.int32, device=dev)
    L.surface_emit_valid(sig.data_ptr(), w.data_ptr(), *res, iso, lo.ctypes.data, step.ctypes.data,
                         work.data_ptr(), n_v, n_q, v.data_ptr() if n_v else None,
                         nr.data_ptr() if n_v else None, f.data_ptr() if n_q else None, st)
    return v, f, nr


@pytest.mark.parametrize("name", list(LATTICES))
def test_all_valid_equals_surface_nets(cuda, name):
    s, lo, step, hi, iso = LATTICES[name]()
    sig = torch.from_numpy(s).to(cuda)
    want = mesh.surface_nets(sig, iso, (lo, hi))
    v, f, nr = _valid_nets(sig, torch.ones_like(sig), iso, lo, hi)
    if name == "smooth":
        assert len(v) > 8 * 1024                          # many counting blocks
    assert torch.equal(f, want.faces)
    assert torch.equal(v.view(torch.int32), want.vertices.view(torch.int32))
    assert torch.equal(nr.view(torch.int32), want.normals.view(torch.int32))


@pytest.mark.parametrize("name", ["sphere24", "noise", "smooth"])
def test_valid_nets_with_holes_match_reference(cuda, name):
    """a fifth of the points unobserved, at random: the two rules, against the
    numpy restatement"""
    s, lo, step, hi, iso = LATTICES[name]()
    w = (np.random.default_rng(5).uniform(size=s.shape) > 0.2).astype(np.float32)
    w *= np.random.default_rng(6).integers(1, 7, s.shape).astype(np.float32)
    v, f, nr = T.surface_nets_valid(s, w, iso, lo, step)
    full = R.surface_nets(s, iso, lo, step)
    assert 0 < len(v) < len(full[0]) and 0 < len(f) < len(full[1])
    gv, gf, gn = _valid_nets(torch.from_numpy(s).to(cuda), torch.from_numpy(w).to(cuda), iso, lo, hi)
    _compare(SimpleNamespace(vertices=gv, faces=gf, normals=gn), v, f, nr,
             float(np.abs(np.stack([lo, hi])).max()))


def test_launches_that_observe_nothing_leave_the_volume(cuda):
    sc = T.scene()
    vol = tsdf.TSDFVolume(sc.res, BOX, trunc=sc.trunc, device=cuda)
    vol.integrate(**_dev(sc, cuda, slice(0, 2)))
    before = _state(vol)
    assert before["w"].any() and before["wc"].any()
    a = _dev(sc, cuda, slice(0, 1))
    # a camera behind every point: it looks away from the box
    away = torch.from_numpy(T.look_at((0.0, 0.0, 2.0), (0.0, 0.1, 4.0), (0.1, 1.0, 0.0))[None]
                            .astype(np.float32)).to(cuda)
    vol.integrate(**dict(a, poses=away))
    _same_bits(_state(vol), before)
    # every pixel a miss, and no carving
    vol.integrate(carve=False, **dict(a, opacity=torch.zeros_like(a["opacity"])))
    _same_bits(_state(vol), before)
    # no camera at all
    e = _dev(sc, cuda, slice(0, 0))
    assert e["poses"].shape == (0, 3, 4) and e["depth"].shape == (0, sc.W * sc.H)
    vol.integrate(**e)
    _same_bits(_state(vol), before)
    # (with carving the same misses do write)
    vol.integrate(carve=True, **dict(a, opacity=torch.zeros_like(a["opacity"])))
    assert (_state(vol)["w"] != before["w"]).any()


def test_one_cell_lattice(cuda):
    """1 x 1 x 1 cells: 8 points, one block, the box's corners"""
    sc = T.scene()
    lo, step = R.box_step(*BOX, (1, 1, 1))
    one = SimpleNamespace(**dict(vars(sc), res=(1, 1, 1), lo=lo, step=step, n_pts=8, trunc=4.0))
    want = T.fresh(8)
    T.integrate(want, one)
    assert not T.decisions64(one)[2].any() and (want["w"] > 0).all()
    vol = tsdf.TSDFVolume(1, BOX)                         # the default device, "cuda"
    assert vol.trunc == 4.0 and vol.device == vol.phi.device
    vol.integrate(**_dev(sc, cuda))
    _same_bits(_state(vol), want)
    got = vol.extract()
    v, f, nr = T.surface_nets_valid(want["phi"].reshape(2, 2, 2), want["w"].reshape(2, 2, 2), 0.0,
                                    lo, step)
    assert got.vertices.shape == (len(v), 3) and got.faces.shape == (0, 3) and len(f) == 0
    assert got.colors.shape == (len(v), 3)


# ---- a model ----------------------------------------------------------------------------
RES_IMG, N_IMG = 24, 6
OPACITY_MIN = 0.05           # an untrained model renders thin fog: trust it, the mesh is a test's


@pytest.fixture(scope="module")
def rig(cuda):
    sc = S.parity_scene(2, device=cuda)
    dirs, poses = S.ring_cameras(N_IMG, RES_IMG)
    half = 0.3                                           # ring_cameras' default half-width
    f = (RES_IMG - 1) / (2 * half)                       # its directions, as a pinhole
    K = np.array([[f, 0, RES_IMG / 2], [0, f, RES_IMG / 2], [0, 0, 1]])
    return SimpleNamespace(sc=sc, dirs=dirs.to(cuda), poses=poses.to(cuda), K=K,
                           wh=(RES_IMG, RES_IMG))


def test_fuse_mesh_equals_its_composition(rig, cuda):
    from radnerf_amd.evaluate import ImageEvaluator
    m, g = rig.sc.m, rig.sc.g
    kw = dict(resolution=(20, 18, 16), opacity_min=OPACITY_MIN)
    got = tsdf.fuse_mesh(m, g, rig.poses, rig.dirs, rig.wh, rig.K, batch=4, **kw)
    ev = ImageEvaluator(m, g, rig.dirs, rig.wh)
    outs = []
    for p in rig.poses:
        o = ev.render_image(p)
        outs.append({k: o[k].clone() for k in ("depth", "opacity", "rgb")})
    op = torch.stack([o["opacity"] for o in outs])
    print(f"opacity: max {float(op.max()):.3f}, share >= {OPACITY_MIN}: "
          f"{float((op >= OPACITY_MIN).float().mean()):.3f}")
    assert (op >= OPACITY_MIN).any()
    vol = tsdf.TSDFVolume(kw["resolution"], mesh._model_box(m), device=cuda)
    for p, o in zip(rig.poses, outs):
        vol.integrate(o["depth"][None], o["opacity"][None], p[None].contiguous(), rig.K, rig.dirs,
                      rig.wh, rgb=o["rgb"][None], opacity_min=OPACITY_MIN)
    want = vol.extract()
    print(f"V {want.vertices.shape[0]} F {want.faces.shape[0]}")
    assert want.vertices.shape[0] > 0 and want.faces.shape[0] > 0
    one = tsdf.fuse_mesh(m, g, rig.poses, rig.dirs, rig.wh, rig.K, batch=1, **kw)
    for other in (got, one):
        assert torch.equal(other.faces, want.faces)
        assert torch.equal(other.vertices.view(torch.int32), want.vertices.view(torch.int32))
        assert torch.equal(other.normals.view(torch.int32), want.normals.view(torch.int32))
        assert torch.equal(other.colors, want.colors)
    kept = tsdf.fuse_mesh(m, g, rig.poses, rig.dirs, rig.wh, rig.K, keep_largest=1, colors=False,
                          **kw)
    assert kept.colors is None and 0 < kept.vertices.shape[0] <= want.vertices.shape[0]
    assert int(mesh.components(kept).n_vertices.numel()) == 1


def test_trainer_export_mesh_tsdf(rig, cuda, tmp_path):
    from radnerf_amd.trainer import Trainer
    sc = rig.sc
    tr = Trainer(sc.m, sc.g, 256, directions=rig.dirs, poses=rig.poses, img_wh=rig.wh,
                 intrinsics=rig.K)

    def snapshot():
        d = {"m." + k: v.clone() for k, v in sc.m.state_dict().items()}
        d.update({"g." + k: v.clone() for k, v in sc.g.state_dict().items()})
        for i, q in enumerate(list(sc.m.parameters()) + list(sc.g.parameters())):
            if q.grad is not None:
                d[f"grad.{i}"] = q.grad.clone()
        for i, (_, st) in enumerate(sorted(tr.opt.state.items(), key=lambda kv: id(kv[0]))):
            d.update({f"opt.{i}.{k}": v.clone() for k, v in st.items() if torch.is_tensor(v)})
        return d, tr.global_step

    before, step = snapshot()
    p = str(tmp_path / "model.ply")
    out = tr.export_mesh(p, method="tsdf", resolution=16, opacity_min=OPACITY_MIN)
    assert out.vertices.shape[0] > 0 and out.vertices.is_cuda and out.colors is not None
    back = mesh.load_ply(p)
    assert torch.equal(back.vertices, out.vertices.cpu())
    assert torch.equal(back.faces, out.faces.cpu())
    assert torch.equal(back.normals, out.normals.cpu())
    assert torch.equal(back.colors, out.colors.cpu())
    same = tsdf.fuse_mesh(sc.m, sc.g, rig.poses, rig.dirs, rig.wh, rig.K, resolution=16,
                          opacity_min=OPACITY_MIN, exp_step_factor=tr.esf, **tr.routing)
    assert torch.equal(same.faces, out.faces) and torch.equal(same.vertices, out.vertices)
    # fewer poses, given by the call
    part = tr.export_mesh(str(tmp_path / "part.obj"), method="tsdf", poses=rig.poses[:2],
                          resolution=16, opacity_min=OPACITY_MIN, colors=False)
    assert part.colors is None
    after, step2 = snapshot()
    assert step2 == step and set(after) == set(before)
    for k in before:
        assert torch.equal(before[k], after[k]), k
