"""CPU: the training state's format, file and checks (radnerf_amd.train_state,
Trainer.state_dict / load_state_dict / save_state / load_state, fit_resumable's
checkpoint arguments, export_reference / load_reference).  The GPU side --
that a resumed run equals the uninterrupted one bit for bit -- is
tests/test_gpu_resume.py.

The trainer here is assembled without a device (Trainer.__new__ and the
attributes the state reads, the pattern of tests/test_sampler_api.py): a real
MNGP / Ray_Gate with a small hash table on the CPU, a FusedAdam whose moments
are filled by hand.  With `no_library`, loading librn.so fails the test.
"""
import inspect
import math
import os

import pytest
import torch

from radnerf_amd import _lib, checkpoint, sampler
from radnerf_amd import train_state as TS
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.optim import FusedAdam
from radnerf_amd.trainer import Trainer

K, SCALE, N_IMG = 2, 0.5, 3


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (sampler, _lib):
        monkeypatch.setattr(mod, "lib", boom)


def _trainer(ext=True, seed=1, filled=True, **over):
    """a Trainer on the CPU with everything the state reads, nothing else"""
    gen = torch.Generator().manual_seed(100 + seed)
    tr = Trainer.__new__(Trainer)
    tr.model, tr.gate = MNGP(SCALE, size=K, t=8, seed=seed), Ray_Gate(K, seed=seed + 1)
    tr.device = torch.device("cpu")
    tr.optimize_ext = ext
    tr.poses = torch.rand(N_IMG, 3, 4, generator=gen)
    tr.directions = torch.rand(16, 3, generator=gen)
    params = [tr.model.xyz_encoder.params, tr.model.mlp_params, tr.gate.params]
    groups = [dict(params=params)]
    if ext:
        tr.dR = torch.nn.Parameter(torch.rand(N_IMG, 3, generator=gen) * 1e-3)
        tr.dT = torch.nn.Parameter(torch.rand(N_IMG, 3, generator=gen) * 1e-3)
        groups.append(dict(params=[tr.dR, tr.dT], lr=1e-8, eps=1e-8))
    tr.opt = FusedAdam(groups, lr=1e-2, eps=1e-15)
    tr.n_rays, tr.seed, tr.update_interval, tr.warmup_steps = 512, 3, 16, 256
    tr.lr0, tr.pose_lr, tr.esf = 1e-2, 1e-8, 0.0
    tr.random_bg, tr.erode, tr.deterministic = False, False, True
    tr.lambdas = dict(lambda_opacity=1e-3, lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3,
                      lambda_distortion=0.0)
    tr.global_step, tr.images, tr.img_wh = 0, None, None
    tr.last_batch = tr._evaluator = tr._fit_progress = tr._saver = None
    for k, v in over.items():
        setattr(tr, k, v)
    if filled:
        with torch.no_grad():
            for i in range(K):
                getattr(tr.model, f"density_grid_{i}").copy_(
                    torch.rand(tr.model.cascades, 128 ** 3, generator=gen))
                bits = getattr(tr.model, f"density_bitfield_{i}")
                bits.copy_(torch.randint(256, bits.shape, generator=gen).to(torch.uint8))
        for j, (_, p) in enumerate(tr._named_params()):
            tr.opt.state[p] = {"step": 37 + j, "exp_avg": torch.rand(p.shape, generator=gen),
                               "exp_avg_sq": torch.rand(p.shape, generator=gen)}
        tr.opt.param_groups[0]["lr"] = 0.00731
        tr.global_step = 37
    return tr


@pytest.fixture(scope="module")
def saved():
    """one filled trainer's state_dict, made once and never written to"""
    return _trainer().state_dict()


# ---- the state and its file ---------------------------------------------------
def _walk(obj, path="state"):
    """every leaf of a loaded object: tensors and plain values only"""
    if isinstance(obj, dict):
        assert all(type(k) is str for k in obj), path
        for k, v in obj.items():
            _walk(v, f"{path}/{k}")
    elif type(obj) is list:
        for i, v in enumerate(obj):
            _walk(v, f"{path}/{i}")
    else:
        assert type(obj) in (torch.Tensor, int, float, str, bool), (path, type(obj))
        if torch.is_tensor(obj):
            assert obj.device.type == "cpu" and not obj.requires_grad, path


def _same(a, b):
    ta, tb = dict(TS.tensors(a)), dict(TS.tensors(b))
    assert set(ta) == set(tb)
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and torch.equal(ta[k], tb[k]), k

    def plain(s):
        if torch.is_tensor(s):
            return tuple(s.shape)
        if isinstance(s, dict):
            return {k: plain(v) for k, v in s.items()}
        return [plain(v) for v in s] if isinstance(s, list) else s
    assert plain(a) == plain(b)


def test_state_holds_what_the_table_says(saved):
    _walk(saved)
    assert set(saved) == {"header", "structure", "hyper", "model", "poses", "optimizer",
                          "progress", "generators"}
    assert saved["header"]["version"] == TS.VERSION == 1
    assert set(saved["structure"]) == {"K", "scale", "cascades", "grid_size", "table_len",
                                       "gate_out_dim", "gate_type", "optimize_ext", "n_images",
                                       "world_size"}
    assert set(saved["hyper"]) == {
        "n_rays", "seed", "update_interval", "warmup_steps", "lr0", "pose_lr", "lambda_opacity",
        "lambda_cv_importance", "lambda_depth_mutual", "lambda_distortion", "esf", "random_bg",
        "erode", "deterministic", "adam.0.betas", "adam.0.eps", "adam.1.betas", "adam.1.eps"}
    want = {"xyz_encoder.params", "mlp_params", "gating_net.params", "center", "xyz_min",
            "xyz_max", "half_size"}
    want |= {f"density_{w}_{i}" for w in ("grid", "bitfield") for i in range(K)}
    assert set(saved["model"]) == want                # no count_grid: the model has none
    assert saved["model"]["xyz_encoder.params"].dtype == torch.float32
    assert set(saved["poses"]) == {"dR", "dT"}
    assert set(saved["optimizer"]["state"]) == {"xyz_encoder.params", "mlp_params",
                                                "gating_net.params", "dR", "dT"}
    assert saved["optimizer"]["state"]["mlp_params"]["step"] == 38
    assert [g["lr"] for g in saved["optimizer"]["groups"]] == [0.00731, 1e-8]
    assert saved["progress"] == {"global_step": 37}   # no epoch position outside fit
    assert set(saved["generators"]) == {"cpu"}
    # every tensor has its size and checksum in the header
    table = saved["header"]["tensors"]
    assert set(table) == {p for p, _ in TS.tensors({k: v for k, v in saved.items()
                                                   if k != "header"})}
    n = saved["model"]["mlp_params"].numel() * 4
    assert table["model/mlp_params"]["bytes"] == n
    # a count_grid and no pose refinement: the parts come and go with them
    tr = _trainer(ext=False, filled=False)
    tr.model.count_grid = torch.rand(tr.model.cascades, 128 ** 3)
    sd = tr.state_dict()
    assert "poses" not in sd and "count_grid" in sd["model"]
    assert sd["optimizer"]["state"]["mlp_params"]["step"] == 0
    assert not sd["optimizer"]["state"]["mlp_params"]["exp_avg"].any()


def test_round_trip_through_a_file(tmp_path):
    src = _trainer()
    saved = src.state_dict()
    path = str(tmp_path / "state.pt")
    assert src.save_state(path).wait() == path
    raw = torch.load(path, map_location="cpu", weights_only=True)
    _walk(raw)
    _same(raw, saved)
    dst = _trainer(seed=7, filled=False)
    assert not torch.equal(dst.model.mlp_params, src.model.mlp_params)
    v0 = dst.model.mlp_params._version
    torch.rand(3)                                      # the generator moves on
    dst.load_state(path)
    _same(dst.state_dict(), saved)
    assert dst.global_step == 37 and dst.opt.param_groups[0]["lr"] == 0.00731
    assert dst.opt.state[dst.dR]["step"] == 40
    # written in place: the derived caches' key moved
    assert dst.model.mlp_params._version > v0
    assert torch.equal(dst.model.mlp_params, src.model.mlp_params)
    import numpy as np
    assert np.array_equal(dst.model._h_min, src.model._h_min)
    # the same through a background save on this device
    h = src.save_state(path, background=True)
    src.global_step = 99                               # after the call: not in the file
    assert h.wait() == path and h.done()
    src.wait_saves()
    assert TS.read_file(path)["progress"]["global_step"] == 37
    assert os.listdir(tmp_path) == ["state.pt"]


def test_a_failed_write_leaves_the_earlier_file(saved, tmp_path, monkeypatch):
    ckpt = tmp_path / "ckpt"
    ckpt.mkdir()
    path = str(ckpt / TS.checkpoint_name(1))
    TS.write_file(dict(saved), path)
    before = open(path, "rb").read()

    def refuse(*a, **k):
        raise OSError("no space left on device")
    monkeypatch.setattr(TS.os, "replace", refuse)
    tr = _trainer()
    tr.global_step = 38
    with pytest.raises(OSError, match="no space"):
        tr.save_state(path)
    with pytest.raises(OSError, match="no space"):
        tr.save_state(str(ckpt / TS.checkpoint_name(2)))
    h = tr.save_state(str(ckpt / TS.checkpoint_name(3)), background=True)
    with pytest.raises(OSError, match="no space"):
        h.wait()
    tr.wait_saves()                                    # the error was handed over once
    assert open(path, "rb").read() == before
    assert os.listdir(ckpt) == [TS.checkpoint_name(1)]     # nothing partial, no leftovers
    assert TS.read_file(path)["progress"]["global_step"] == 37


def test_lookup_and_keep(saved, tmp_path):
    ckpt = str(tmp_path)
    assert TS.list_checkpoints(ckpt) == [] and TS.newest_checkpoint(ckpt) is None
    assert TS.newest_checkpoint(str(tmp_path / "absent")) is None
    for epoch in (1, 2, 3, 12):
        st = dict(saved, progress={"global_step": 10 * epoch})
        TS.write_file(st, os.path.join(ckpt, TS.checkpoint_name(epoch)))
    # temporary and foreign names are not checkpoints
    tmp = TS._tmp_name(os.path.join(ckpt, TS.checkpoint_name(13)))
    assert os.path.dirname(tmp) == ckpt and not TS.NAME.match(os.path.basename(tmp))
    for name in (os.path.basename(tmp), "state_epoch0014.pt.part", "notes.txt",
                 "state_epoch15.pt"):
        open(os.path.join(ckpt, name), "wb").write(b"half a file")
    assert [e for e, _ in TS.list_checkpoints(ckpt)] == [1, 2, 3, 12]
    path, state = TS.newest_checkpoint(ckpt)
    assert os.path.basename(path) == "state_epoch0012.pt"
    assert state["progress"]["global_step"] == 120
    # a damaged newest file is passed over for the one before it
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) // 2)
    path, state = TS.newest_checkpoint(ckpt)
    assert os.path.basename(path) == "state_epoch0003.pt"
    TS.prune(ckpt, 2)
    assert [e for e, _ in TS.list_checkpoints(ckpt)] == [3, 12]
    assert "notes.txt" in os.listdir(ckpt)             # only its own files go
    TS.prune(ckpt, 5)
    assert [e for e, _ in TS.list_checkpoints(ckpt)] == [3, 12]


# ---- integrity ------------------------------------------------------------------
def test_one_flipped_byte_names_the_file_and_the_tensor(saved, tmp_path):
    path = str(tmp_path / "state.pt")
    TS.write_file(dict(saved), path)
    blob = bytearray(open(path, "rb").read())
    needle = saved["model"]["gating_net.params"].numpy().tobytes()
    at = bytes(blob).find(needle)
    assert at > 0 and bytes(blob).find(needle, at + 1) < 0
    blob[at + len(needle) // 2] ^= 0x10
    open(path, "wb").write(bytes(blob))
    tr = _trainer(seed=7, filled=False)
    before = tr.model.mlp_params.detach().clone()
    with pytest.raises(ValueError) as e:
        tr.load_state(path)
    assert path in str(e.value) and "model/gating_net.params" in str(e.value)
    assert "checksum" in str(e.value)
    assert torch.equal(tr.model.mlp_params, before) and tr.global_step == 0
    # the same check guards a dict handed over in memory
    bad = dict(saved, model=dict(saved["model"], center=saved["model"]["center"] + 1))
    with pytest.raises(ValueError, match="model/center"):
        tr.load_state_dict(bad)


def test_truncated_and_foreign_files_name_the_file(saved, tmp_path):
    path = str(tmp_path / "state.pt")
    TS.write_file(dict(saved), path)
    size = os.path.getsize(path)
    tr = _trainer(seed=7, filled=False)
    for cut in (size - 1, size // 2, 100, 0):
        with open(path, "r+b") as f:
            f.truncate(cut)
        with pytest.raises(ValueError) as e:
            tr.load_state(path)
        assert path in str(e.value), cut
    with pytest.raises(ValueError) as e:
        tr.load_state(str(tmp_path / "absent.pt"))
    assert "absent.pt" in str(e.value)
    # a pickle that is not a state, and one weights_only refuses
    torch.save({"state_dict": {}}, path)
    with pytest.raises(ValueError) as e:
        tr.load_state(path)
    assert path in str(e.value) and "header" in str(e.value)
    torch.save({"fn": os.getcwd}, path)
    with pytest.raises(ValueError) as e:
        tr.load_state(path)
    assert path in str(e.value)
    assert tr.global_step == 0


def test_wrong_version_names_the_file(saved, tmp_path):
    path = str(tmp_path / "state.pt")
    st = dict(saved, header=dict(saved["header"], version=TS.VERSION + 1))
    TS.atomic_save(st, path)
    with pytest.raises(ValueError) as e:
        _trainer(seed=7, filled=False).load_state(path)
    assert path in str(e.value) and "version 2" in str(e.value)
    with pytest.raises(ValueError, match="version"):
        TS.verify(dict(saved, header=dict(saved["header"], version="1")))
    with pytest.raises(ValueError, match="ndarray|plain|is a"):
        TS.check_plain({"a": {"b": [1, 2.0, (3,)]}})


# ---- the two compatibility checks -----------------------------------------------
OTHER = {"K": 3, "scale": 16.0, "cascades": 6, "grid_size": 64, "table_len": 12, "gate_out_dim": 4,
         "gate_type": "image", "optimize_ext": False, "n_images": 5, "world_size": 2}


@pytest.mark.parametrize("field", sorted(OTHER))
def test_each_structural_field_is_reported(saved, field):
    tr = _trainer(seed=7, filled=False)
    own = tr._structure()[field]
    assert own != OTHER[field]
    st = dict(saved, structure=dict(saved["structure"], **{field: OTHER[field]}))
    for override in (False, True):                      # override does not excuse structure
        with pytest.raises(ValueError) as e:
            tr.load_state_dict(st, override=override)
        msg = str(e.value)
        assert "structure" in msg
        assert f"{field}: saved {OTHER[field]!r}, this trainer {own!r}" in msg
    assert tr.global_step == 0


def test_structure_lists_every_differing_field(saved):
    tr = _trainer(seed=7, filled=False)
    st = dict(saved, structure=dict(saved["structure"], K=3, world_size=2))
    with pytest.raises(ValueError) as e:
        tr.load_state_dict(st)
    assert "K: saved 3, this trainer 2" in str(e.value)
    assert "world_size: saved 2, this trainer 1" in str(e.value)


HYPER = {"n_rays": 1024, "seed": 4, "update_interval": 8, "warmup_steps": 128, "lr0": 2e-2,
         "pose_lr": 1e-7, "lambda_opacity": 2e-3, "lambda_cv_importance": 0.0,
         "lambda_depth_mutual": 0.5, "lambda_distortion": 1e-3, "esf": 1 / 256, "random_bg": True,
         "erode": True, "deterministic": False, "adam.0.betas": [0.8, 0.99], "adam.0.eps": 1e-8,
         "adam.1.betas": [0.9, 0.9], "adam.1.eps": 1e-15}


def test_hyper_table_is_complete(saved):
    assert set(HYPER) == set(saved["hyper"])


@pytest.mark.parametrize("field", sorted(HYPER))
def test_each_hyper_parameter_is_reported(saved, field):
    tr = _trainer(seed=7, filled=False)
    own = tr._hyper()[field]
    assert own != HYPER[field]
    st = dict(saved, hyper=dict(saved["hyper"], **{field: HYPER[field]}))
    with pytest.raises(ValueError) as e:
        tr.load_state_dict(st)
    msg = str(e.value)
    assert "override=True" in msg
    assert f"{field}: saved {HYPER[field]!r}, this trainer {own!r}" in msg
    assert tr.global_step == 0
    tr.load_state_dict(st, override=True)               # the trainer's own value stands
    assert tr.global_step == 37 and tr._hyper()[field] == own


# ---- fit --------------------------------------------------------------------------
def _fake_images(n_images, n_pix):
    ti = sampler.TrainImages.__new__(sampler.TrainImages)
    ti.images = torch.zeros(n_images, n_pix, 3, dtype=torch.uint8)
    ti.n_images, ti.n_pix, ti.dtype_code = n_images, n_pix, 0
    ti.device = ti.images.device
    return ti


def test_fit_checkpoint_argument_checks(no_library, saved, tmp_path):
    p = inspect.signature(Trainer.fit_resumable).parameters
    assert [(k, p[k].default) for k in list(p)[-4:]] == [
        ("ckpt_dir", None), ("ckpt_every", None), ("keep", 2), ("resume", False)]
    # fit keeps its argument list: fit_resumable's without the last four
    f = inspect.signature(Trainer.fit).parameters
    assert [(k, f[k].default) for k in f] == [(k, p[k].default) for k in list(p)[:-4]]
    q = inspect.signature(Trainer.save_state).parameters
    assert q["background"].default is False
    assert inspect.signature(Trainer.load_state).parameters["override"].default is False
    assert inspect.signature(Trainer.load_state_dict).parameters["override"].default is False
    assert inspect.signature(Trainer.export_reference).parameters["save_poses"].default is None
    tr = _trainer(seed=7, filled=False, images=_fake_images(N_IMG, 16))
    ckpt = str(tmp_path)
    with pytest.raises(ValueError, match="ckpt_every needs ckpt_dir"):
        tr.fit_resumable(ckpt_every=1)
    with pytest.raises(ValueError, match="ckpt_every must be at least 1"):
        tr.fit_resumable(ckpt_dir=ckpt, ckpt_every=0)
    with pytest.raises(ValueError, match="keep must be at least 1"):
        tr.fit_resumable(ckpt_dir=ckpt, keep=0)
    with pytest.raises(ValueError, match=r"resume=True\) needs ckpt_dir"):
        tr.fit_resumable(resume=True)
    # a saved schedule other than the call's: before anything is loaded
    fit = {"num_epochs": 3, "steps_per_epoch": 10, "eta_min": 1e-2 / 30, "next_epoch": 1,
           "log": [{"epoch": 0, "lr": 1e-2}]}
    st = dict(saved, progress={"global_step": 37, "fit": fit})
    path = TS.write_file(st, os.path.join(ckpt, TS.checkpoint_name(1)))
    for kw, msg in ((dict(num_epochs=4, steps_per_epoch=10), "num_epochs: saved 3, this call 4"),
                    (dict(num_epochs=3, steps_per_epoch=11),
                     "steps_per_epoch: saved 10, this call 11"),
                    (dict(num_epochs=3, steps_per_epoch=10, eta_min=0.0), "eta_min: saved")):
        for resume in (True, path):
            with pytest.raises(ValueError) as e:
                tr.fit_resumable(ckpt_dir=ckpt, resume=resume, **kw)
            assert msg in str(e.value) and path in str(e.value)
    # a state saved outside fit has no epoch position
    by_hand = TS.write_file(dict(saved), str(tmp_path / "by_hand.pt"))
    with pytest.raises(ValueError, match="no epoch position"):
        tr.fit_resumable(3, 10, resume=by_hand)
    assert tr.global_step == 0 and not tr.opt.state[tr.model.mlp_params]


def test_fit_writes_keeps_and_resumes_on_the_schedule(no_library, monkeypatch, tmp_path):
    """fit_resumable's bookkeeping with the step replaced by a stub (the real step is
    tests/test_gpu_resume.py::test_fit_resumes): the files, `keep`, the log,
    and the resumed epoch's lr, which is sampler.cosine_lr's."""
    lrs = []

    def stub(self):
        lrs.append(self.opt.param_groups[0]["lr"])
        self.global_step += 1
        return {"rgb": torch.tensor(0.25), "opacity": torch.tensor(0.5)}
    monkeypatch.setattr(Trainer, "step_sampled", stub)
    ckpt = str(tmp_path / "ckpt")
    E, S, eta = 5, 3, 1e-4

    class Stop(Exception):
        pass

    def stop(entry):
        # the epoch's file is complete or on its way before the callback
        if entry["epoch"] == 2:
            raise Stop
    a = _trainer(filled=False, images=_fake_images(N_IMG, 16))
    with pytest.raises(Stop):
        a.fit_resumable(E, S, eta_min=eta, ckpt_dir=ckpt, ckpt_every=1, keep=2, callback=stop)
    assert a._fit_progress is None                       # absent outside fit
    assert sorted(os.listdir(ckpt)) == [TS.checkpoint_name(2), TS.checkpoint_name(3)]
    st = TS.read_file(os.path.join(ckpt, TS.checkpoint_name(3)))
    assert st["progress"]["global_step"] == 3 * S
    assert st["progress"]["fit"]["next_epoch"] == 3
    assert [e["epoch"] for e in st["progress"]["fit"]["log"]] == [0, 1, 2]
    del lrs[:]
    b = _trainer(seed=7, filled=False, images=_fake_images(N_IMG, 16))
    log = b.fit_resumable(E, S, eta_min=eta, ckpt_dir=ckpt, ckpt_every=2, keep=1, resume=True)
    assert b.global_step == E * S and [e["epoch"] for e in log] == list(range(E))
    assert lrs == [sampler.cosine_lr(1e-2, e, E, eta) for e in (3, 4) for _ in range(S)]
    assert [e["lr"] for e in log] == [sampler.cosine_lr(1e-2, e, E, eta) for e in range(E)]
    assert log[4]["terms"] == {"rgb": 0.25, "opacity": 0.5} and log[4]["loss"] == 0.75
    assert log[4]["train_psnr"] == -10 * math.log10(0.25)
    # every 2 epochs and after the last: 4 and 5; keep=1 leaves the last
    assert os.listdir(ckpt) == [TS.checkpoint_name(5)]
    # resume=True with an empty directory starts fresh
    c = _trainer(filled=False, images=_fake_images(N_IMG, 16))
    log = c.fit_resumable(2, 1, ckpt_dir=str(tmp_path / "none"), resume=True)
    assert [e["epoch"] for e in log] == [0, 1]
    # blocking checkpoints on request
    c.ckpt_background = False
    c.global_step = 0
    c.fit_resumable(2, 1, ckpt_dir=str(tmp_path / "blocking"))
    assert os.listdir(tmp_path / "blocking") == [TS.checkpoint_name(2)]


# ---- the reference's slim checkpoint ------------------------------------------------
def _lightning_keys(tr):
    """the Lightning module's state_dict keys (train_ml.py:74-78, 126-134)"""
    keys = set(checkpoint.reference_state_dict(tr.model, tr.gate)["state_dict"])
    keys |= {"directions", "poses"}
    return keys | ({"dR", "dT"} if tr.optimize_ext else set())


def _slim(keys, save_poses):
    """utils/util.py:33-43 on a key set"""
    pop = ["directions", "model.density_grid", "model.grid_coords"]
    if not save_poses:
        pop += ["poses"]
    pop += [k for k in keys if k.startswith("val_lpips")]
    return set(keys) - set(pop)


@pytest.mark.parametrize("save_poses", [False, True, None])
@pytest.mark.parametrize("ext", [False, True])
def test_export_reference_keys(tmp_path, ext, save_poses):
    tr = _trainer(ext=ext)
    path = str(tmp_path / "slim.ckpt")
    tr.export_reference(path, save_poses=save_poses)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    want = _slim(_lightning_keys(tr), ext if save_poses is None else save_poses)
    assert set(sd) == want
    assert "model.grid_coords" not in sd and "directions" not in sd
    assert all(f"model.density_grid_{i}" in sd for i in range(K))    # the rule, literally
    assert ("dR" in sd) == ext and ("poses" in sd) == (ext if save_poses is None else save_poses)
    if "poses" in sd:
        assert torch.equal(sd["poses"], tr.poses)
    if ext:
        assert torch.equal(sd["dR"], tr.dR.detach()) and torch.equal(sd["dT"], tr.dT.detach())
    assert os.listdir(tmp_path) == ["slim.ckpt"]


def test_load_reference_restores_the_poses(tmp_path):
    src = _trainer(ext=True)
    path = str(tmp_path / "slim.ckpt")
    src.export_reference(path)
    dst = _trainer(ext=True, seed=7, filled=False)
    assert not torch.equal(dst.dR, src.dR)
    dst.load_reference(path)
    assert torch.equal(dst.dR, src.dR) and torch.equal(dst.dT, src.dT)
    # the weights went through the reference's f16
    f16 = lambda t: t.detach().half().float()
    assert torch.equal(dst.model.xyz_encoder.params, f16(src.model.xyz_encoder.params))
    assert torch.equal(dst.model.mlp_params, f16(src.model.mlp_params))
    assert torch.equal(dst.gate.params, f16(src.gate.params))
    assert torch.equal(dst.model.density_bitfield_1, src.model.density_bitfield_1)
    assert torch.equal(dst.model.density_grid_0, src.model.density_grid_0)
    # a trainer without pose refinement refuses a file with corrections
    with pytest.raises(ValueError, match="optimize_ext=False"):
        _trainer(ext=False, seed=7, filled=False).load_reference(path)
    # and one without them leaves dR / dT alone
    plain = _trainer(ext=False)
    plain.export_reference(path)
    before = dst.dR.detach().clone()
    dst.load_reference(path)
    assert torch.equal(dst.dR, before)
