"""CPU: the argument checks and the state layout of error-guided sampling
(sampler.GuidedSampler, FusedMLRenderer.train_step(ray_weight=, guided=),
Trainer(guided=True)), and the four C entries' declarations and checks.  Every
ValueError comes before the library is loaded or anything is allocated
(`no_library`, the pattern of tests/test_sampler_api.py).  The GPU side is
tests/test_gpu_guided.py.
"""
import importlib.util
import inspect
import os
import re

import pytest
import torch

from radnerf_amd import _lib, sampler
from radnerf_amd.fused import FusedMLRenderer
from radnerf_amd.sampler import GuidedSampler
from radnerf_amd.trainer import Trainer

from test_train_state_api import _trainer as _cpu_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "rn_guided_weights": "pliiipppp",
    "rn_sample_batch_guided": "pillpppppulilippppppppiiifppppp",
    "rn_guided_epilogue": "pppplilpppppp",
    "rn_guided_refresh": "ppplfp",
}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (sampler, _lib):
        monkeypatch.setattr(mod, "lib", boom)


def _fake_images(n_images, n_pix):
    """a TrainImages without a device, for the checks that come after it"""
    ti = sampler.TrainImages.__new__(sampler.TrainImages)
    ti.images = torch.zeros(1, 1, 3, dtype=torch.uint8)
    ti.n_images, ti.n_pix, ti.dtype_code = n_images, n_pix, 0
    ti.device = ti.images.device
    return ti


def test_guided_sampler_argument_checks(no_library, monkeypatch):
    def no_alloc(*a, **k):
        raise AssertionError("allocated before the argument check")
    ti, big = _fake_images(3, 37 * 21), _fake_images(4096, 64 * 64)
    for fn in ("ones", "zeros", "empty"):
        monkeypatch.setattr(sampler.torch, fn, no_alloc)
    with pytest.raises(ValueError, match="train_images must be a TrainImages"):
        GuidedSampler(None, (37, 21))
    for tile in (0, 257, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"tile must be an int in 1\.\.256"):
            GuidedSampler(ti, (37, 21), tile=tile)
    with pytest.raises(ValueError, match=r"img_wh \(37, 20\) does not match the images' 777"):
        GuidedSampler(ti, (37, 20))
    with pytest.raises(ValueError, match="img_wh must be"):
        GuidedSampler(ti, None)
    # 2^24 cells: 4096 images of 64 x 64 one-pixel tiles; one image fewer fits
    with pytest.raises(ValueError, match=r"16777216 cells, the map holds fewer than 2\^24"):
        GuidedSampler(big, (64, 64), tile=1)
    assert sampler.guided_geometry("x", 4095, 64 * 64, (64, 64), 1)[5] == (1 << 24) - 4096
    for f in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"uniform_frac must be in \[0, 1\]"):
            GuidedSampler(ti, (37, 21), uniform_frac=f)
    for a in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"alpha must be in \(0, 1\]"):
            GuidedSampler(ti, (37, 21), alpha=a)
    p = inspect.signature(GuidedSampler.__init__).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [
        ("train_images", inspect.Parameter.empty), ("img_wh", inspect.Parameter.empty),
        ("tile", 16), ("uniform_frac", 0.5), ("alpha", 0.5)]
    assert sampler.guided_geometry("x", 3, 37 * 21, (37, 21), 16) == (37, 21, 16, 3, 2, 18)
    for name in ("sample", "accumulate", "refresh", "error_map", "state_dict", "load_state_dict"):
        assert callable(getattr(GuidedSampler, name))
    ps = inspect.signature(GuidedSampler.sample).parameters
    pb = inspect.signature(sampler.sample_batch).parameters
    assert list(ps)[1:] == list(pb)[1:]
    assert sampler.GUIDED_KEYS == sampler.KEYS + ("cell_idx", "ray_weight")


def test_trainer_argument_checks(no_library):
    p = inspect.signature(Trainer.__init__).parameters
    assert [(k, p[k].default) for k in list(p)[-5:]] == [
        ("guided", False), ("guided_tile", 16), ("guided_uniform_frac", 0.5),
        ("guided_alpha", 0.5), ("guided_refresh_every", 16)]
    d, poses = torch.rand(480, 3), torch.rand(2, 3, 4)
    ti = _fake_images(2, 480)
    kw = dict(directions=d, poses=poses, guided=True)
    # raised before the model is looked at
    with pytest.raises(ValueError, match=r"Trainer\(guided=True\) needs images and img_wh"):
        Trainer(None, None, 64, img_wh=(24, 20), **kw)
    with pytest.raises(ValueError, match=r"Trainer\(guided=True\) needs images and img_wh"):
        Trainer(None, None, 64, images=ti, **kw)
    kw.update(images=ti, img_wh=(24, 20))
    for f in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match=r"guided_uniform_frac must be in \(0, 1\]"):
            Trainer(None, None, 64, guided_uniform_frac=f, **kw)
    with pytest.raises(ValueError, match=r"guided_alpha must be in \(0, 1\]"):
        Trainer(None, None, 64, guided_alpha=0.0, **kw)
    with pytest.raises(ValueError, match=r"tile must be an int in 1\.\.256"):
        Trainer(None, None, 64, guided_tile=300, **kw)
    for n in (0, 2.0, True):
        with pytest.raises(ValueError, match="guided_refresh_every must be an int >= 1"):
            Trainer(None, None, 64, guided_refresh_every=n, **kw)


def test_trainer_refuses_data_parallel(no_library, monkeypatch):
    from radnerf_amd import trainer
    monkeypatch.setattr(trainer, "_world", lambda: 2)
    with pytest.raises(ValueError, match="does not run under data parallelism"):
        Trainer(None, None, 64, directions=torch.rand(480, 3), poses=torch.rand(2, 3, 4),
                images=_fake_images(2, 480), img_wh=(24, 20), guided=True)


def test_train_step_takes_the_weights():
    p = inspect.signature(FusedMLRenderer.train_step).parameters
    assert p["ray_weight"].default is None and p["guided"].default is None
    assert list(p)[-2:] == ["ray_weight", "guided"]


# ---- the state ------------------------------------------------------------------
UNGUIDED_KEYS = {"header", "structure", "hyper", "model", "poses", "optimizer", "progress",
                 "generators"}
UNGUIDED_HYPER = {
    "n_rays", "seed", "update_interval", "warmup_steps", "lr0", "pose_lr", "lambda_opacity",
    "lambda_cv_importance", "lambda_depth_mutual", "lambda_distortion", "esf", "random_bg",
    "erode", "deterministic", "adam.0.betas", "adam.0.eps", "adam.1.betas", "adam.1.eps"}
GUIDED_HYPER = {"guided": True, "guided_tile": 16, "guided_uniform_frac": 0.25,
                "guided_alpha": 0.5, "guided_refresh_every": 8}


class _CpuSampler:
    """what the state reads of a GuidedSampler, on the CPU"""
    tile, uniform_frac, alpha, n_cells = 16, 0.25, 0.5, 18

    def __init__(self):
        gen = torch.Generator().manual_seed(9)
        self.emap = torch.rand(18, generator=gen)
        self.acc_sum = torch.randint(1 << 40, (18,), generator=gen)
        self.acc_cnt = torch.randint(1 << 20, (18,), generator=gen).int()


def test_unguided_state_is_what_it_was():
    tr = _cpu_trainer()
    tr.guided = None
    sd = tr.state_dict()
    assert set(sd) == UNGUIDED_KEYS and set(sd["hyper"]) == UNGUIDED_HYPER
    assert not any(k.startswith("guided") for k in sd["header"]["tensors"])
    # a trainer assembled before the option existed has no attribute at all
    del tr.guided
    sd2 = tr.state_dict()
    assert set(sd2) == UNGUIDED_KEYS and sd2["hyper"] == sd["hyper"]


def test_guided_state_carries_the_map():
    tr = _cpu_trainer(guided=_CpuSampler(), guided_refresh_every=8)
    sd = tr.state_dict()
    assert set(sd) == UNGUIDED_KEYS | {"guided"}
    assert {k: sd["hyper"][k] for k in GUIDED_HYPER} == GUIDED_HYPER
    assert set(sd["hyper"]) == UNGUIDED_HYPER | set(GUIDED_HYPER)
    g = sd["guided"]
    assert set(g) == {"emap", "acc_sum", "acc_cnt"}
    assert (g["emap"].dtype, g["acc_sum"].dtype, g["acc_cnt"].dtype) == (
        torch.float32, torch.int64, torch.int32)
    for k in g:
        assert torch.equal(g[k], getattr(tr.guided, k)) and g[k] is not getattr(tr.guided, k)
        assert sd["header"]["tensors"]["guided/" + k]["bytes"] == g[k].numel() * g[k].element_size()
    # a flipped value in the map fails its checksum
    bad = dict(sd, guided=dict(g, emap=g["emap"].clone()))
    bad["guided"]["emap"][3] += 1
    with pytest.raises(ValueError, match="guided/emap fails its checksum"):
        _cpu_trainer(guided=_CpuSampler(), guided_refresh_every=8).load_state_dict(bad)


def test_guided_and_unguided_states_do_not_mix(no_library):
    guided = _cpu_trainer(guided=_CpuSampler(), guided_refresh_every=8).state_dict()
    plain = _cpu_trainer().state_dict()
    tr = _cpu_trainer(seed=7, filled=False)
    with pytest.raises(ValueError) as e:
        tr.load_state_dict(guided)
    assert "override=True" in str(e.value) and "guided: saved True, this trainer '(absent)'" \
        in str(e.value)
    assert tr.global_step == 0
    tr.load_state_dict(guided, override=True)           # the trainer stays unguided
    assert tr.global_step == 37 and "guided" not in tr.state_dict()
    tr = _cpu_trainer(seed=7, filled=False, guided=_CpuSampler(), guided_refresh_every=8)
    with pytest.raises(ValueError, match=r"guided: saved '\(absent\)', this trainer True"):
        tr.load_state_dict(plain)
    assert tr.global_step == 0
    # each of the five is a hyper-parameter
    for k, v in (("guided_tile", 32), ("guided_uniform_frac", 0.5), ("guided_alpha", 0.25),
                 ("guided_refresh_every", 16)):
        st = dict(guided, hyper=dict(guided["hyper"], **{k: v}))
        with pytest.raises(ValueError, match=f"{k}: saved {v!r}, this trainer"):
            tr.load_state_dict(st)


# ---- the C entries ----------------------------------------------------------------
def test_entries_declared_and_bound():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    table = _lib.parse_signature_table(gs.table(hdr))
    for name, codes in ENTRIES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert _lib.binding_signatures()[name] == table[name] == codes, name
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    assert "guided.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define\s+RN_GUIDED_WORK_BYTES\s+%d\b" % _lib.GUIDED_WORK_BYTES, hdr)
    # the header states the stream constants the restatement was written from
    for s in ("0xa0761d6478bd642f", "0xe7037ed1a0b428db"):
        assert s in hdr, s


def _sample(**kw):
    """rn_sample_batch_guided with valid sizes and no pointer, `kw` replacing arguments"""
    a = dict(images=None, image_dtype=0, n_images=3, n_pix=777, directions=None, poses=None,
             dR=None, dT=None, mean_dir=None, seed=1, step=0, rank=0, n_rays=16, n_models=2,
             img_idxs=None, pix_idxs=None, target_rgb=None, rays_o=None, rays_d=None,
             imgs_d=None, noise=None, bg=None, W=37, H=21, tile=16, uniform_frac=0.5, w=None,
             cdf=None, cell_idx=None, ray_weight=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.lib().sample_batch_guided(*a.values())


@pytest.mark.parametrize("kw,msg", [
    (dict(step=-1), r"step must be in \[0, 2\^40\)"),
    (dict(rank=1 << 24), r"rank must be in \[0, 2\^24\)"),
    (dict(image_dtype=2), "image_dtype must be 0"),
    (dict(n_models=0), "bad sizes"),
    (dict(mean_dir=64), "imgs_d and mean_dir must be given together"),
    (dict(tile=0), r"tile must be in 1\.\.256"),
    (dict(tile=257), r"tile must be in 1\.\.256"),
    (dict(W=36), "W \\* H must equal n_pix"),
    (dict(n_rays=0, H=20), "W \\* H must equal n_pix"),
    (dict(uniform_frac=-0.5), r"uniform_frac must be in \[0, 1\]"),
    (dict(uniform_frac=1.5), r"uniform_frac must be in \[0, 1\]"),
    (dict(uniform_frac=float("nan")), r"uniform_frac must be in \[0, 1\]"),
    (dict(n_images=4096, W=64, H=64, n_pix=4096, tile=1), r"n_cells must be below 2\^24"),
    (dict(), "null pointer"),
])
def test_sample_entry_checks_without_gpu(kw, msg):
    with pytest.raises(RuntimeError, match=r"rn_sample_batch_guided failed \(status 1\).*" + msg):
        _sample(**kw)
    assert _sample(n_rays=0) == 0


def test_other_entries_check_without_gpu():
    L = _lib.lib()
    with pytest.raises(RuntimeError, match=r"rn_guided_weights failed.*tile must be in 1\.\.256"):
        L.guided_weights(None, 3, 37, 21, 0, None, None, None, None)
    with pytest.raises(RuntimeError, match=r"rn_guided_weights failed.*n_cells must be below"):
        L.guided_weights(None, 4096, 64, 64, 1, None, None, None, None)
    with pytest.raises(RuntimeError, match="rn_guided_weights failed.*null pointer"):
        L.guided_weights(None, 3, 37, 21, 16, None, None, None, None)
    with pytest.raises(RuntimeError, match="rn_guided_epilogue failed.*given together"):
        L.guided_epilogue(None, None, None, None, 16, 2, 18, 64, None, None, None, None, None)
    with pytest.raises(RuntimeError, match=r"rn_guided_epilogue failed.*n_cells must be in"):
        L.guided_epilogue(None, None, None, None, 16, 2, 0, 64, 64, None, None, None, None)
    with pytest.raises(RuntimeError, match="rn_guided_epilogue failed.*null pointer"):
        L.guided_epilogue(None, None, None, None, 16, 2, 18, None, None, None, None, None, None)
    assert L.guided_epilogue(None, None, None, None, 0, 2, 18, None, None, None, None, None,
                             None) == 0
    for alpha in (0.0, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"rn_guided_refresh failed.*alpha must be in"):
            L.guided_refresh(64, 64, 64, 18, alpha, None)
    with pytest.raises(RuntimeError, match=r"rn_guided_refresh failed.*n_cells must be in"):
        L.guided_refresh(64, 64, 64, 1 << 24, 0.5, None)
    with pytest.raises(RuntimeError, match="rn_guided_refresh failed.*null pointer"):
        L.guided_refresh(None, 64, 64, 18, 0.5, None)
