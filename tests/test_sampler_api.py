"""CPU: the surface of the device-resident training set (tests/test_gpu_sampler.py
and tests/test_gpu_fit.py hold the GPU side).

  * the numpy restatement of the sampler's stream (tests/sampler_ref.py, written
    from the header comment) is uniform, covers the (image, pixel) table, is
    independent across ranks and steps, and its jitter is uniform in [0, 1);
  * sampler.cosine_lr is torch's CosineAnnealingLR(T_max, eta_min = lr / 30);
  * the argument checks of TrainImages, Trainer(images=...), step_sampled and
    fit run before the library is loaded;
  * rn_sample_batch is declared, bound and generated with the same codes, the
    ABI version stays, and its own argument checks return status 1 without a
    device.
"""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import sampler_ref as SR
from radnerf_amd import _lib, sampler
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = "pillpppppulilippppppppp"


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (sampler, _lib):
        monkeypatch.setattr(mod, "lib", boom)


# ---- the stream -------------------------------------------------------------
SEED, N_IMG, N_PIX, STEPS, N = 11, 7, 23 * 37, 64, 8192


@pytest.fixture(scope="module")
def stream():
    """the picks of ranks 0 and 1 over STEPS steps, computed once"""
    out = {}
    for rank in (0, 1):
        p = [SR.picks(SEED, s, rank, N, N_IMG, N_PIX) for s in range(STEPS)]
        out[rank] = (np.stack([a for a, _ in p]), np.stack([b for _, b in p]))
    return out


def _chi2(counts):
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2).sum() / e)


def test_stream_is_uniform(stream):
    img, pix = stream[0]
    assert img.dtype == np.int64 and img.shape == (STEPS, N)
    assert img.min() >= 0 and img.max() < N_IMG and pix.min() >= 0 and pix.max() < N_PIX
    for name, idx, cells in (("image", img, N_IMG), ("pixel", pix, N_PIX),
                             ("joint", img * N_PIX + pix, N_IMG * N_PIX)):
        df = cells - 1
        c2 = _chi2(np.bincount(idx.reshape(-1), minlength=cells).astype(np.float64))
        print(f"chi2 of the {name} index: {c2:.1f} at {df} d.o.f.")
        assert abs(c2 - df) <= 5 * math.sqrt(2 * df), (name, c2, df)
    # every image and every pixel is reached
    assert len(np.unique(img)) == N_IMG and len(np.unique(pix)) == N_PIX


def test_stream_differs_by_rank_and_step(stream):
    cell = {r: stream[r][0] * N_PIX + stream[r][1] for r in (0, 1)}
    other_rank = float((cell[0] == cell[1]).mean())
    other_step = float((cell[0][1:] == cell[0][:-1]).mean())
    frac = (other_rank + other_step) / 2
    print(f"picks equal to the other rank's {other_rank:.2e}, to the next step's "
          f"{other_step:.2e}; by chance {1 / (N_IMG * N_PIX):.2e}")
    assert frac < 1e-3 and other_rank < 1e-3 and other_step < 1e-3
    # another seed is another stream, the same key the same one
    a = SR.picks(SEED + 1, 0, 0, N, N_IMG, N_PIX)
    assert float((a[0] * N_PIX + a[1] == cell[0][0]).mean()) < 1e-3
    b = SR.picks(SEED, 0, 0, N, N_IMG, N_PIX)
    assert np.array_equal(b[0], stream[0][0][0]) and np.array_equal(b[1], stream[0][1][0])
    # a shorter batch is a prefix (pick i depends on i and the key alone)
    c = SR.picks(SEED, 0, 0, 100, N_IMG, N_PIX)
    assert np.array_equal(c[0], b[0][:100]) and np.array_equal(c[1], b[1][:100])


def test_jitter_and_background():
    K, n, steps = 2, 1000, 32
    nz = np.stack([SR.noise(SEED, s, 0, K, n) for s in range(steps)])
    assert nz.dtype == np.float32 and nz.shape == (steps, K, n)
    assert nz.min() >= 0.0 and nz.max() < 1.0
    cnt = nz.size
    z = (float(nz.astype(np.float64).mean()) - 0.5) / math.sqrt(1 / 12 / cnt)
    c2 = _chi2(np.bincount((nz.reshape(-1) * 64).astype(np.int64), minlength=64)
               .astype(np.float64))
    print(f"jitter: z of the mean {z:.2f}, 64-bin chi2 {c2:.1f} at 63 d.o.f.")
    assert abs(z) <= 5 and abs(c2 - 63) <= 5 * math.sqrt(2 * 63)
    # the two sub-NeRFs' rows and two steps differ
    assert not np.array_equal(nz[0, 0], nz[0, 1]) and not np.array_equal(nz[0], nz[1])
    bgs = np.stack([SR.bg(SEED, s) for s in range(steps)])
    assert bgs.shape == (steps, 3) and bgs.min() >= 0 and bgs.max() < 1
    assert len(np.unique(bgs)) == bgs.size
    # the three streams of a key are distinct
    assert SR.bg(SEED, 0)[0] != SR.noise(SEED, 0, 0, 1, 1)[0, 0]


def test_mix_matches_python_ints():
    z = np.array([0, 1, SR.G, SR.MASK, 0x0123456789abcdef], dtype=np.uint64)
    assert [int(v) for v in SR.mix(z)] == [SR.mix_int(int(v)) for v in z]
    assert SR.mix_int(0) == 0 and SR.key(3, 5, 2) != SR.key(3, 5, 1) != SR.key(3, 4, 1)
    # the largest step and rank do not collide with their neighbours' fields
    assert SR.key(0, (1 << 40) - 1, 0) != SR.key(0, 0, 1)


# ---- the schedule -----------------------------------------------------------
def test_cosine_lr_is_cosine_annealing():
    lr0, T = 1e-2, 30
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T, eta_min=lr0 / 30)
    worst = 0.0
    for e in range(T + 1):
        want = opt.param_groups[0]["lr"]
        got = sampler.cosine_lr(lr0, e, T)
        worst = max(worst, abs(got - want) / want)
        opt.step()
        sched.step()
    print(f"cosine_lr vs CosineAnnealingLR over {T + 1} epochs: {worst:.2e} relative")
    assert worst <= 1e-12
    assert sampler.cosine_lr(lr0, 0, T) == lr0
    assert abs(sampler.cosine_lr(lr0, T, T) - lr0 / 30) <= 1e-18
    assert sampler.cosine_lr(lr0, T, T, eta_min=0.0) <= 1e-18
    assert sampler.cosine_lr(lr0, 15, T, eta_min=0.0) == pytest.approx(lr0 / 2, rel=1e-15)
    with pytest.raises(ValueError, match="num_epochs"):
        sampler.cosine_lr(lr0, 0, 0)


# ---- argument checks --------------------------------------------------------
def test_train_images_argument_checks(no_library):
    with pytest.raises(ValueError, match="images must be a tensor"):
        sampler.TrainImages(np.zeros((2, 480, 3), np.uint8))
    with pytest.raises(ValueError, match=r"images must be \(N, H\*W, 3\)"):
        sampler.TrainImages(torch.zeros(2, 24, 20, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"images must be \(N, H\*W, 3\)"):
        sampler.TrainImages(torch.zeros(2, 480, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"images must be \(N, H\*W, 3\)"):
        sampler.TrainImages(torch.zeros(0, 480, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8 or float32"):
        sampler.TrainImages(torch.zeros(2, 480, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="uint8 or float32"):
        sampler.TrainImages(torch.zeros(2, 480, 3, dtype=torch.int16))
    with pytest.raises(ValueError, match="images must be contiguous"):
        sampler.TrainImages(torch.zeros(2, 3, 480, dtype=torch.uint8).transpose(1, 2))
    # host tensors are refused by name, never handed to a kernel
    with pytest.raises(ValueError, match="must be on the GPU"):
        sampler.TrainImages(torch.zeros(2, 480, 3, dtype=torch.uint8))


def _fake_images(n_images, n_pix, dtype=torch.uint8):
    """a TrainImages without a device, for the checks that come after it"""
    ti = sampler.TrainImages.__new__(sampler.TrainImages)
    ti.images = torch.zeros(n_images, n_pix, 3, dtype=dtype)
    ti.n_images, ti.n_pix, ti.dtype_code = n_images, n_pix, 0
    ti.device = ti.images.device
    return ti


def test_sample_batch_argument_checks(no_library):
    ti = _fake_images(2, 480)
    d, poses = torch.rand(480, 3), torch.rand(2, 3, 4)
    with pytest.raises(ValueError, match="must be a TrainImages"):
        sampler.sample_batch(ti.images, d, poses, 16, 2, 0, 0)
    with pytest.raises(ValueError, match="n_rays must be"):
        sampler.sample_batch(ti, d, poses, -1, 2, 0, 0)
    with pytest.raises(ValueError, match="n_rays must be"):
        sampler.sample_batch(ti, d, poses, 16, 0, 0, 0)
    with pytest.raises(ValueError, match=r"step must be in \[0, 2\^40\)"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, -1)
    with pytest.raises(ValueError, match=r"step must be in"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 1 << 40)
    with pytest.raises(ValueError, match=r"rank must be in \[0, 2\^24\)"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0, rank=1 << 24)
    with pytest.raises(ValueError, match=r"directions must be \(480, 3\)"):
        sampler.sample_batch(ti, d[:-1], poses, 16, 2, 0, 0)
    with pytest.raises(ValueError, match="directions must be contiguous float32"):
        sampler.sample_batch(ti, d.double(), poses, 16, 2, 0, 0)
    with pytest.raises(ValueError, match=r"poses must be \(2, 3, 4\)"):
        sampler.sample_batch(ti, d, torch.rand(3, 3, 4), 16, 2, 0, 0)
    with pytest.raises(ValueError, match=r"dR must be \(2, 3\)"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0, dR=torch.zeros(3, 3))
    with pytest.raises(ValueError, match=r"dT must be contiguous float32"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0, dT=torch.zeros(3, 2).t())
    with pytest.raises(ValueError, match=r"mean_dir must be \(3,\)"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0, mean_dir=torch.zeros(1, 3))
    with pytest.raises(ValueError, match="out must be a dict"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0, out={"img_idxs": None})
    out = sampler._buffers(16, 2, False, ti.device)
    with pytest.raises(ValueError, match=r"out\['noise'\] must be"):
        sampler.sample_batch(ti, d, poses, 16, 3, 0, 0, out=out)
    with pytest.raises(ValueError, match=r"out\['img_idxs'\] must be"):
        sampler.sample_batch(ti, d, poses, 17, 2, 0, 0, out=out)
    with pytest.raises(ValueError, match=r"out\['target'\] must be"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0,
                             out=dict(out, target=torch.empty(16, 3).double()))
    with pytest.raises(ValueError, match=r"out\['imgs_d'\] must be"):
        sampler.sample_batch(ti, d, poses, 16, 2, 0, 0, mean_dir=torch.zeros(3), out=out)
    import inspect
    p = inspect.signature(sampler.sample_batch).parameters
    assert list(p) == ["train_images", "directions", "poses", "n_rays", "n_models", "seed",
                       "step", "rank", "dR", "dT", "mean_dir", "out"]
    assert p["rank"].default == 0 and all(p[k].default is None
                                          for k in ("dR", "dT", "mean_dir", "out"))


def test_trainer_images_argument_checks(no_library):
    import inspect
    p = inspect.signature(Trainer.__init__).parameters
    assert p["images"].default is None
    d, poses = torch.rand(480, 3), torch.rand(2, 3, 4)
    u8 = torch.zeros(2, 480, 3, dtype=torch.uint8)
    # raised before the model is looked at
    with pytest.raises(ValueError, match=r"Trainer\(images=...\) needs directions and poses"):
        Trainer(None, None, 64, images=u8)
    with pytest.raises(ValueError, match="uint8 or float32"):
        Trainer(None, None, 64, directions=d, poses=poses, images=u8.double())
    with pytest.raises(ValueError, match="must be on the GPU"):
        Trainer(None, None, 64, directions=d, poses=poses, images=u8)
    with pytest.raises(ValueError, match="images are 3 x 480 pixels for 2 poses and 480 rows"):
        Trainer(None, None, 64, directions=d, poses=poses, images=_fake_images(3, 480))
    with pytest.raises(ValueError, match="images are 2 x 479 pixels for 2 poses and 480 rows"):
        Trainer(None, None, 64, directions=d, poses=poses, images=_fake_images(2, 479))


def test_fit_argument_checks(no_library):
    import inspect
    p = inspect.signature(Trainer.fit).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [
        ("num_epochs", 30), ("steps_per_epoch", 1000), ("val_poses", None),
        ("val_images", None), ("val_every", None), ("eta_min", None), ("callback", None)]
    assert inspect.signature(Trainer.step_sampled).parameters["noise"].default is None
    tr = Trainer.__new__(Trainer)           # the loop's own checks, no device
    tr.images = None
    with pytest.raises(ValueError, match="Trainer.fit needs"):
        tr.fit()
    with pytest.raises(ValueError, match="Trainer.step_sampled needs"):
        tr.step_sampled()
    tr.images, tr.img_wh = _fake_images(2, 480), None
    poses, ims = torch.rand(1, 3, 4), torch.rand(1, 480, 3)
    with pytest.raises(ValueError, match="at least 1"):
        tr.fit(num_epochs=0)
    with pytest.raises(ValueError, match="at least 1"):
        tr.fit(steps_per_epoch=0)
    with pytest.raises(ValueError, match="val_poses and val_images together"):
        tr.fit(val_poses=poses)
    with pytest.raises(ValueError, match="val_poses and val_images together"):
        tr.fit(val_images=ims)
    with pytest.raises(ValueError, match=r"needs Trainer\(img_wh"):
        tr.fit(val_poses=poses, val_images=ims)
    with pytest.raises(ValueError, match="val_every must be at least 1"):
        tr.fit(val_every=0)
    with pytest.raises(ValueError, match="callback must be callable"):
        tr.fit(callback=3)


# ---- the C entry ------------------------------------------------------------
def test_entry_declared_and_bound():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    table = _lib.parse_signature_table(gs.table(hdr))
    name = "rn_sample_batch"
    assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
    assert _lib.binding_signatures()[name] == table[name] == CODES
    # an additive entry: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    assert "sample.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()
    # the header states what the entry stands for and the stream this file's
    # restatement was written from
    for s in ("datasets/base.py:23-31", "train_ml.py:84-96,180", "0xd1b54a32d192ed03",
              "0x8cb92ba72f3d8dd7", "0x9e3779b97f4a7c15"):
        assert s in hdr, s
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "L.rn_sample_batch.argtypes" in doc


def _call(**kw):
    """rn_sample_batch with valid sizes and no pointer, `kw` replacing arguments"""
    a = dict(images=None, image_dtype=0, n_images=5, n_pix=851, directions=None, poses=None,
             dR=None, dT=None, mean_dir=None, seed=1, step=0, rank=0, n_rays=16, n_models=2,
             img_idxs=None, pix_idxs=None, target_rgb=None, rays_o=None, rays_d=None,
             imgs_d=None, noise=None, bg=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.lib().sample_batch(*a.values())


@pytest.mark.parametrize("kw,msg", [
    (dict(step=-1), r"step must be in \[0, 2\^40\)"),
    (dict(step=1 << 40), r"step must be in \[0, 2\^40\)"),
    (dict(rank=-1), r"rank must be in \[0, 2\^24\)"),
    (dict(rank=1 << 24), r"rank must be in \[0, 2\^24\)"),
    (dict(n_images=0), r"n_images and n_pix must be in \[1, 2\^32\)"),
    (dict(n_images=1 << 32), "n_images and n_pix"),
    (dict(n_pix=0), "n_images and n_pix"),
    (dict(n_pix=1 << 32), "n_images and n_pix"),
    (dict(image_dtype=2), "image_dtype must be 0"),
    (dict(image_dtype=-1), "image_dtype must be 0"),
    (dict(n_rays=-1), "bad sizes"),
    (dict(n_models=0), "bad sizes"),
    (dict(), "null pointer"),
    # imgs_d and mean_dir come together (never dereferenced: the check is first)
    (dict(mean_dir=64), "imgs_d and mean_dir must be given together"),
    (dict(imgs_d=64), "imgs_d and mean_dir must be given together"),
    (dict(n_rays=0, imgs_d=64), "imgs_d and mean_dir must be given together"),
])
def test_entry_argument_checks_without_gpu(kw, msg):
    with pytest.raises(RuntimeError, match=r"rn_sample_batch failed \(status 1\).*" + msg):
        _call(**kw)


def test_entry_no_rays_is_a_no_op():
    assert _call(n_rays=0) == 0
    assert _call(n_rays=0, step=(1 << 40) - 1, rank=(1 << 24) - 1, n_images=(1 << 32) - 1,
                 n_pix=(1 << 32) - 1, image_dtype=1) == 0
