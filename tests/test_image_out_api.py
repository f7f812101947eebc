"""CPU: the surface of the validation images (tests/test_gpu_image_out.py holds
the GPU side).

  * rn_minmax_finite / rn_quantize_u8 / rn_colormap_u8 / rn_gate_map_u8 are
    declared in the header and bound in _lib with the codes csrc/gen_sig.py
    derives from the header; the ABI version stays (the entries are additive);
  * TURBO_LUT is the published table (its sha256 and three rows);
  * write_png round trips through a decoder written here from the PNG
    specification (tests/image_out_ref.py read_png: CRCs, inflate, filter 0),
    and through PIL where it imports;
  * ImageSaver on CPU tensors: the names, nothing written before a buffer
    comes up again, everything there after flush();
  * the argument checks of the Python functions run before the library is
    loaded.
"""
import hashlib
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import image_out_ref as IR
from radnerf_amd import _lib, evaluate, imageout, metrics
from radnerf_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rn_minmax_finite": "pllppp", "rn_quantize_u8": "plpp", "rn_colormap_u8": "pllppipp",
       "rn_gate_map_u8": "plipipp"}


@pytest.fixture
def no_library(monkeypatch):
    """Loading librn.so fails the test: the checks must come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the argument check")
    for mod in (imageout, metrics, evaluate, _lib):
        monkeypatch.setattr(mod, "lib", boom)


def test_entries_declared_and_bound():
    spec = importlib.util.spec_from_file_location(
        "gen_sig", os.path.join(ROOT, "rad-nerf_amd", "csrc", "gen_sig.py"))
    gs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gs)
    hdr = open(os.path.join(ROOT, "include", "radnerf.h")).read()
    table = _lib.parse_signature_table(gs.table(hdr))
    sig = _lib.binding_signatures()
    for name, codes in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert sig[name] == table[name] == codes, name
    assert re.search(r"train_ml\.py:47-52,238-248", hdr)
    # additive entries: the ABI version stays
    assert _lib.ABI_VERSION == 9 and re.search(r"#define\s+RN_ABI_VERSION\s+9\b", hdr)
    assert "imageout.hip" in open(os.path.join(ROOT, "rad-nerf_amd", "csrc", "Makefile")).read()


def test_turbo_lut():
    lut = imageout.TURBO_LUT
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert hashlib.sha256(np.ascontiguousarray(lut).tobytes()).hexdigest() == \
        "c4ae9ddb8a7f13561562fe15fd276fb55ab04e194786c39edfb2ef2cc0929b2b"
    assert tuple(lut[0]) == (48, 18, 59) and tuple(lut[128]) == (164, 252, 60)
    assert tuple(lut[255]) == (122, 4, 3)
    # the default palette: evenly spaced rows, a single model the middle one
    assert np.array_equal(imageout.default_palette(1), lut[[128]])
    assert np.array_equal(imageout.default_palette(2), lut[[0, 255]])
    assert np.array_equal(imageout.default_palette(5), lut[[0, 64, 128, 191, 255]])
    assert imageout.default_palette(16).shape == (16, 3)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="n_models must be 1..16"):
            imageout.default_palette(bad)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (20, 24), (1, 1, 3), (3, 5, 3), (20, 24, 3)])
@pytest.mark.parametrize("level", [0, 6])
def test_write_png_round_trip(tmp_path, shape, level):
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    imageout.write_png(path, a, compress_level=level)
    got, chunks = IR.read_png(path)
    assert chunks == [b"IHDR", b"IDAT", b"IEND"]          # one IDAT chunk
    assert got.shape == a.shape and np.array_equal(got, a)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.mode == ("RGB" if len(shape) == 3 else "L")
        assert np.array_equal(np.asarray(im), a)


def test_write_png_argument_checks(tmp_path):
    p = str(tmp_path / "x.png")
    ok = np.zeros((4, 5, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="uint8 numpy array"):
        imageout.write_png(p, ok.astype(np.float32))
    with pytest.raises(ValueError, match="uint8 numpy array"):
        imageout.write_png(p, torch.zeros(4, 5, dtype=torch.uint8))
    for shape in ((4,), (4, 5, 4), (4, 5, 3, 1), (0, 5), (4, 0, 3)):
        with pytest.raises(ValueError, match=r"\(H, W\) or \(H, W, 3\)"):
            imageout.write_png(p, np.zeros(shape, dtype=np.uint8))
    with pytest.raises(ValueError, match="compress_level"):
        imageout.write_png(p, ok, compress_level=10)
    assert not os.path.exists(p)
    # a non-contiguous view is written as its values
    imageout.write_png(p, np.arange(60, dtype=np.uint8).reshape(5, 4, 3).transpose(1, 0, 2))
    assert np.array_equal(IR.read_png(p)[0],
                          np.arange(60, dtype=np.uint8).reshape(5, 4, 3).transpose(1, 0, 2))


def test_image_saver_on_cpu_tensors(tmp_path):
    d = tmp_path / "val" / "run"                          # created, parents included
    sv = imageout.ImageSaver(d)
    ims = [torch.randint(0, 256, (6, 7, 3), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(i)) for i in range(5)]
    grey = torch.randint(0, 256, (6, 7), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(9))
    files = lambda: sorted(os.listdir(d))
    assert sv.save("000epoch3.png", ims[0], "rgb") == os.path.join(str(d), "000epoch3.png")
    sv.save("000epoch3_d.png", ims[1], "depth")
    sv.save("001epoch3.png", ims[2], "rgb")
    sv.save("001epoch3_d.png", ims[3], "depth")
    assert files() == []                                  # two buffers per kind: none reused yet
    kept = ims[2].clone()
    sv.save("002epoch3.png", ims[4], "rgb")               # rgb's first buffer comes up again
    assert files() == ["000epoch3.png"]
    ims[2].zero_()                                        # the staging copy is the saver's own
    sv.save("g.png", grey, "grey")
    sv.flush()
    assert files() == ["000epoch3.png", "000epoch3_d.png", "001epoch3.png", "001epoch3_d.png",
                       "002epoch3.png", "g.png"]
    want = {"000epoch3.png": ims[0], "000epoch3_d.png": ims[1], "001epoch3.png": kept,
            "001epoch3_d.png": ims[3], "002epoch3.png": ims[4], "g.png": grey}
    for name, t in want.items():
        assert np.array_equal(IR.read_png(str(d / name))[0], t.numpy()), name
    sv.flush()                                            # nothing pending: a no-op
    # a kind may change its shape
    sv.save("h.png", grey[:3].contiguous(), "grey")
    sv.flush()
    assert IR.read_png(str(d / "h.png"))[0].shape == (3, 7)
    with pytest.raises(ValueError, match="uint8 tensor"):
        sv.save("x.png", ims[0].float())
    with pytest.raises(ValueError, match=r"\(H, W\) or \(H, W, 3\)"):
        sv.save("x.png", torch.zeros(4, 5, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        sv.save("x.png", torch.zeros(5, 4, dtype=torch.uint8).t())
    with pytest.raises(ValueError, match="file name"):
        sv.save("../x.png", grey)


def test_map_argument_checks(no_library):
    x = torch.rand(30, 3)
    with pytest.raises(ValueError, match="x must be a tensor"):
        imageout.to_uint8(x.numpy())
    with pytest.raises(ValueError, match="x must be float32"):
        imageout.to_uint8(x.double())
    with pytest.raises(ValueError, match="x must be contiguous"):
        imageout.to_uint8(torch.rand(3, 30).t())
    with pytest.raises(ValueError, match="out must be a uint8 tensor"):
        imageout.to_uint8(x, out=torch.zeros(30, 3))
    with pytest.raises(ValueError, match="out must hold 90 bytes"):
        imageout.to_uint8(x, out=torch.zeros(30, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be contiguous"):
        imageout.to_uint8(x, out=torch.zeros(3, 30, dtype=torch.uint8).t())
    with pytest.raises(ValueError, match="must be on the GPU"):
        imageout.to_uint8(x)

    d = torch.rand(40)
    with pytest.raises(ValueError, match="depth must be a tensor"):
        imageout.depth2img(None)
    with pytest.raises(ValueError, match="depth must be float32"):
        imageout.depth2img(d.half())
    with pytest.raises(ValueError, match="contiguous or a 1-D view"):
        imageout.depth2img(torch.rand(8, 5).t())          # 2-D and strided
    with pytest.raises(ValueError, match="contiguous or a 1-D view"):
        imageout.depth2img(d.expand(3, 40)[:, 0])         # 1-D with stride 0
    with pytest.raises(ValueError, match="out must hold 120 bytes"):
        imageout.depth2img(d, out=torch.zeros(40, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must hold 24 bytes"):
        imageout.depth2img(torch.rand(8, 5)[:, 2], out=torch.zeros(40, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="must be on the GPU"):
        imageout.depth2img(torch.rand(8, 5)[:, 2])        # a column is accepted as it is
    with pytest.raises(ValueError, match="must be on the GPU"):
        imageout.depth2img(torch.rand(4, 10))

    g = torch.rand(12, 4)
    with pytest.raises(ValueError, match="gate must be float32"):
        imageout.gate2img(g.double())
    with pytest.raises(ValueError, match=r"gate must be \(N, K\)"):
        imageout.gate2img(torch.rand(12))
    with pytest.raises(ValueError, match="1 <= K <= 16"):
        imageout.gate2img(torch.rand(12, 17))
    with pytest.raises(ValueError, match="gate must be contiguous"):
        imageout.gate2img(torch.rand(4, 12).t())
    with pytest.raises(ValueError, match="palette must be a uint8 tensor"):
        imageout.gate2img(g, palette=torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"palette must be a contiguous \(4, 3\)"):
        imageout.gate2img(g, palette=torch.zeros(5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must hold 36 bytes"):
        imageout.gate2img(g, out=torch.zeros(12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="must be on the GPU"):
        imageout.gate2img(g, palette=torch.zeros(4, 3, dtype=torch.uint8))


def test_wiring_signatures(no_library, tmp_path):
    p = inspect.signature(evaluate.ImageEvaluator.images8).parameters
    assert p["swap_rb"].default is False and p["hard_gate"].default is False
    v = inspect.signature(Trainer.validate).parameters
    assert v["save_dir"].default is None and v["epoch"].default == 0
    assert v["swap_rb"].default is False
    assert Trainer.val_save_dir is None                 # fit()'s save_dir, off by default
    assert inspect.signature(imageout.depth2img).parameters["swap_rb"].default is False
    assert inspect.signature(imageout.gate2img).parameters["hard"].default is False
    # validate()'s own checks still come first: no directory for a refused call
    tr = Trainer.__new__(Trainer)
    tr.directions, tr.img_wh = torch.rand(480, 3), (24, 20)
    with pytest.raises(ValueError, match=r"poses must be \(N, 3, 4\)"):
        tr.validate(torch.rand(3, 4), torch.rand(2, 480, 3), save_dir=tmp_path / "out")
    assert not (tmp_path / "out").exists()


def test_restatement_is_what_the_header_says():
    """The yardstick of the GPU tests on cases worked by hand."""
    F = np.float32
    q = IR.quantize_u8(np.array([0, -0.0, 1, 1 - 2.0 ** -24, 256 / 255, 2, -1, np.nan, np.inf,
                                 -np.inf, 0.5, 127 / 255], dtype=F))
    # (127 / 255) * 255 rounds to 127 exactly in fp32; 0.5 * 255 = 127.5 truncates
    assert q.tolist() == [0, 0, 255, 254, 255, 255, 0, 0, 255, 0, 127, 127]
    assert IR.minmax_finite(np.array([np.nan, 3, -np.inf, -2, np.inf], dtype=F)).tolist() == [-2, 3]
    assert IR.minmax_finite(np.array([np.nan, np.inf], dtype=F)).tolist() == [0, 0]
    assert IR.minmax_finite(np.zeros(0, dtype=F)).tolist() == [0, 0]
    lut = imageout.TURBO_LUT
    x = np.array([1, 3, 2, np.nan, np.inf], dtype=F)
    img = IR.depth2img(x, lut)
    assert np.array_equal(img, lut[[0, 255, 127, 0, 0]])
    assert np.array_equal(IR.depth2img(x, lut, swap_rb=True), lut[[0, 255, 127, 0, 0]][:, ::-1])
    assert np.array_equal(IR.depth2img(np.full(5, 2.5, dtype=F), lut), lut[[0] * 5])
    pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 100]], dtype=np.uint8)
    g = np.array([[1, 0, 0], [0.5, 0.5, 0], [0.2, 0.2, 0.6], [np.nan, 0.3, 0.3],
                  [np.nan, np.nan, np.nan]], dtype=F)
    hard = IR.gate_map_u8(g, pal, hard=True)
    assert np.array_equal(hard, pal[[0, 0, 2, 1, 0]])     # ties: the first; NaN never wins
    soft = IR.gate_map_u8(g, pal)
    assert soft[0].tolist() == [255, 0, 0] and soft[1].tolist() == [128, 128, 0]
    # a NaN gate times any palette value (0 included) is NaN: the pixel's bytes are 0
    assert soft[2].tolist() == [51, 51, 60] and soft[3].tolist() == [0, 0, 0]
    assert soft[4].tolist() == [0, 0, 0]


def test_fit_passes_save_dir_and_epoch(monkeypatch, tmp_path):
    """fit() hands Trainer.val_save_dir and its epoch to every validation"""
    tr = Trainer.__new__(Trainer)
    tr.images, tr.img_wh, tr.lr0, tr.device = object(), (24, 20), 1e-2, torch.device("cpu")
    tr.opt = type("Opt", (), {"param_groups": [{"lr": 0.0}]})()
    calls = []
    monkeypatch.setattr(Trainer, "step_sampled",
                        lambda self: {"rgb": torch.tensor(0.25, dtype=torch.float64)})
    monkeypatch.setattr(Trainer, "validate", lambda self, poses, images, **kw:
                        calls.append(kw) or {"psnr": torch.tensor(20.0), "ssim": torch.tensor(0.5)})
    poses, ims = torch.rand(2, 3, 4), torch.rand(2, 480, 3)
    tr.fit(num_epochs=3, steps_per_epoch=1, val_poses=poses, val_images=ims, val_every=2)
    assert calls == [{"save_dir": None, "epoch": 1}, {"save_dir": None, "epoch": 2}]
    del calls[:]
    tr.val_save_dir = tmp_path
    log = tr.fit(num_epochs=2, steps_per_epoch=2, val_poses=poses, val_images=ims, val_every=1)
    assert calls == [{"save_dir": tmp_path, "epoch": 0}, {"save_dir": tmp_path, "epoch": 1}]
    assert [e["val"] for e in log] == [{"psnr": 20.0, "ssim": 0.5}] * 2
