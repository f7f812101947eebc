"""GPU: the validation images (csrc/imageout.hip, radnerf_amd.imageout,
ImageEvaluator.images8, Trainer.validate(save_dir=...)).

Every comparison is byte for byte against the numpy restatement of
tests/image_out_ref.py.  Sizes 1, 3, 4, 5, 255, 256, 257, 1025 (a lane's four
pixels, the tail, one block and the next) and 70 001 for the min/max partials,
each also with the base pointers one element on (the unaligned path), strides
1, 2, 5, K in {1, 2, 5, 16}; the values that decide a truncation (every k / 255
and its two fp32 neighbours, 0, -0, 1, 1 - 2^-24, 256/255, 2, -1, NaN, +-inf).
Output buffers carry guard bytes on both sides, which must stay as they were.
"""
import os

import numpy as np
import pytest
import torch

import image_out_ref as IR
from radnerf_amd import imageout
from radnerf_amd._lib import METRICS_WORK_BYTES, lib
from radnerf_amd.evaluate import ImageEvaluator
from radnerf_amd.trainer import Trainer
from test_gpu_evaluate import CHUNK, WH, _setup

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [1, 3, 4, 5, 255, 256, 257, 1025]
GUARD, FILL = 16, 0xAB


def _values():
    k = (np.arange(256, dtype=F) / F(255)).astype(F)
    special = np.array([0, -0.0, 1, 1 - 2.0 ** -24, 256 / 255, 2, -1, np.nan, np.inf, -np.inf],
                       dtype=F)
    return np.concatenate([k, np.nextafter(k, F(-np.inf)), np.nextafter(k, F(np.inf)), special])


VALUES = _values()


def _cycle(n, seed):
    """n of VALUES in a shuffled order (all of them once n reaches their count)"""
    v = VALUES[np.random.default_rng(seed).permutation(VALUES.size)]
    return np.resize(v, n).astype(F)


class Dev:
    """Device arrays whose first element sits `off` elements behind an
    aligned allocation, and guarded output buffers."""

    def __init__(self, cuda):
        self.dev = cuda

    def f32(self, a, off):
        a = np.ascontiguousarray(a, dtype=F)
        buf = torch.zeros(a.size + off + 4, dtype=torch.float32, device=self.dev)
        view = buf[off:off + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return view

    def out(self, shape, off_bytes):
        n = int(np.prod(shape))
        buf = torch.full((GUARD + off_bytes + n + GUARD,), FILL, dtype=torch.uint8,
                         device=self.dev)
        return buf, buf[GUARD + off_bytes:GUARD + off_bytes + n].view(shape)

    @staticmethod
    def guards_intact(buf, view):
        b = buf.cpu().numpy()
        n, lo = view.numel(), view.data_ptr() - buf.data_ptr()
        return bool((b[:lo] == FILL).all() and (b[lo + n:] == FILL).all())


@pytest.fixture(scope="module")
def D(cuda):
    return Dev(cuda)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@pytest.fixture(scope="module")
def work(cuda):
    return torch.empty(METRICS_WORK_BYTES // 8, dtype=torch.float64, device=cuda)


def _minmax(x_view, n, stride, work, cuda):
    out = torch.full((2,), 7.0, device=cuda)
    lib().minmax_finite(x_view.data_ptr(), n, stride, work.data_ptr(), out.data_ptr(),
                        _stream(cuda))
    return out.cpu().numpy()


# ---- rn_quantize_u8 ------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
def test_quantize_values_and_sizes(D, off):
    want_all = IR.quantize_u8(VALUES)
    buf, out = D.out(VALUES.shape, off)
    got = imageout.to_uint8(D.f32(VALUES, off), out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), want_all)
    assert D.guards_intact(buf, out)
    # numpy's own cast where it is defined: [0, 256/255)
    inside = (VALUES >= 0) & (VALUES < F(256) / F(255))
    assert np.array_equal(want_all[inside], (VALUES[inside] * F(255)).astype(np.uint8))
    for n in SIZES:
        for dst_off in (off, 2, 3):
            x = _cycle(n, n)
            buf, out = D.out((n,), dst_off)
            imageout.to_uint8(D.f32(x, off), out=out)
            assert np.array_equal(out.cpu().numpy(), IR.quantize_u8(x)), (n, dst_off)
            assert D.guards_intact(buf, out), (n, dst_off)
    # an image-shaped input keeps its shape; a fresh output is allocated
    x = _cycle(24 * 20 * 3, 5).reshape(20, 24, 3)
    got = imageout.to_uint8(D.f32(x, 0))
    assert got.shape == (20, 24, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), IR.quantize_u8(x))
    assert imageout.to_uint8(torch.empty(0, 3, device=D.dev)).shape == (0, 3)


# ---- rn_minmax_finite -----------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 5])
def test_minmax_finite(D, work, cuda, stride):
    rng = np.random.default_rng(stride)
    for n in SIZES + [70001]:
        for off in (0, 1):
            x = rng.standard_normal(n * stride).astype(F) * F(3)
            x[rng.random(x.size) < 0.1] = np.nan
            x[rng.random(x.size) < 0.05] = np.inf
            x[rng.random(x.size) < 0.05] = -np.inf
            xd = D.f32(x, off)
            want = IR.minmax_finite(x[::stride])
            got = _minmax(xd, n, stride, work, cuda)
            assert got.dtype == F and np.array_equal(got, want), (n, off, got, want)
            # the min and the max each in the last element
            for last in (F(-50), F(50)):
                x[(n - 1) * stride] = last
                got = _minmax(D.f32(x, off), n, stride, work, cuda)
                assert np.array_equal(got, IR.minmax_finite(x[::stride])), (n, off, last)
                assert last in got
    # no finite value, and no value at all: {0, 0}
    none = np.array([np.nan, np.inf, -np.inf] * 100, dtype=F)
    for n in (1, 5, 60):
        assert _minmax(D.f32(none, 0), n, stride, work, cuda).tolist() == [0, 0]
    assert _minmax(D.f32(none, 0), 0, stride, work, cuda).tolist() == [0, 0]
    # the elements between the strided ones are not read as values
    x = np.full(40 * stride, 1e30, dtype=F)
    x[::stride] = np.arange(40, dtype=F)
    if stride > 1:
        assert _minmax(D.f32(x, 0), 40, stride, work, cuda).tolist() == [0, 39]


# ---- rn_colormap_u8 / depth2img ---------------------------------------------------------
@pytest.mark.parametrize("swap", [False, True])
def test_depth2img_values(D, swap):
    """min 0, max 1 (the non-finite values are skipped), so t = x and the
    index thresholds are quantize's"""
    x = VALUES[~(np.isfinite(VALUES) & ((VALUES < 0) | (VALUES > 1)))]
    assert IR.minmax_finite(x).tolist() == [0, 1] and np.isnan(x).any() and np.isinf(x).any()
    want = IR.depth2img(x, imageout.TURBO_LUT, swap)
    for off in (0, 1):
        buf, out = D.out((x.size, 3), 3 * off)
        imageout.depth2img(D.f32(x, off), swap_rb=swap, out=out)
        assert np.array_equal(out.cpu().numpy(), want), off
        assert D.guards_intact(buf, out)
    fin = np.isfinite(x)
    idx = np.clip(x[fin] * F(255), 0, 255).astype(np.uint8)
    lut = imageout.TURBO_LUT[:, ::-1] if swap else imageout.TURBO_LUT
    assert np.array_equal(want[fin], lut[idx]) and np.array_equal(want[~fin], lut[[0] * 3])


@pytest.mark.parametrize("stride", [1, 2, 5])
def test_depth2img_sizes_and_strides(D, stride):
    rng = np.random.default_rng(10 + stride)
    for n in SIZES:
        for off in (0, 1):
            x = (rng.random(n * stride) * 7 + 2).astype(F)
            x[rng.random(x.size) < 0.1] = np.nan
            xs = x[::stride]
            want = IR.depth2img(xs, imageout.TURBO_LUT)
            view = D.f32(x, off)[::stride]
            assert view.stride(0) == stride and view.numel() == n
            for dst_off in (3 * off, 1, 2):
                buf, out = D.out((n, 3), dst_off)
                imageout.depth2img(view, out=out)
                assert np.array_equal(out.cpu().numpy(), want), (n, off, dst_off)
                assert D.guards_intact(buf, out), (n, off, dst_off)
    # a constant image (mx == mn) and one with no finite value: row 0 everywhere
    for x in (np.full(37, 2.5, dtype=F), np.full(37, np.nan, dtype=F)):
        got = imageout.depth2img(D.f32(x, 0)).cpu().numpy()
        assert got.shape == (37, 3) and np.array_equal(got, imageout.TURBO_LUT[[0] * 37])
    # an (H, W) depth gives (H, W, 3)
    x = (rng.random((20, 24)) * 4).astype(F)
    got = imageout.depth2img(D.f32(x, 0))
    assert got.shape == (20, 24, 3)
    assert np.array_equal(got.cpu().numpy(), IR.depth2img(x, imageout.TURBO_LUT))


# ---- rn_gate_map_u8 / gate2img -----------------------------------------------------------
def _gates(n, K, rng):
    """softmax rows, with exact ties, a NaN gate, an all-NaN row and one-hot
    rows among them"""
    z = rng.standard_normal((n, K)).astype(F)
    e = np.exp(z - z.max(1, keepdims=True)).astype(F)
    g = (e / e.sum(1, keepdims=True).astype(F)).astype(F)
    kind = rng.integers(0, 8, n)
    hot = rng.integers(0, K, n)
    g[kind == 0] = F(1) / F(K)                               # every gate ties
    if K > 1:
        t = kind == 1                                        # the last two tie at the top
        g[t, -1] = g[t, -2] = F(0.75)
    g[kind == 2, hot[kind == 2]] = np.nan                    # a NaN gate
    g[kind == 3] = np.nan                                    # nothing but NaN
    one = np.zeros((n, K), dtype=F)
    one[np.arange(n), hot] = 1
    g[kind == 4] = one[kind == 4]
    return g, kind == 4


@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_gate2img(D, K):
    rng = np.random.default_rng(20 + K)
    pal = rng.integers(0, 256, (K, 3), dtype=np.uint8)
    pal_d = torch.from_numpy(pal).to(D.dev)
    for n in SIZES:
        g, onehot = _gates(n, K, rng)
        for off in (0, 1):
            gd = D.f32(g, off)
            res = {}
            for hard in (False, True):
                want = IR.gate_map_u8(g, pal, hard)
                for dst_off in (3 * off, 1, 2):
                    buf, out = D.out((n, 3), dst_off)
                    imageout.gate2img(gd, palette=pal_d, hard=hard, out=out)
                    res[hard] = out.cpu().numpy()
                    assert np.array_equal(res[hard], want), (n, off, hard, dst_off)
                    assert D.guards_intact(buf, out), (n, off, hard, dst_off)
            # on a one-hot row the blend is the palette row, as the hard map
            assert np.array_equal(res[False][onehot], res[True][onehot])
    # the default palette
    g, _ = _gates(257, K, rng)
    got = imageout.gate2img(D.f32(g, 0)).cpu().numpy()
    assert np.array_equal(got, IR.gate_map_u8(g, imageout.default_palette(K)))


# ---- the C ABI's own checks ----------------------------------------------------------------
def test_c_abi_argument_checks(D, work, cuda):
    L, st = lib(), _stream(cuda)
    x = D.f32(np.linspace(0, 1, 64, dtype=F), 0)
    lut = torch.from_numpy(imageout.TURBO_LUT.copy()).to(cuda)
    rng2 = torch.tensor([0.0, 1.0], device=cuda)
    out2 = torch.full((2,), 7.0, device=cuda)
    buf, out = D.out((64, 3), 0)
    p = lambda t: t.data_ptr()
    bad = [
        ("minmax_finite", (p(x), 64, 0, p(work), p(out2), st), "stride"),
        ("minmax_finite", (p(x), 64, -2, p(work), p(out2), st), "stride"),
        ("minmax_finite", (None, 64, 1, p(work), p(out2), st), "null pointer"),
        ("minmax_finite", (p(x), 64, 1, None, p(out2), st), "null pointer"),
        ("minmax_finite", (p(x), 0, 1, p(work), None, st), "null pointer"),
        ("minmax_finite", (p(x), -1, 1, p(work), p(out2), st), "bad sizes"),
        ("quantize_u8", (None, 64, p(out), st), "null pointer"),
        ("quantize_u8", (p(x), 64, None, st), "null pointer"),
        ("quantize_u8", (p(x), -1, p(out), st), "bad sizes"),
        ("colormap_u8", (p(x), 64, 0, p(rng2), p(lut), 0, p(out), st), "stride"),
        ("colormap_u8", (None, 64, 1, p(rng2), p(lut), 0, p(out), st), "null pointer"),
        ("colormap_u8", (p(x), 64, 1, None, p(lut), 0, p(out), st), "null pointer"),
        ("colormap_u8", (p(x), 64, 1, p(rng2), None, 0, p(out), st), "null pointer"),
        ("colormap_u8", (p(x), 64, 1, p(rng2), p(lut), 0, None, st), "null pointer"),
        ("gate_map_u8", (p(x), 3, 17, p(lut), 0, p(out), st), "n_models"),
        ("gate_map_u8", (p(x), 3, 0, p(lut), 0, p(out), st), "n_models"),
        ("gate_map_u8", (None, 4, 16, p(lut), 0, p(out), st), "null pointer"),
        ("gate_map_u8", (p(x), 4, 16, None, 0, p(out), st), "null pointer"),
        ("gate_map_u8", (p(x), 4, 16, p(lut), 1, None, st), "null pointer"),
    ]
    for name, args, msg in bad:
        with pytest.raises(RuntimeError, match=rf"rn_{name} failed \(status 1\).*{msg}"):
            getattr(L, name)(*args)
    torch.cuda.synchronize()
    assert out2.tolist() == [7, 7] and bool((buf == FILL).all())
    # n == 0 is a no-op, null data pointers and all
    L.quantize_u8(None, 0, None, st)
    L.colormap_u8(None, 0, 1, None, None, 0, None, st)
    L.gate_map_u8(None, 0, 1, None, 0, None, st)
    L.minmax_finite(None, 0, 1, None, p(out2), st)
    assert out2.tolist() == [0, 0] and bool((buf == FILL).all())


# ---- ImageEvaluator.images8, Trainer.validate(save_dir=...) ----------------------------------
def _restated(res, K, swap_rb=False, hard=False):
    W, H = WH
    np_ = lambda k: res[k].cpu().numpy()
    want = {"rgb": IR.quantize_u8(np_("rgb")).reshape(H, W, 3),
            "depth": IR.depth2img(np_("depth"), imageout.TURBO_LUT, swap_rb).reshape(H, W, 3)}
    if K > 1:
        want["gate"] = IR.gate_map_u8(np_("gating_code"), imageout.default_palette(K),
                                      hard).reshape(H, W, 3)
    return want


@pytest.mark.parametrize("K,gate_type", [(2, "ray"), (1, None)])
def test_images8(cuda, tmp_path, K, gate_type):
    W, H = WH
    m, g, dirs, poses = _setup(cuda, K, gate_type, 0.5)
    kinds = ["rgb", "depth", "gate"] if K > 1 else ["rgb", "depth"]
    ev = ImageEvaluator(m, g, dirs, WH, chunk=CHUNK)
    assert ev.out8 is None                         # nothing allocated before the first call
    res = ev.render_image(poses[0])
    for swap, hard in ((False, False), (True, True)):
        im8 = ev.images8(swap_rb=swap, hard_gate=hard)
        want = _restated(res, K, swap, hard)
        assert sorted(im8) == sorted(kinds)
        for k in kinds:
            assert im8[k].shape == (H, W, 3) and im8[k].dtype == torch.uint8 and im8[k].is_cuda
            assert np.array_equal(im8[k].cpu().numpy(), want[k]), (k, swap, hard)
    # the pictures are not trivial: rgb has the white background and rays that
    # hit (test_gpu_evaluate.py's scene), depth uses both ends of the table
    plain = _restated(res, K)
    assert int(plain["rgb"].max()) == 255 and len(np.unique(plain["rgb"])) > 2
    flat = plain["depth"].reshape(-1, 3)
    for row in (0, 255):
        assert (flat == imageout.TURBO_LUT[row]).all(1).any()
    assert ev.images8()["rgb"].data_ptr() == im8["rgb"].data_ptr()      # reused buffers
    # through the saver's pinned buffers: a single NGP has no gate map to save
    sv = imageout.ImageSaver(tmp_path)
    for k, v in ev.images8().items():
        sv.save(f"{k}.png", v, k)
    assert os.listdir(tmp_path) == []
    sv.flush()
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.png" for k in kinds)
    for k in kinds:
        assert np.array_equal(IR.read_png(str(tmp_path / f"{k}.png"))[0], plain[k]), k


def test_validate_saves_images(cuda, tmp_path, monkeypatch):
    K, kinds = 2, ["rgb", "depth", "gate"]
    m, g, dirs, poses = _setup(cuda, K, "ray", 0.5)
    tr = Trainer(m, g, 256, directions=dirs, poses=poses, img_wh=WH)
    gt = torch.rand(2, dirs.shape[0], 3, generator=torch.Generator().manual_seed(4)).to(cuda)
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    monkeypatch.chdir(cwd)
    base = tr.validate(poses, gt)
    assert os.listdir(cwd) == [] and tr._evaluator.out8 is None         # no files, no buffers
    out = tmp_path / "val"
    val = tr.validate(poses, gt, save_dir=out, epoch=3)
    tails = {"rgb": "", "depth": "_d", "gate": "_g"}
    names = sorted(f"{i:03d}epoch3{tails[k]}.png" for i in range(2) for k in kinds)
    assert sorted(os.listdir(out)) == names and os.listdir(cwd) == []
    # the numbers are those of a validation that saves nothing, bit for bit
    for k in ("psnr", "ssim"):
        assert torch.equal(val[k], base[k])
        for a, b in zip(val["per_image"], base["per_image"]):
            assert torch.equal(a[k], b[k])
    swapped = tmp_path / "val_bgr"
    tr.validate(poses, gt, save_dir=swapped, epoch=3, swap_rb=True)
    assert sorted(os.listdir(swapped)) == names
    for i in range(2):
        tr._evaluator.render_image(poses[i])
        im8 = {k: v.cpu().numpy() for k, v in tr._evaluator.images8().items()}
        for k in kinds:
            name = f"{i:03d}epoch3{tails[k]}.png"
            got, chunks = IR.read_png(str(out / name))
            assert chunks == [b"IHDR", b"IDAT", b"IEND"]
            assert np.array_equal(got, im8[k]), name
            other = IR.read_png(str(swapped / name))[0]
            assert np.array_equal(other, im8[k][..., ::-1] if k == "depth" else im8[k]), name
    first, second = (IR.read_png(str(out / f"00{i}epoch3.png"))[0] for i in range(2))
    assert not np.array_equal(first, second)                            # two views
