"""The pictures of validation_step (train_ml.py:47-52,238-248) from the
device: 8-bit rgb, the depth through depth2img (min-max normalise, Turbo), a
picture of the gating code, and PNG files -- with no cv2, imageio or matplotlib.

    to_uint8(x)                          -> uint8, (x * 255).astype(np.uint8)
    depth2img(depth, swap_rb=False)      -> (..., 3) uint8
    gate2img(gate, palette=None, hard=False) -> (N, 3) uint8
    write_png(path, array, compress_level=6)
    ImageSaver(directory).save(name, u8_tensor, kind) / .flush()

The three maps are device tensors in, device tensors out, on the current
stream with no host synchronisation (csrc/imageout.hip: rn_quantize_u8,
rn_minmax_finite + rn_colormap_u8 back to back, rn_gate_map_u8).  Argument
errors raise ValueError naming the argument before the library is touched.
The reference hands cv2's BGR colormap to imageio as it is, so its depth files
carry Turbo with red and blue exchanged: swap_rb=True reproduces those files,
the default is Turbo as published.
"""
import os
import struct
import zlib

import numpy as np
import torch

from . import metrics
from ._lib import lib

MAX_MODELS = 16          # rn_gate_map_u8's bound (rn_gate_fwd's)

# rint(255 t) of the Turbo colormap's 256 published entries (A. Mikhailov,
# Google, Apache-2.0), C order; what cv2.COLORMAP_TURBO holds after
# convertTo(CV_8U, 255).  No entry is within 0.0014 of a rounding tie.
TURBO_LUT = np.frombuffer(bytes.fromhex(
    "30123b32154333184a341b51351e5836215f37246638276d392a733a2d793b2f803c32863d358b3e38913f3b973f3e9c"
    "4040a24143a74146ac4249b1424bb5434eba4451bf4454c34456c74559cb455ccf455ed34661d64664da4666dd4669e0"
    "466be3476ee64771e94773eb4776ee4778f0477bf2467df44680f64682f84685fa4687fb458afc458cfd448ffe4391fe"
    "4294ff4196ff4099ff3e9bfe3d9efe3ba0fd3aa3fc38a5fb37a8fa35abf833adf731aff52fb2f42eb4f22cb7f02ab9ee"
    "28bceb27bee925c0e723c3e422c5e220c7df1fc9dd1ecbda1ccdd81bd0d51ad2d21ad4d019d5cd18d7ca18d9c818dbc5"
    "18ddc218dec018e0bd19e2bb19e3b91ae4b61ce6b41de7b21fe9af20eaac22ebaa25eca727eea42aefa12cf09e2ff19b"
    "32f29835f39438f4913cf58e3ff68a43f78746f8844af8804ef97d52fa7a55fa7659fb735dfc6f61fc6c65fd6969fd66"
    "6dfe6271fe5f75fe5c79fe597dff5680ff5384ff5188ff4e8bff4b8fff4992ff4796fe4499fe429cfe409ffd3fa1fd3d"
    "a4fc3ca7fc3aa9fb39acfb38affa37b1f936b4f836b7f735b9f635bcf534bef434c1f334c3f134c6f034c8ef34cbed34"
    "cdec34d0ea34d2e935d4e735d7e535d9e436dbe236dde037dfdf37e1dd37e3db38e5d938e7d739e9d539ebd339ecd13a"
    "eecf3aefcd3af1cb3af2c93af4c73af5c53af6c33af7c13af8be39f9bc39faba39fbb838fbb637fcb336fcb136fdae35"
    "fdac34fea933fea732fea431fea130fe9e2ffe9b2dfe992cfe962bfe932afe9029fd8d27fd8a26fc8725fc8423fb8122"
    "fb7e21fa7b1ff9781ef9751df8721cf76f1af66c19f56918f46617f36315f26014f15d13f05b12ef5811ed5510ec530f"
    "eb500eea4e0de84b0ce7490ce5470be4450ae2430ae14109df3f08dd3d08dc3b07da3907d83706d63506d43305d23105"
    "d02f05ce2d04cc2b04ca2a04c82803c52603c32503c12302be2102bc2002b91e02b71d02b41b01b21a01af1801ac1701"
    "a91601a71401a41301a112019e10019b0f01980e01950d01920b018e0a018b09028808028507028106027e05027a0403"
), dtype=np.uint8).reshape(256, 3)


def default_palette(n_models):
    """(K, 3) uint8: sub-NeRF k gets TURBO_LUT[round(255 k / (K - 1))], a
    single one row 128."""
    K = int(n_models)
    if not 1 <= K <= MAX_MODELS:
        raise ValueError(f"default_palette: n_models must be 1..{MAX_MODELS}, got {n_models}")
    rows = [128] if K == 1 else [round(255 * k / (K - 1)) for k in range(K)]
    return TURBO_LUT[rows].copy()


# ---- device maps -----------------------------------------------------------------
_consts = {}


def _const(dev, key, make):
    """Per-device constants and scratch (the table, the default palettes, the
    {min, max} pair); calls on one device are ordered by its current stream."""
    t = _consts.get((dev, key))
    if t is None:
        t = _consts[(dev, key)] = make().to(dev)
    return t


def _check_f32(fn, name, t):
    if not torch.is_tensor(t):
        raise ValueError(f"{fn}: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{fn}: {name} must be float32, got {t.dtype}")


def _check_out(fn, out, shape, src):
    if out is None:
        return
    n = 1
    for v in shape:
        n *= v
    if not torch.is_tensor(out) or out.dtype != torch.uint8:
        raise ValueError(f"{fn}: out must be a uint8 tensor")
    if out.numel() != n:
        raise ValueError(f"{fn}: out must hold {n} bytes {tuple(shape)}, got "
                         f"{tuple(out.shape)}")
    if not out.is_contiguous():
        raise ValueError(f"{fn}: out must be contiguous")
    if out.device != src.device:
        raise ValueError(f"{fn}: out is on {out.device}, the input on {src.device}")


def _check_device(fn, t):
    # last of the checks: the kernels take device pointers only
    if not t.is_cuda:
        raise ValueError(f"{fn}: the input must be on the GPU, got {t.device}")


def _new(out, shape, dev):
    return torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else out


def to_uint8(x, out=None):
    """(x * 255).astype(np.uint8) of a contiguous fp32 tensor of any shape,
    with NaN -> 0 and values clamped to [0, 255] where numpy's cast is
    undefined (rn_quantize_u8)."""
    _check_f32("to_uint8", "x", x)
    if not x.is_contiguous():
        raise ValueError("to_uint8: x must be contiguous")
    _check_out("to_uint8", out, x.shape, x)
    _check_device("to_uint8", x)
    out = _new(out, x.shape, x.device)
    lib().quantize_u8(x.data_ptr(), x.numel(), out.data_ptr(), metrics._stream(x.device))
    return out


def depth2img(depth, swap_rb=False, out=None):
    """depth2img (train_ml.py:47-52): (depth - min) / (max - min) through the
    Turbo table, min and max over the finite values; a constant or non-finite
    depth gets row 0.  depth: fp32, contiguous of any shape, or a 1-D view with
    any element stride >= 1 (a column of depth_k).  Returns depth.shape + (3,)
    uint8; swap_rb exchanges red and blue as the reference's files have them."""
    fn = "depth2img"
    _check_f32(fn, "depth", depth)
    if depth.is_contiguous():
        stride = 1
    elif depth.ndim == 1 and depth.stride(0) >= 1:
        stride = depth.stride(0)
    else:
        raise ValueError(f"{fn}: depth must be contiguous or a 1-D view with a positive "
                         f"stride, got shape {tuple(depth.shape)} strides {depth.stride()}")
    shape = tuple(depth.shape) + (3,)
    _check_out(fn, out, shape, depth)
    _check_device(fn, depth)
    dev, n = depth.device, depth.numel()
    out = _new(out, shape, dev)
    lut = _const(dev, "turbo", lambda: torch.from_numpy(TURBO_LUT.copy()))
    rng = _const(dev, "range", lambda: torch.zeros(2, dtype=torch.float32))
    L, st = lib(), metrics._stream(dev)
    L.minmax_finite(depth.data_ptr(), n, stride, metrics._work(dev).data_ptr(), rng.data_ptr(), st)
    L.colormap_u8(depth.data_ptr(), n, stride, rng.data_ptr(), lut.data_ptr(), int(bool(swap_rb)),
                  out.data_ptr(), st)
    return out


def gate2img(gate, palette=None, hard=False, out=None):
    """A picture of the gating code: gate (N, K) fp32, K <= 16, palette (K, 3)
    uint8 on gate's device (None: default_palette(K)).  hard=False blends the
    palette rows with the gate values (k ascending, + 0.5, truncated);
    hard=True takes the row of the first maximal gate.  Returns (N, 3) uint8."""
    fn = "gate2img"
    _check_f32(fn, "gate", gate)
    if gate.ndim != 2 or not 1 <= gate.shape[1] <= MAX_MODELS:
        raise ValueError(f"{fn}: gate must be (N, K) with 1 <= K <= {MAX_MODELS}, got "
                         f"{tuple(gate.shape)}")
    if not gate.is_contiguous():
        raise ValueError(f"{fn}: gate must be contiguous")
    N, K = gate.shape
    if palette is not None:
        if not torch.is_tensor(palette) or palette.dtype != torch.uint8:
            raise ValueError(f"{fn}: palette must be a uint8 tensor")
        if tuple(palette.shape) != (K, 3) or not palette.is_contiguous():
            raise ValueError(f"{fn}: palette must be a contiguous ({K}, 3) tensor, got "
                             f"{tuple(palette.shape)}")
        if palette.device != gate.device:
            raise ValueError(f"{fn}: palette is on {palette.device}, gate on {gate.device}")
    _check_out(fn, out, (N, 3), gate)
    _check_device(fn, gate)
    dev = gate.device
    out = _new(out, (N, 3), dev)
    if palette is None:
        palette = _const(dev, ("palette", K), lambda: torch.from_numpy(default_palette(K)))
    lib().gate_map_u8(gate.data_ptr(), N, K, palette.data_ptr(), int(bool(hard)), out.data_ptr(),
                      metrics._stream(dev))
    return out


# ---- PNG ---------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def write_png(path, array, compress_level=6):
    """An 8-bit (H, W) grey or (H, W, 3) RGB numpy array as a PNG file: filter
    type 0 on every row, one IDAT chunk, the standard library's zlib."""
    a = array
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
        raise ValueError("write_png: array must be a uint8 numpy array, got "
                         f"{getattr(a, 'dtype', type(a).__name__)}")
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 \
            or a.shape[1] < 1:
        raise ValueError(f"write_png: array must be (H, W) or (H, W, 3), got {a.shape}")
    level = int(compress_level)
    if not -1 <= level <= 9:
        raise ValueError(f"write_png: compress_level must be -1..9, got {compress_level}")
    H, W = a.shape[:2]
    rows = np.empty((H, 1 + a.size // H), dtype=np.uint8)
    rows[:, 0] = 0                                      # filter type 0: the bytes as they are
    rows[:, 1:] = a.reshape(H, -1)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr)
                + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))


class _Slot:
    __slots__ = ("buf", "pinned", "event", "path", "seq")

    def __init__(self):
        self.buf = self.event = self.path = None
        self.pinned, self.seq = False, 0


class ImageSaver:
    """Writes device images as PNG files under `directory` without stalling
    the stream.  Each map kind has two staging buffers (pinned for a GPU
    source, plain for a CPU one): save() enqueues a non-blocking copy into the
    kind's next buffer and records an event; the file of a buffer is encoded
    and written when that buffer comes up again, or at flush(), so the encode
    of one image overlaps the render of the next.  No threads."""

    def __init__(self, directory, compress_level=6):
        self.directory = os.fspath(directory)
        os.makedirs(self.directory, exist_ok=True)
        self.compress_level = int(compress_level)
        self._slots, self._next, self._seq = {}, {}, 0

    def save(self, name, image, kind="image"):
        """image: a contiguous uint8 (H, W) or (H, W, 3) tensor; the file
        directory/name exists after the kind's second next save(), or
        flush().  Returns the path."""
        if not torch.is_tensor(image) or image.dtype != torch.uint8:
            raise ValueError("ImageSaver.save: image must be a uint8 tensor")
        if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3) \
                or image.numel() == 0:
            raise ValueError(f"ImageSaver.save: image must be (H, W) or (H, W, 3), got "
                             f"{tuple(image.shape)}")
        if not image.is_contiguous():
            raise ValueError("ImageSaver.save: image must be contiguous")
        if not name or os.path.basename(name) != name:
            raise ValueError(f"ImageSaver.save: name must be a file name, got {name!r}")
        slots = self._slots.setdefault(kind, (_Slot(), _Slot()))
        i = self._next.get(kind, 0)
        self._next[kind] = i ^ 1
        slot = slots[i]
        self._write(slot)
        pin = image.is_cuda
        if slot.buf is None or slot.buf.shape != image.shape or slot.pinned != pin:
            slot.buf, slot.pinned = torch.empty(image.shape, dtype=torch.uint8, pin_memory=pin), pin
        slot.buf.copy_(image, non_blocking=True)
        if image.is_cuda:
            slot.event = torch.cuda.Event()
            slot.event.record(torch.cuda.current_stream(image.device))
        slot.path = os.path.join(self.directory, name)
        self._seq += 1
        slot.seq = self._seq
        return slot.path

    def _write(self, slot):
        if slot.path is None:
            return
        if slot.event is not None:
            slot.event.synchronize()
            slot.event = None
        write_png(slot.path, slot.buf.numpy(), self.compress_level)
        slot.path = None

    def flush(self):
        """Write every pending file, in the order of the save() calls."""
        pending = [s for pair in self._slots.values() for s in pair if s.path is not None]
        for slot in sorted(pending, key=lambda s: s.seq):
            self._write(slot)
