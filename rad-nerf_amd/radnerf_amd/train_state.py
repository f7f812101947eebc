"""The whole training state of radnerf_amd.trainer.Trainer, in memory and in a
file (DESIGN.md §4 "Checkpoint and resume"): what train_ml.py gets from
Lightning's `--ckpt_path` ("including optimizers, etc") and its
ModelCheckpoint, held to the bar Trainer(deterministic=True) allows -- a run
continued from a state equals the uninterrupted one bit for bit.

A state is a nested dict of CPU tensors and plain int / float / str / bool /
list / dict values, and nothing else:

  header      format, version, and per tensor its byte size and zlib.crc32
  structure   what must match the trainer exactly (sizes, world size)
  hyper       what must match unless the caller overrides it
  model       parameters (fp32), the box, the occupancy grids and bitfields,
              the count_grid when the model has one
  poses       dR / dT under optimize_ext
  optimizer   per parameter step / exp_avg / exp_avg_sq, per group the lr
  progress    global_step and, inside fit, the epoch position and the log
  generators  torch's CPU generator and the device's

The file is torch.save's and is read only with torch.load(...,
weights_only=True): the loader executes nothing from the file
(checkpoint.py's rule).  Writing is atomic (a temporary name in the same
directory, then os.replace); reading checks the version and every tensor's
size and checksum before anything is handed on, and raises ValueError naming
the file (and the tensor) otherwise.

BackgroundSaver is the save that does not stop the run: a staging copy on the
training stream, a copy to reused pinned host buffers on a side stream, and
one writer thread for the checksums and the file.
"""
import os
import re
import threading
import zlib

import torch

FORMAT = "radnerf_amd.train_state"
VERSION = 1
NAME = re.compile(r"^state_epoch(\d{4,})\.pt$")
PLAIN = (bool, int, float, str)


def checkpoint_name(epoch):
    """fit's file after `epoch` finished epochs"""
    return f"state_epoch{int(epoch):04d}.pt"


def _tmp_name(path):
    d, b = os.path.split(os.path.abspath(path))
    return os.path.join(d, f".{b}.tmp{os.getpid()}")


# ---- walking a state ----------------------------------------------------------
def tensors(state, _prefix=""):
    """(path, tensor) of every tensor of a state, paths joined by '/'"""
    items = state.items() if isinstance(state, dict) else enumerate(state)
    for k, v in items:
        path = f"{_prefix}{k}"
        if torch.is_tensor(v):
            yield path, v
        elif isinstance(v, (dict, list)):
            yield from tensors(v, path + "/")


def check_plain(state, _path="state"):
    """ValueError unless `state` holds CPU tensors and plain values alone"""
    if torch.is_tensor(state):
        if state.device.type != "cpu":
            raise ValueError(f"train state: {_path} is a tensor on {state.device}")
    elif isinstance(state, dict):
        for k, v in state.items():
            if not isinstance(k, str):
                raise ValueError(f"train state: {_path} has the key {k!r}, not a str")
            check_plain(v, f"{_path}/{k}")
    elif isinstance(state, list):
        for i, v in enumerate(state):
            check_plain(v, f"{_path}/{i}")
    elif not isinstance(state, PLAIN):
        raise ValueError(f"train state: {_path} is a {type(state).__name__}")


def _crc(t):
    t = t.detach().contiguous().reshape(-1)
    if t.numel() == 0:
        return 0, 0
    raw = t.view(torch.uint8).numpy()
    return raw.nbytes, zlib.crc32(raw) & 0xFFFFFFFF


def seal(state):
    """Write the header: the version and every tensor's size and checksum."""
    state.pop("header", None)
    table = {}
    for path, t in tensors(state):
        n, c = _crc(t)
        table[path] = {"bytes": n, "crc32": c}
    state["header"] = {"format": FORMAT, "version": VERSION, "tensors": table}
    return state


def verify(state, where="the state"):
    """The integrity check: format and version, then every tensor against the
    header's size and checksum.  ValueError naming `where` (and the tensor)."""
    head = state.get("header") if isinstance(state, dict) else None
    if not isinstance(head, dict) or head.get("format") != FORMAT:
        raise ValueError(f"{where}: not a radnerf_amd training state (no header)")
    if head.get("version") != VERSION:
        raise ValueError(f"{where}: format version {head.get('version')!r}, this build reads "
                         f"version {VERSION}")
    table = head.get("tensors")
    if not isinstance(table, dict):
        raise ValueError(f"{where}: the header has no checksum table")
    body = {k: v for k, v in state.items() if k != "header"}
    found = dict(tensors(body))
    if set(found) != set(table):
        odd = sorted(set(found) ^ set(table))
        raise ValueError(f"{where}: tensors and checksum table differ: {', '.join(odd[:8])}")
    for path, t in found.items():
        n, c = _crc(t)
        want = table[path]
        if n != want.get("bytes"):
            raise ValueError(f"{where}: tensor {path} has {n} bytes, the header says "
                             f"{want.get('bytes')}")
        if c != want.get("crc32"):
            raise ValueError(f"{where}: tensor {path} fails its checksum (crc32 {c:#010x}, the "
                             f"header says {want.get('crc32'):#010x})")
    check_plain(state)
    return state


# ---- the file -----------------------------------------------------------------
def atomic_save(obj, path):
    """torch.save under a temporary name of the same directory, then
    os.replace: a failed write leaves an earlier file as it was."""
    path = os.path.abspath(path)
    tmp = _tmp_name(path)
    try:
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return path


def write_file(state, path):
    """A sealed state into a file, atomically (atomic_save)."""
    if "header" not in state:
        seal(state)
    return atomic_save(state, path)


def read_file(path):
    """The verified state of a file.  Whatever the reader raises (a truncated
    or foreign file, a pickle weights_only refuses) is wrapped in a ValueError
    naming the file."""
    try:
        state = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise ValueError(f"{path}: cannot be read as a training state "
                         f"({type(e).__name__}: {str(e)[:300]})") from e
    return verify(state, str(path))


def list_checkpoints(ckpt_dir):
    """[(epoch, path)] of fit's files in `ckpt_dir`, oldest first; temporary
    names and everything else are ignored."""
    out = []
    if ckpt_dir is not None and os.path.isdir(ckpt_dir):
        for name in os.listdir(ckpt_dir):
            m = NAME.match(name)
            if m:
                out.append((int(m.group(1)), os.path.join(ckpt_dir, name)))
    return sorted(out)


def newest_checkpoint(ckpt_dir):
    """(path, state) of the newest file of `ckpt_dir` that reads and verifies,
    or None.  (Writes are atomic, so a file with a checkpoint's name is whole
    unless the disk damaged it; then the one before it is taken.)"""
    for _, path in reversed(list_checkpoints(ckpt_dir)):
        try:
            return path, read_file(path)
        except ValueError:
            continue
    return None


def prune(ckpt_dir, keep):
    """Remove all but the newest `keep` of fit's files."""
    files = list_checkpoints(ckpt_dir)
    for _, path in files[:max(0, len(files) - int(keep))]:
        try:
            os.unlink(path)
        except OSError:
            pass


# ---- the two compatibility checks ---------------------------------------------
def differences(saved, own):
    """[(field, saved value, own value)] over the union of two flat dicts"""
    missing = "(absent)"
    return [(k, saved.get(k, missing), own.get(k, missing))
            for k in sorted(set(saved) | set(own)) if saved.get(k, missing) != own.get(k, missing)]


def _listing(diff):
    return "; ".join(f"{k}: saved {a!r}, this trainer {b!r}" for k, a, b in diff)


def check_compatible(state, structure, hyper, override=False, where="the state"):
    """Structure must match; the hyper-parameters must match unless
    `override` (the trainer's own values then stand).  ValueError listing each
    differing field with both values."""
    diff = differences(state.get("structure", {}), structure)
    if diff:
        raise ValueError(f"{where}: the structure differs from this trainer's -- "
                         + _listing(diff))
    diff = differences(state.get("hyper", {}), hyper)
    if diff and not override:
        raise ValueError(f"{where}: the hyper-parameters differ from this trainer's "
                         f"(override=True keeps this trainer's) -- " + _listing(diff))


# ---- the background save --------------------------------------------------------
class SaveHandle:
    """One background save: wait() returns the path once the file is in place,
    or raises what the writer raised."""

    def __init__(self, path):
        self.path, self.error, self._thread = path, None, None

    def done(self):
        return self._thread is None or not self._thread.is_alive()

    def wait(self):
        if self._thread is not None:
            self._thread.join()
        if self.error is not None:
            err, self.error = self.error, None
            raise err
        return self.path


class BackgroundSaver:
    """Snapshot on the training stream, device-to-host on a side stream into
    pinned buffers kept for the next save, the file from one writer thread (a
    thread of this process: the GPU stays open in it).  One save is in flight
    at a time: the next one waits for it before it reuses the buffers."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self._stage, self._host, self._side, self.pending = {}, {}, None, None

    def wait(self):
        """Join the writer; raises what it raised."""
        h, self.pending = self.pending, None
        if h is not None:
            h.wait()

    def _buffer(self, pool, key, like, **kw):
        b = pool.get(key)
        if b is None or b.shape != like.shape or b.dtype != like.dtype:
            b = pool[key] = torch.empty(like.shape, dtype=like.dtype, **kw)
        return b

    def fetch(self, key, t):
        """The host tensor `t`'s values at this point of the training stream
        will be in, once the side stream's copy has run (save() waits for it)."""
        t = t.detach()
        if not self.cuda:
            return t.to("cpu", copy=True)
        stage = self._buffer(self._stage, key, t, device=self.device)
        stage.copy_(t)                                  # on the training stream
        self._copies.append((stage, self._buffer(self._host, key, t, pin_memory=True)))
        return self._copies[-1][1]

    def save(self, build, path, after=None):
        """build(fetch) -> the state, its device tensors passed through
        `fetch`; `after()` runs in the writer once the file is in place."""
        self.wait()                                     # a second save waits for the first
        self._copies = []
        state = build(self.fetch)
        event = None
        if self.cuda and self._copies:
            if self._side is None:
                self._side = torch.cuda.Stream(self.device)
            self._side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self._side):
                for stage, host in self._copies:
                    host.copy_(stage, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self._side)
        self._copies = []
        handle = SaveHandle(os.path.abspath(path))

        def work():
            try:
                if event is not None:
                    event.synchronize()
                write_file(seal(state), handle.path)
                if after is not None:
                    after()
            except BaseException as e:              # handed to wait()
                handle.error = e

        # not a daemon: interpreter exit waits for a pending write
        handle._thread = threading.Thread(target=work, name="radnerf-save", daemon=False)
        handle._thread.start()
        self.pending = handle
        return handle
