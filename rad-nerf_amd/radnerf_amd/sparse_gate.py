"""Gate-sparse test-time render: which (ray, sub-NeRF) pairs the gate keeps.

The reference weights every sub-NeRF's render by the softmax gate
(ml_rendering.py:33-36,65-68) and leaves Ray_Gate.forward's third return
value, top_k_indices, at None (networks.py:1087-1093).  Here a pair is live
iff its gate is at least `gate_min` and it is among the row's `gate_topk`
largest gates (rank by gate descending, index ascending); the first maximal
gate of a row is always live.  include/radnerf.h (rn_gate_select) states the
semantics in full; tests/gate_select_ref.py restates them in numpy.

    sel = select(gate, gate_min=1e-3)       # gate (n, K) fp32 on the GPU
    sel["live"]        (n, K) uint8
    sel["gate_used"]   (n, K) fp32: the gate where live, 0 elsewhere
                       (renormalize=True: divided by the row's live sum)
    sel["list"]        (K, n) int32: row i starts with the rays live for i,
                       ascending; the rest of the row is left as it was
    sel["count"]       (K,) int32

ImageEvaluator.render_image(gate_min=..., gate_topk=..., renormalize=...)
(evaluate.py) is the user of this; rendering.ml_render(test_time=True) and the
pinned layout stay dense.  Nothing here synchronises with the host.
"""
import numbers

import torch

from ._lib import GATE_SELECT_WORK_BYTES, lib

MAX_MODELS = 16


def check_params(fn, K, gate_min, gate_topk):
    """(gate_min as float, gate_topk as int with None -> K); ValueError naming
    the argument and its value otherwise.  Touches no library."""
    if isinstance(gate_min, bool) or not isinstance(gate_min, numbers.Real) \
            or not 0.0 <= float(gate_min) < 1.0:
        raise ValueError(f"{fn}: gate_min must be a number in [0, 1), got {gate_min!r}")
    if gate_topk is None:
        gate_topk = K
    if isinstance(gate_topk, bool) or not isinstance(gate_topk, numbers.Integral) or not 1 <= gate_topk <= K:
        raise ValueError(f"{fn}: gate_topk must be None or an int in [1, {K}] "
                         f"({K} sub-NeRFs), got {gate_topk!r}")
    return float(gate_min), int(gate_topk)


def is_dense(K, gate_min, gate_topk):
    """Checked parameters that keep every pair: the dense render's case."""
    return K == 1 or (gate_min == 0.0 and gate_topk == K)


def _check_gate_shape(fn, gate):
    if not torch.is_tensor(gate) or gate.ndim != 2:
        raise ValueError(f"{fn}: gate must be a (n, K) tensor, got "
                         f"{tuple(getattr(gate, 'shape', ())) or type(gate).__name__}")
    if not 1 <= gate.shape[1] <= MAX_MODELS:
        raise ValueError(f"{fn}: gate has {gate.shape[1]} columns, 1 to {MAX_MODELS} sub-NeRFs "
                         f"are supported")


def _check_gate_storage(fn, gate):
    if gate.dtype != torch.float32:
        raise ValueError(f"{fn}: gate must be float32, got {gate.dtype}")
    if not gate.is_contiguous():
        raise ValueError(f"{fn}: gate must be contiguous")
    if gate.device.type != "cuda":
        raise ValueError(f"{fn}: gate must be on the GPU, got a {gate.device.type} tensor")


_OUT = {"live": torch.uint8, "gate_used": torch.float32, "list": torch.int32,
        "count": torch.int32}


def select(gate, gate_min=0.0, gate_topk=None, renormalize=False, out=None):
    """rn_gate_select on gate (n, K): {"live", "gate_used", "list", "count"}
    (module docstring).  out: a dict of those four to write into (shapes (n, K),
    (n, K), (K, n), (K,)), for a caller that renders many chunks; a "work" entry
    (GATE_SELECT_WORK_BYTES of uint8) is used as the scratch if present."""
    fn = "sparse_gate.select"
    _check_gate_shape(fn, gate)
    n, K = gate.shape
    tau, k = check_params(fn, K, gate_min, gate_topk)
    _check_gate_storage(fn, gate)
    shapes = {"live": (n, K), "gate_used": (n, K), "list": (K, n), "count": (K,)}
    if out is not None:
        for name, dt in _OUT.items():
            t = out.get(name) if isinstance(out, dict) else None
            if not torch.is_tensor(t) or tuple(t.shape) != shapes[name] or t.dtype != dt \
                    or not t.is_contiguous() or t.device != gate.device:
                raise ValueError(f"{fn}: out[{name!r}] must be a contiguous {dt} tensor of shape "
                                 f"{shapes[name]} on {gate.device}")
    L = lib()
    dev = gate.device
    if out is None:
        out = {name: torch.empty(shapes[name], dtype=dt, device=dev) for name, dt in _OUT.items()}
    work = out.get("work")
    if work is None:
        work = torch.empty(GATE_SELECT_WORK_BYTES, dtype=torch.uint8, device=dev)
    elif work.numel() * work.element_size() < GATE_SELECT_WORK_BYTES or work.device != dev:
        raise ValueError(f"{fn}: out['work'] must hold {GATE_SELECT_WORK_BYTES} bytes on {dev}")
    L.gate_select(gate.data_ptr(), n, K, tau, k, int(bool(renormalize)), out["live"].data_ptr(),
                  out["gate_used"].data_ptr(), out["list"].data_ptr(), out["count"].data_ptr(),
                  None, None, None, None, work.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
    return {name: out[name] for name in _OUT}
