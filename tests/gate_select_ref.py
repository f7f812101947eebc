"""The gate-sparse selection restated in numpy fp32 (include/radnerf.h,
rn_gate_select): what the GPU tests compare the kernel with bit for bit, and
the crafted gates they share.

Pair (r, i) is live iff gate[r,i] >= gate_min and fewer than gate_topk indices j
have gate[r,j] > gate[r,i], or gate[r,j] == gate[r,i] with j < i.  The first
maximal gate of a row (rank 0) is live whatever gate_min is.  gate_used is the
gate where live and 0.0 elsewhere; with renormalize it is gate / S, S the fp32
sum of the row's live gates in index order, the division correctly rounded
(numpy's fp32 division is).  list[i] holds the rays live for sub-NeRF i in
ascending order, count[i] how many.
"""
import numpy as np


def select_ref(gate, gate_min=0.0, gate_topk=None, renormalize=False):
    g = np.ascontiguousarray(gate, dtype=np.float32)
    n, K = g.shape
    k = K if gate_topk is None else int(gate_topk)
    assert 0.0 <= gate_min < 1.0 and 1 <= k <= K
    tau = np.float32(gate_min)
    gi, gj = g[:, :, None], g[:, None, :]                     # [r, i, j]
    idx = np.arange(K)
    before = (gj > gi) | ((gj == gi) & (idx[None, None, :] < idx[None, :, None]))
    rank = before.sum(2)
    live = (rank < k) & ((g >= tau) | (rank == 0))
    S = np.zeros(n, np.float32)
    for i in range(K):                                        # index order, fp32
        S = np.where(live[:, i], S + g[:, i], S).astype(np.float32)
    used = np.where(live, g, np.float32(0)).astype(np.float32)
    if renormalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            used = np.where(live, g / S[:, None], np.float32(0)).astype(np.float32)
    lists = [np.nonzero(live[:, i])[0].astype(np.int32) for i in range(K)]
    count = np.array([len(l) for l in lists], np.int32)
    return {"live": live.astype(np.uint8), "gate_used": used, "list": lists, "count": count,
            "S": S, "rank": rank}


def combine_ref(gate, op_k, depth_k, rgb_k, bg):
    """rn_ml_combine_test in fp32, its operation order: gate (n, K), op_k /
    depth_k (K, n), rgb_k (K, n, 3), bg (3,) -> rgb (n, 3), opacity, depth."""
    f = np.float32
    n, K = gate.shape
    rgb, op, de = np.zeros((n, 3), f), np.zeros(n, f), np.zeros(n, f)
    for i in range(K):
        gi = gate[:, i].astype(f)
        rest = (f(1) - op_k[i]).astype(f)
        for c in range(3):
            term = (rgb_k[i, :, c] + (bg[c] * rest).astype(f)).astype(f)
            rgb[:, c] = (rgb[:, c] + (term * gi).astype(f)).astype(f)
        op = (op + (op_k[i] * gi).astype(f)).astype(f)
        de = (de + (depth_k[i] * gi).astype(f)).astype(f)
    return rgb, op, de


def softmax_rows(n, K, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, K)) * spread).astype(np.float32)
    e = np.exp(z - z.max(1, keepdims=True)).astype(np.float32)
    return (e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def crafted_rows(K):
    """Rows that probe the rules: all equal (exactly 1/K), pairs of equal
    gates, zeros, denormals, saturated rows (one gate 1, the rest 0 or 1e-30),
    a descending and an ascending ramp."""
    f = np.float32
    rows = [np.full(K, f(1) / f(K), f)]
    sat = np.zeros(K, f); sat[K - 1] = 1
    rows.append(sat)
    sat2 = np.full(K, 1e-30, f); sat2[0] = 1
    rows.append(sat2)
    den = np.full(K, 1e-40, f); den[K // 2] = 1                 # denormal gates
    rows.append(den)
    tie = np.zeros(K, f); tie[0] = tie[K - 1] = 0.5             # two equal maxima
    rows.append(tie)
    tie2 = np.full(K, 0.25 / max(K - 2, 1), f); tie2[-1] = tie2[-2] = 0.375
    rows.append(tie2)
    zden = np.zeros(K, f); zden[K - 1] = 1e-40; zden[0] = 1e-40  # equal denormals and zeros
    rows.append(zden)
    ramp = np.arange(K, 0, -1).astype(f); ramp /= ramp.sum()
    rows += [ramp, ramp[::-1].copy()]
    return np.stack(rows).astype(f)


def gate_rows(n, K, seed):
    """n rows: the crafted ones (cycled through) interleaved with softmax rows."""
    soft, craft = softmax_rows(n, K, seed), crafted_rows(K)
    g = soft.copy()
    pos = np.arange(0, n, 3)
    g[pos] = craft[np.arange(len(pos)) % len(craft)]
    return np.ascontiguousarray(g)
