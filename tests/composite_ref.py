"""The compositing kernels of csrc/composite.hip restated in numpy with fp64
products and sums (test code: the package does not import it), each output with
the rounding scale that bounds an fp32 evaluation of it, plus the segments that
aim at the wave kernels' special cases.

Written from the formulas the kernel comments cite: volumerendering.cu:6-45
(forward), :87-152 (backward), :206-250 (test-time step), losses.cu:47-142
(distortion loss and its gradient) and the gated combine's seeds.  Plain
serial code per segment; nothing is shared with the kernels or the fp32 oracle
except what is discrete or bit-exact by design:

  * the per-sample alpha is the fp32 value 1 - det_expf(-sigma * delta)
    (oracle.det_expf, bit-identical to the kernels' rn_exp_det).  1 - alpha is
    exact in fp32 (Sterbenz, on either side of 1/2), so fp64 1 - alpha is the
    kernels' factor;
  * the termination sample `used` of a segment is an input (the fp32 oracle's
    serial fold; the tests assert the kernels' equals it).  Samples 0..used
    contribute and get gradients, m = min(used + 1, n) of them; everything past
    is exactly zero;
  * the backward functions take what the kernels' ABI takes: the forward's
    opacity / depth / rgb, `ws` where a kernel reads it, the segment's loss
    where the in-chain distortion backward reads it.  They are functions of
    those fp32 arrays as given.

With these fixed, a kernel and this file differ by the roundings of products
and sums alone.  A length-n sum or product evaluated in any order is within
n eps sum|terms| of the exact one (eps = 2^-24), so per output element

    |kernel - ref| <= (length + c) eps scale,

scale = the sum of the absolute values of every term that enters the element in
the form the kernel under test adds them, c the elementwise roundings outside
the long sums (BARS below).  A term that runs through two (three) long scans
before it reaches the element -- a prefix sum of products of scanned values --
is counted two (three) times in the scale, which keeps the one factor
(m + 16).  Where the reference is exactly zero the kernel's value must be zero.
"""
import numpy as np

import oracle

F32 = np.float32
F64 = np.float64
EPS = 2.0 ** -24
THR = 1e-4
WAVE = 64

# ---------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------


def bar_ws(ws, k):
    """w = a * T_ex: k - 1 factors of T_ex, the product with a."""
    return (k + 2) * EPS * np.abs(ws)


def bar_out(value, m):
    """opacity / depth / rgb of m non-negative terms (value = its own scale)."""
    m = np.asarray(m, F64)
    return (m.reshape(m.shape + (1,) * (np.ndim(value) - m.ndim)) + 2) * EPS * np.abs(value)


def bar_drgb(drgb, k):
    """g_c w: w as above, the seed's one rounding (ml fold), the product."""
    return (k[:, None] + 3) * EPS * np.abs(drgb)


def bar_sum(scale, m):
    """dsigma, the distortion loss and its dL_dws."""
    return (np.asarray(m, F64) + 16) * EPS * scale


def ratios(got, ref, bar):
    """|got - ref| / bar per element; inf where the reference is exactly zero
    and the value is not, or where the value is not finite."""
    got, ref, bar = (np.asarray(a, F64) for a in (got, ref, bar))
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bar)
    r = np.where((ref == 0) & (got != 0), np.inf, r)
    return np.where(np.isfinite(got), r, np.inf)


def check(name, got, ref, bar, out=None):
    """assert got within bar of ref everywhere, zeros exactly; returns (and
    records in `out`) the largest error / bound ratio"""
    r = ratios(got, ref, bar)
    worst = float(r.max()) if r.size else 0.0
    if out is not None:
        out[name] = max(out.get(name, 0.0), worst)
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f"{name}: element {i} got {np.asarray(got)[i]!r} ref "
                             f"{np.asarray(ref)[i]!r} bar {np.asarray(bar)[i]:.3e} "
                             f"(ratio {worst:.3g}); {int((r > 1).sum())} of {r.size} outside")
    return worst


# ---------------------------------------------------------------------------
# layout helpers
# ---------------------------------------------------------------------------


def alphas(sig, dl):
    """fp32 1 - det_expf(-sigma * delta) per sample, as kernels and oracle form it"""
    x = ((-np.asarray(sig, F32)) * np.asarray(dl, F32)).astype(F32)
    return (F32(1) - oracle.det_expf(x).reshape(x.shape)).astype(F32)


def layout(cap, starts, counts, used):
    """per sample: k (1-based index in its segment, 0 in padding), seg (segment
    number, -1 in padding), m (its segment's contributing count); per segment m"""
    k = np.zeros(cap, np.int64)
    seg = np.full(cap, -1, np.int64)
    m = np.minimum(np.asarray(used, np.int64) + 1, np.asarray(counts, np.int64))
    for j, (a, n) in enumerate(zip(starts, counts)):
        k[a:a + n] = np.arange(1, n + 1)
        seg[a:a + n] = j
    return dict(k=k, seg=seg, inside=seg >= 0, m=m, m_s=np.where(seg >= 0, m[seg], 0))


# ---------------------------------------------------------------------------
# forward (volumerendering.cu:6-45)
# ---------------------------------------------------------------------------


def _weights(alpha, m):
    """(w, T after each sample) of the m contributing samples"""
    a = alpha[:m].astype(F64)
    t_in = np.cumprod(1.0 - a)
    t_ex = np.concatenate([[1.0], t_in[:-1]])
    return a * t_ex, t_in


def forward(alpha, rgbs, ts, starts, counts, used):
    """ws (cap; zero past the termination sample and in padding), opacity,
    depth (n_seg), rgb (n_seg, 3).  Each value is its own rounding scale."""
    cap, ns = len(alpha), len(counts)
    ws = np.zeros(cap)
    op, de, rgb = np.zeros(ns), np.zeros(ns), np.zeros((ns, 3))
    for j, (a0, n, u) in enumerate(zip(starts, counts, used)):
        m = min(int(u) + 1, int(n))
        if m <= 0:
            continue
        w, _ = _weights(alpha[a0:a0 + n], m)
        ws[a0:a0 + m] = w
        op[j] = w.sum()
        de[j] = (w * ts[a0:a0 + m].astype(F64)).sum()
        rgb[j] = (w[:, None] * rgbs[a0:a0 + m].astype(F64)).sum(0)
    return dict(ws=ws, opacity=op, depth=de, rgb=rgb)


# ---------------------------------------------------------------------------
# distortion loss (losses.cu:47-142) of given ws
# ---------------------------------------------------------------------------


def _dist_scans(w, t):
    wi, wti = np.cumsum(w), np.cumsum(w * t)
    return wi, wti, wi - w, wti - w * t


def distortion_fw(ws, dl, ts, starts, counts, rel):
    """loss per segment of the fp32 `ws` as given, and its scale.  rel: the
    in-chain form 2 w (t' W_ex - WT'_ex), t' = t - t_0 (each leaf through the
    scan and the sum over samples: twice); else k_distortion_fw's
    2 (WT_in W_ex - W_in WT_ex) on absolute t (a product of two scans, summed:
    three times).  Also the inclusive scans of w and w t (absolute t)."""
    ns, cap = len(counts), len(ws)
    loss, scale = np.zeros(ns), np.zeros(ns)
    wi_all, wti_all = np.zeros(cap), np.zeros(cap)
    for j, (a0, n) in enumerate(zip(starts, counts)):
        if n <= 0:
            continue
        s = slice(a0, a0 + n)
        w, t, d = ws[s].astype(F64), ts[s].astype(F64), dl[s].astype(F64)
        wi, wti, wex, wtex = _dist_scans(w, t)
        wi_all[s], wti_all[s] = wi, wti
        tr = t - t[0]
        _, _, _, wtrex = _dist_scans(w, tr)
        own = w * w * d / 3
        loss[j] = (2 * w * (tr * wex - wtrex) + own).sum()
        if rel:
            scale[j] = 2 * (2 * w * (tr * wex + wtrex) + own).sum()
        else:
            scale[j] = 3 * (2 * (wti * wex + wi * wtex) + own).sum()
    return dict(loss=loss, scale=scale, ws_incl=wi_all, wts_incl=wti_all)


def _dist_grad(g, w, t, d):
    """dL_dws of one segment for the seed g, and the sum of |terms| (t as given:
    absolute, or relative to the first sample)"""
    wi, wti, wex, wtex = _dist_scans(w, t)
    wtot, wttot = wi[-1], wti[-1]
    front = t * wex - wtex
    back = (wttot - wti) - t * (wtot - wi)
    own = (2.0 / 3) * w * d
    gw = g * 2 * (front + back) + g * own
    sc = abs(g) * (2 * (np.abs(t) * wex + np.abs(wtex) + np.abs(wttot) + np.abs(wti)
                        + np.abs(t) * (wtot + wi)) + own)
    return gw, sc


def distortion_bw(g, ws, dl, ts, starts, counts):
    """k_distortion_bw's dL_dws (every sample of the segment, absolute t) for
    the per-segment seeds g, and its scale"""
    cap = len(ws)
    out, scale = np.zeros(cap), np.zeros(cap)
    for j, (a0, n) in enumerate(zip(starts, counts)):
        if n <= 0:
            continue
        s = slice(a0, a0 + n)
        out[s], scale[s] = _dist_grad(float(g[j]), ws[s].astype(F64), ts[s].astype(F64),
                                      dl[s].astype(F64))
    return out, scale


# ---------------------------------------------------------------------------
# backward (volumerendering.cu:87-152)
# ---------------------------------------------------------------------------


def fold_seeds(gate, bg, gRGB, gO, gDepth):
    """k_ml_composite_bw's per-segment seeds, segment k B + r:
    dRGB_k = g_k dL/drgb, dO_k = g_k (dL/dO - bg . dL/drgb), dD_k = dL/ddepth[:, k]
    (zero when gDepth is None), and the absolute sums behind them."""
    gate, bg, gRGB, gO = (np.asarray(a, F64) for a in (gate, bg, gRGB, gO))
    B, K = gate.shape
    g = gate.T                                                   # [K][B]
    gr = g[:, :, None] * gRGB[None]
    go = g * (gO - gRGB @ bg)[None]
    go_abs = np.abs(g) * (np.abs(gO) + np.abs(gRGB) @ np.abs(bg))[None]
    gd = np.zeros((K, B)) if gDepth is None else np.asarray(gDepth, F64).T
    return dict(gRGB=gr.reshape(-1, 3), gO=go.reshape(-1), gD=gd.reshape(-1),
                gO_abs=go_abs.reshape(-1))


def backward(alpha, rgbs, dl, ts, starts, counts, used, opacity, depth, rgb, gO, gD, gRGB,
             gO_abs=None, gw=None, ws=None, gdist=None, dist=None, defect=None):
    """dsigma (cap), drgb (cap, 3) and dsigma's scale.  opacity / depth / rgb are
    the forward's fp32 outputs as the kernel receives them; seeds per segment.

    gw + ws: dL_dws given (rn_composite_train_bw); the kernel reads ws only for
    the products gw_j ws_j.  gdist + dist + ws: the in-chain distortion backward
    (k_ml_composite_dist_bw): dL_dws is the distortion gradient of `ws` for the
    seed gdist with t relative to the segment's first sample, and the total of
    dL_dws ws is 2 gdist dist with `dist` the forward's loss as given.

    defect (the checker's self-test): ("carry", b) drops the carry of the red
    prefix sum into chunk b; "exclusive" uses exclusive prefix sums;
    "nodepth" drops the depth term."""
    cap = len(alpha)
    dsig, scale, drgb = np.zeros(cap), np.zeros(cap), np.zeros((cap, 3))
    gO_abs = np.abs(gO) if gO_abs is None else gO_abs
    for j, (a0, n, u) in enumerate(zip(starts, counts, used)):
        m = min(int(u) + 1, int(n))
        if m <= 0:
            continue
        s = slice(a0, a0 + m)
        w, T = _weights(alpha[a0:a0 + n], m)
        c, t, d = rgbs[s].astype(F64), ts[s].astype(F64), dl[s].astype(F64)
        g3 = np.asarray(gRGB[j], F64)
        R, O, D = np.asarray(rgb[j], F64), float(opacity[j]), float(depth[j])
        pc, pd = np.cumsum(w[:, None] * c, 0), np.cumsum(w * t)
        if defect == "exclusive":
            pc, pd = pc - w[:, None] * c, pd - w * t
        elif isinstance(defect, tuple) and m > WAVE * defect[1]:
            pc = pc.copy()
            pc[WAVE * defect[1]:, 0] -= pc[WAVE * defect[1] - 1, 0]
        drgb[s] = g3[None] * w[:, None]
        v = ((c * T[:, None] - (R[None] - pc)) * g3[None]).sum(1) + float(gO[j]) * (1 - O)
        sc = ((c * T[:, None] + (np.abs(R)[None] + np.abs(pc))) * np.abs(g3)[None]).sum(1) \
            + float(gO_abs[j]) * (1 + abs(O))
        if defect != "nodepth":
            v = v + float(gD[j]) * (t * T - (D - pd))
        sc = sc + abs(float(gD[j])) * (t * T + abs(D) + pd)
        if gw is not None:
            sf = slice(a0, a0 + n)          # the scan of gw ws runs over the whole segment
            q = gw[sf].astype(F64) * ws[sf].astype(F64)
            pre = np.cumsum(q)[:m]
            v = v + T * gw[s].astype(F64) - (q.sum() - pre)
            sc = sc + T * np.abs(gw[s].astype(F64)) + np.abs(q).sum() + np.cumsum(np.abs(q))[:m]
        elif gdist is not None:
            sf = slice(a0, a0 + n)
            wf, tf = ws[sf].astype(F64), ts[sf].astype(F64)
            g = float(gdist[j])
            gwf, gsf = _dist_grad(g, wf, tf - tf[0], dl[sf].astype(F64))
            wtot = 2 * g * float(dist[j])
            v = v + T * gwf[:m] - (wtot - np.cumsum(gwf * wf)[:m])
            sc = sc + T * gsf[:m] + abs(wtot) + 2 * np.cumsum(gsf * wf)[:m]
        dsig[s], scale[s] = d * v, d * sc
    return dict(dsig=dsig, drgb=drgb, scale=scale)


# ---------------------------------------------------------------------------
# test-time step (volumerendering.cu:206-250)
# ---------------------------------------------------------------------------


def composite_test(alpha, rgbs, ts, n_eff, opacity, depth, rgb, thr=THR):
    """One composite_test_fw call on prior opacity / depth / rgb per alive row
    (already gathered).  Returns the new values, m (the prior and the processed
    samples: the terms of each sum) and `dead` (n_eff == 0 or T <= thr reached).
    The break is the serial fp32 fold T = (1 - O) prod (1 - a), exact products
    aside the same operations in kernel and oracle."""
    na = len(n_eff)
    op, de, col = (np.array(a, F64) for a in (opacity, depth, rgb))
    m, dead = np.ones(na, np.int64), np.zeros(na, bool)
    for i in range(na):
        if n_eff[i] == 0:
            dead[i] = True
            continue
        T32 = F32(1) - F32(opacity[i])
        p = int(n_eff[i])
        for s in range(p):
            T32 = F32(T32 * (F32(1) - alpha[i, s]))
            if T32 <= F32(thr):
                p, dead[i] = s + 1, True
                break
        a = alpha[i, :p].astype(F64)
        t_in = (1.0 - op[i]) * np.cumprod(1.0 - a)
        w = a * np.concatenate([[1.0 - op[i]], t_in[:-1]])
        op[i] += w.sum()
        de[i] += (w * ts[i, :p].astype(F64)).sum()
        col[i] += (w[:, None] * rgbs[i, :p].astype(F64)).sum(0)
        m[i] = p + 1
    return dict(opacity=op, depth=de, rgb=col, m=m, dead=dead)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023,
          1024)
# optical depth sum(sigma delta): T ends at 0.6 / 0.05 (never terminates), crosses
# 1e-4 = exp(-9.2) three quarters in (12) or a quarter in (40)
TAUS = (0.5, 3.0, 12.0, 40.0)
# (n, forced break sample): lane 0, lane 63, mid-chunk, the segment's last
# sample at lane 63 and at lane 0
FORCED = ((128, 64), (129, 63), (200, 100), (128, 127), (65, 64), (1024, 20))
FLUSH = (192, 70)           # sigma delta = 120 at sample 70: the exponent is 0, T = 0 from there
ZERO_N = 1024               # one segment with every sigma = 0
SEED_SIZE = (1.0, 0.1, 0.01)    # per-segment size of the loss seeds, cyclic


def make_segments(seed=31):
    """The segment pool: dicts of sig, rgbs, dl, ts (fp32) with `n` and `want`
    (the intended termination sample, "never" or None for wherever the fold
    says).  30 % of the sigmas are zero; ts start 0.05 .. 6 from the origin."""
    rng = np.random.default_rng(seed)
    spec = [(n, tau, None) for n in COUNTS for tau in TAUS]
    spec += [(n, 0.7, e) for n, e in FORCED] + [(FLUSH[0], 0.7, FLUSH[1]), (ZERO_N, 0.0, None)]
    t0s = np.linspace(0.05, 6.0, len(spec))
    segs = []
    for i, (n, tau, e) in enumerate(spec):
        dl = rng.uniform(1e-3, 5e-3, n).astype(F32)
        ts = (np.cumsum(dl, dtype=F64) + t0s[(7 * i) % len(spec)]).astype(F32)
        zero = rng.random(n) < 0.3
        live = max(1, int((~zero[:n if e is None else e]).sum()))
        sig = rng.uniform(0, 2 * tau / live, n) / dl
        sig[zero] = 0.0
        want = None
        if e is not None:
            sig[e] = (120.0 if (n, e) == FLUSH else 12.0) / dl[e]
            want = e
        elif tau <= 3.0:
            want = "never"
        segs.append(dict(n=n, tau=tau, want=want, sig=sig.astype(F32), dl=dl, ts=ts,
                         rgbs=rng.random((n, 3), dtype=F32)))
    return segs


def pack(segs, K=1, B=None, align=1):
    """Flat sample arrays of `segs` laid out as K sub-NeRFs of B segments each
    (segment k B + r; missing ones empty), every sub-NeRF's base and the
    capacity rounded up to `align`.  Padding: sigma 0, delta 1e-3, t 0, rgb 0.5."""
    B = len(segs) if B is None else B
    assert len(segs) <= K * B
    counts = np.zeros(K * B, np.int32)
    counts[:len(segs)] = [s["n"] for s in segs]
    starts = np.zeros(K * B, np.int32)
    base = 0
    for k in range(K):
        base = -(-base // align) * align
        c = counts[k * B:(k + 1) * B]
        starts[k * B:(k + 1) * B] = base + np.concatenate([[0], np.cumsum(c)[:-1]])
        base += int(c.sum())
    cap = max(align, -(-base // align) * align)
    sig, dl, ts = np.zeros(cap, F32), np.full(cap, 1e-3, F32), np.zeros(cap, F32)
    rgbs = np.full((cap, 3), 0.5, F32)
    for s, a in zip(segs, starts):
        n = s["n"]
        sig[a:a + n], dl[a:a + n], ts[a:a + n], rgbs[a:a + n] = s["sig"], s["dl"], s["ts"], s["rgbs"]
    return dict(sig=sig, dl=dl, ts=ts, rgbs=rgbs, starts=starts, counts=counts, cap=cap, K=K, B=B,
                want=[s["want"] for s in segs] + [None] * (K * B - len(segs)))


# (K, B) of the fused layout -> the pool's segments it holds (pool order: COUNTS
# x TAUS, then FORCED, FLUSH, the all-zero segment); (4, 22) holds all 88
ML_SHAPES = {(1, 1): (79,),
             (2, 7): (80, 81, 82, 83, 84, 85, 86, 87, 0, 5, 18, 22, 75, 30),
             (3, 5): (78, 76, 3, 7, 9, 14, 27, 33, 38, 43, 50, 55, 62, 67, 71),
             (4, 22): tuple(range(88))}
SEG_ALIGN = 128             # radnerf_amd.fused.SEG_ALIGN (asserted by the GPU test)


def ml_case(segs, K, B):
    return pack([segs[i] for i in ML_SHAPES[(K, B)]], K, B, SEG_ALIGN)


def rows_of(p, ray=None):
    """rays_a (ray, start, count) int64 of a packed set; ray defaults to the row"""
    ns = len(p["counts"])
    ray = np.arange(ns) if ray is None else ray
    return np.stack([ray, p["starts"], p["counts"]], 1).astype(np.int64)


def oracle_used(p):
    """the fp32 oracle's forward on a packed set (segment order): its `used` is
    the termination input of every reference function here"""
    used, op, de, rgb, ws = oracle.composite_train_fw(p["sig"], p["rgbs"], p["dl"], p["ts"],
                                                      rows_of(p), THR)
    return dict(used=used, opacity=op, depth=de, rgb=rgb, ws=ws)


def prepare(p):
    """a packed set with its alphas, the oracle's forward (`orc`) and the layout"""
    p = dict(p)
    p["alpha"] = alphas(p["sig"], p["dl"])
    p["orc"] = oracle_used(p)
    p["lay"] = layout(p["cap"], p["starts"], p["counts"], p["orc"]["used"])
    return p


def check_conditions(p, used, early=True):
    """what the inputs were built for did come out (asserted on the oracle):
    every forced break where intended and, on the whole pool, at least 15 % of
    the non-empty segments terminating early"""
    n = p["counts"].astype(np.int64)
    some = n > 0
    if early:
        assert ((used < n) & some).sum() >= 0.15 * some.sum()
    for j, w in enumerate(p["want"]):
        if w == "never":
            assert used[j] == n[j], (j, used[j], n[j])
        elif w is not None:
            assert used[j] == w, (j, used[j], w)


def seeds(n_seg, rng):
    """per-segment loss seeds gO, gD (n_seg), gRGB (n_seg, 3): N(0, 1) times the
    segment's SEED_SIZE"""
    size = np.array([SEED_SIZE[j % len(SEED_SIZE)] for j in range(n_seg)], F32)
    gO = (rng.normal(0, 1, n_seg) * size).astype(F32)
    gD = (rng.normal(0, 1, n_seg) * size).astype(F32)
    gR = (rng.normal(0, 1, (n_seg, 3)) * size[:, None]).astype(F32)
    return gO, gD, gR


def ml_seeds(K, B, rng):
    """the combine's seeds for K sub-NeRFs of B rays: gate (B, K) rows summing
    to 1 with one entry exactly 0 (when there is more than one), a non-trivial
    bg, gRGB (B, 3), gO (B), gDepth (B, K); sized per ray by SEED_SIZE"""
    gate = rng.random((B, K)).astype(F32) + F32(0.05)
    if K * B > 1:
        gate[B // 2, K - 1] = 0.0
    gate = (gate / np.maximum(gate.sum(1, keepdims=True), F32(1e-6))).astype(F32)
    size = np.array([SEED_SIZE[r % len(SEED_SIZE)] for r in range(B)], F32)
    return dict(gate=gate, bg=rng.uniform(0.1, 1.0, 3).astype(F32),
                gRGB=(rng.normal(0, 1, (B, 3)) * size[:, None]).astype(F32),
                gO=(rng.normal(0, 1, B) * size).astype(F32),
                gDepth=(rng.normal(0, 1, (B, K)) * size[:, None]).astype(F32))


def fold_seeds_f32(gate, bg, gRGB, gO, gDepth):
    """fold_seeds in fp32 with k_ml_composite_bw's operation order (what the
    fp32 oracle is fed when it stands in for that kernel)"""
    f = F32
    gr = (gate.T[:, :, None] * gRGB[None]).astype(f)
    bgdot = (f(bg[0]) * gRGB[:, 0] + f(bg[1]) * gRGB[:, 1]).astype(f)
    bgdot = (bgdot + f(bg[2]) * gRGB[:, 2]).astype(f)
    go = (gate.T * (gO - bgdot)[None]).astype(f)
    gd = np.zeros_like(go) if gDepth is None else np.ascontiguousarray(gDepth.T)
    return gr.reshape(-1, 3), go.reshape(-1), gd.reshape(-1)


def step_inputs(n_alive, n_samples, seed):
    """One composite_test_fw call: n_alive rows of n_samples samples on n_rays >
    n_alive rays with prior opacity in [0, 0.9999), n_eff from 0 to full, sigma
    sized so that part of the rows reach T <= 1e-4 inside the call."""
    rng = np.random.default_rng(seed)
    n_rays = n_alive + 5
    dl = rng.uniform(1e-3, 5e-3, (n_alive, n_samples)).astype(F32)
    ts = (np.cumsum(dl, 1, dtype=F64) + rng.uniform(0.05, 6.0, (n_alive, 1))).astype(F32)
    tau = rng.choice([0.5, 3.0, 12.0, 40.0], (n_alive, 1))
    sig = rng.uniform(0, 2 * tau / n_samples, (n_alive, n_samples)) / dl
    sig[rng.random((n_alive, n_samples)) < 0.3] = 0.0
    n_eff = rng.integers(0, n_samples + 1, n_alive).astype(np.int32)
    n_eff[0] = n_samples
    if n_alive > 1:
        n_eff[1] = 0
    op = rng.uniform(0, 0.9999, n_rays).astype(F32)
    op[op >= F32(0.9999)] = F32(0.5)
    op[::4] = op[::4] * F32(0.01)           # rays that have hardly met anything yet
    return dict(sig=sig.astype(F32), dl=dl, ts=ts, rgbs=rng.random((n_alive, n_samples, 3), dtype=F32),
                n_eff=n_eff, alive=rng.permutation(n_rays)[:n_alive].astype(np.int64), opacity=op,
                depth=(rng.random(n_rays) * 6).astype(F32), rgb=rng.random((n_rays, 3), dtype=F32))
