"""Depth supervision's three kernels restated in numpy (test code: the package
does not import it), in the operation order include/radnerf.h states:

  * rn_gather_depth        gather_depth: fp32, bit for bit;
  * rn_ml_composite_depth  seg_var (fp64) / seg_var_f32 (the lanes' fmaf order),
    _fw / _bw              seg_seed_terms, seg_dsigma (fp64, analytic) and
                           seg_loss (fp64, the function central differences and
                           autograd differentiate);
  * rn_depth_loss          depth_loss: the two terms and the three seeds in
                           fp64 or fp32.

Per segment the weights are w_s = a_s prod_{j<s} (1 - a_j), a = 1 - exp(-sigma
delta); the first m samples contribute (m - 1 is the termination sample) and
everything past them is exactly zero.  phi_s = min((t_s - z)^2, clip^2), and
z <= 0 means "no measurement": V = 0 and no gradient.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
WAVE = 64


# ---------------------------------------------------------------------------
# rn_gather_depth
# ---------------------------------------------------------------------------
def gather_depth(depths, scale, kind, directions, img_idxs, pix_idxs):
    """target_t (n,) fp32.  depths (N, P) uint16 or fp32; kind 0: v * scale;
    kind 1: (v * scale) / sqrt((dx dx + dy dy) + dz dz), every operation one
    correctly rounded fp32 operation.  0 for v <= 0, NaN, a result not > 0 and
    a pick outside the maps."""
    depths = np.asarray(depths)
    N, P = depths.shape
    n = len(img_idxs)
    out = np.zeros(n, F32)
    s = F32(scale)
    with np.errstate(all="ignore"):
        for r in range(n):
            im, px = int(img_idxs[r]), int(pix_idxs[r])
            if not (0 <= im < N and 0 <= px < P):
                continue
            v = F32(depths[im, px])
            if not v > F32(0):
                continue
            t = F32(v * s)
            if kind == 1:
                d = np.asarray(directions[px], F32)
                q = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
                t = F32(t / np.sqrt(q, dtype=F32))
            out[r] = t if t > F32(0) else F32(0)
    return out


# ---------------------------------------------------------------------------
# the composite's term
# ---------------------------------------------------------------------------
def weights(sig, dl, m=None):
    """(w, T after each sample) in fp64 of the first m samples (all by default)"""
    sig, dl = np.asarray(sig, F64), np.asarray(dl, F64)
    m = len(sig) if m is None else m
    a = 1.0 - np.exp(-sig[:m] * dl[:m])
    t_in = np.cumprod(1.0 - a)
    t_ex = np.concatenate([[1.0], t_in[:-1]])
    return a * t_ex, t_in


def phi(t, z, clip):
    """min((t - z)^2, clip^2) in the dtype of t; 0 everywhere for z <= 0"""
    t = np.asarray(t)
    if not z > 0:
        return np.zeros_like(t)
    e = t - t.dtype.type(z)
    c = t.dtype.type(clip)
    with np.errstate(over="ignore"):
        return np.minimum(e * e, c * c)


def seg_var(w, t, z, clip):
    """V = sum w phi in fp64 (w, t: the contributing samples)"""
    return float((np.asarray(w, F64) * phi(np.asarray(t, F64), float(z), float(clip))).sum())


def _fmaf(a, b, c):
    # fp32 products are exact in fp64; the one fp64 rounding before the fp32
    # one differs from a fused operation in rare half-way cases only
    return F32(F64(a) * F64(b) + F64(c))


def seg_var_f32(w, t, z, clip):
    """the forward kernel's order: lane l folds samples l, l + 64, ... with
    acc = fmaf(w, phi, acc); the 64 lanes are summed by an xor butterfly"""
    w, t = np.asarray(w, F32), np.asarray(t, F32)
    acc = np.zeros(WAVE, F32)
    if z > 0:
        p = phi(t, F32(z), clip)            # clip^2: one fp32 multiply, as the entry's
        for i in range(len(w)):
            acc[i % WAVE] = _fmaf(w[i], p[i], acc[i % WAVE])
    off = WAVE // 2
    while off:
        acc = (acc + acc[np.arange(WAVE) ^ off]).astype(F32)
        off //= 2
    return float(acc[0])


def dist_loss(w, t, d):
    """the Mip-NeRF 360 distortion loss of one segment (losses.cu:47-110)"""
    wi, wti = np.cumsum(w), np.cumsum(w * t)
    wex, wtex = wi - w, wti - w * t
    return float((2 * w * (t * wex - wtex) + w * w * d / 3).sum())


def dist_grad(w, t, d):
    """its gradient in w (losses.cu:113-142)"""
    wi, wti = np.cumsum(w), np.cumsum(w * t)
    wex, wtex = wi - w, wti - w * t
    front = t * wex - wtex
    back = (wti[-1] - wti) - t * (wi[-1] - wi)
    return 2 * (front + back) + (2.0 / 3) * w * d


def seg_seed_terms(w, t, d, z, clip, gv, g_dist=0.0):
    """(gw per sample, wtot) as the backward kernel forms them:
    gw_s = gw_dist_s + gv phi_s, wtot = 2 g dist + gv V"""
    w, t, d = (np.asarray(a, F64) for a in (w, t, d))
    p = phi(t, float(z), float(clip))
    gw = gv * p
    wtot = gv * float((w * p).sum())
    if g_dist:
        gw = g_dist * dist_grad(w, t - t[0], d) + gw
        wtot = 2 * g_dist * dist_loss(w, t - t[0], d) + wtot
    return gw, wtot


def seg_loss(sig, dl, ts, z, clip, gv, m=None, g_dist=0.0):
    """gv V + g_dist dist of the segment's first m samples, fp64"""
    w, _ = weights(sig, dl, m)
    m = len(w)
    t, d = np.asarray(ts, F64)[:m], np.asarray(dl, F64)[:m]
    out = gv * seg_var(w, t, z, clip)
    if g_dist:
        out += g_dist * dist_loss(w, t - t[0], d)
    return out


def seg_dsigma(sig, dl, ts, z, clip, gv, m=None, g_dist=0.0):
    """dL/dsigma_s = delta_s [T_{s+1} gw_s - (wtot - sum_{j<=s} gw_j w_j)] of
    seg_loss, fp64; zero past sample m - 1"""
    n = len(sig)
    w, T = weights(sig, dl, m)
    m = len(w)
    t, d = np.asarray(ts, F64)[:m], np.asarray(dl, F64)[:m]
    gw, wtot = seg_seed_terms(w, t, d, z, clip, gv, g_dist)
    out = np.zeros(n)
    out[:m] = d * (T * gw - (wtot - np.cumsum(gw * w)))
    return out


# ---------------------------------------------------------------------------
# rn_depth_loss
# ---------------------------------------------------------------------------
def depth_loss(depth, gate, dvar_k, target_t, ray_weight, lambda_depth, lambda_depth_var,
               dtype=F64):
    """terms (the sums divided by B) and the seeds the kernel ADDS: d_depth,
    d_gate (B, K), d_dvar [K][B] (None without dvar_k), in `dtype` arithmetic in
    the header's order (the sums over rays are plain numpy sums)."""
    f = dtype
    depth, gate = np.asarray(depth, f), np.asarray(gate, f)
    B, K = gate.shape
    z = np.asarray(target_t, f)
    m = z > 0
    rw = np.ones(B, f) if ray_weight is None else np.asarray(ray_weight, f)
    ld, lv = f(lambda_depth), f(lambda_depth_var)
    d_depth, d_gate = np.zeros((B, K), f), np.zeros((B, K), f)
    l0 = np.zeros(B, f)
    if lambda_depth > 0:
        mean = np.zeros(B, f)
        for k in range(K):
            mean = (mean + gate[:, k] * depth[:, k]).astype(f)
        e = (mean - z).astype(f)
        l0 = np.where(m, ld * (e * e), f(0)).astype(f)
        s = np.where(m, ((f(2) * ld / f(B)) * e) * rw, f(0)).astype(f)
        d_depth = (s[:, None] * gate).astype(f)
        d_gate = (s[:, None] * depth).astype(f)
    terms = {"depth": float(l0.astype(F64).sum()) / B}
    d_dvar = None
    if dvar_k is not None:
        V = np.asarray(dvar_k, f)                        # [K][B]
        acc = np.zeros(B, f)
        for k in range(K):
            acc = (acc + gate[:, k] * V[k]).astype(f)
        l1 = np.where(m, lv * acc, f(0)).astype(f)
        s = np.where(m & (lambda_depth_var > 0), (lv / f(B)) * rw, f(0)).astype(f)
        d_dvar = (s[None, :] * gate.T).astype(f)
        d_gate = (d_gate + s[:, None] * V.T).astype(f)
        terms["depth_var"] = float(l1.astype(F64).sum()) / B
    return terms, d_depth, d_gate, d_dvar
