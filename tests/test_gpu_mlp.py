"""The field's two MLPs on MFMA (csrc/rn_field.h mlp_forward, sh_lane; csrc/field.hip
bwd_window, the dW ownership and block scales; csrc/field_aux.hip dx_chain), per
activation and per weight against the fp64 reference tests/mlp_ref.py, whose
docstring derives every bound used here (DESIGN.md section 2 has the summary and
the measured ratios).  The reference takes the kernel's own f16 encoding
cache, the f16 weights, the fp32 directions and seeds as given.

  (a) forward: the 16 geo features inside [rn16(v - 2a), rn16(v + 2a)], sigma
      and rgb within their bounds, sigma / rgb / geo features bit-identical
      between the entry points; dense and eight banded weight sets, scales
      0.5 and 16, every prefix count; nothing excluded
  (b) SH per coefficient through the probe weights: the f16 the kernel fed to
      the rgb net, recovered from rgb, inside [rn16(Y - s), rn16(Y + s)]
  (c) dW of rn_field_bwd per weight, all 9472 of each sub-NeRF, nine seed sets
      (two scales, zero iterations and tiles, magnitude steps), one block
      walking all iterations and one block per iteration; the other
      sub-NeRFs' gradients exactly 0
  (d) grid gradient per entry (rn_field_bwd), dL/dxyz and dL/ddir per sample
      (rn_field_dinput) with a live MLP
  (e) the production chain (ml_render_fused on lattice rays): the three
      forwards bit-identical with a live rgb net, sigma and rgb within (a),
      dW per weight for rn_field_bwd_merged (fp32 and fixed-point scatter) and
      rn_field_bwd_merged_det + rn_reduce_partials
  (f) scale equivariance: deterministic gradients bitwise 2^k times the
      unscaled run's under seeds times 2^k

A model of three sub-NeRFs carries three weight sets at a time and each is
exercised in turn.  Every test prints its largest error / bound.
"""
import numpy as np
import pytest
import torch

from radnerf_amd.networks import MNGP

import encode_ref as ER
import mlp_ref as MR

pytestmark = pytest.mark.gpu

K = 3
N = MR.N_SAMPLES
_MODELS = {}


def _model(cuda, scale):
    if scale not in _MODELS:
        c = ER.case(scale)
        m = MNGP(scale, size=K, seed=3)
        with torch.no_grad():
            m.xyz_encoder.params.copy_(torch.from_numpy(c.table.astype(np.float32)).view(-1))
        _MODELS[scale] = m.to(cuda)
    return _MODELS[scale]


def _load(m, flats):
    """the next (up to) three weight sets into the model's sub-NeRFs"""
    p = np.zeros((K, MR.FIELD_PARAMS), np.float32)
    for k, f in enumerate(flats):
        p[k] = f
    with torch.no_grad():
        m.mlp_params.copy_(torch.from_numpy(p))


def _groups(sets):
    names = list(sets)
    for g in range(0, len(names), K):
        yield [(k, n, sets[n]) for k, n in enumerate(names[g:g + K])]


def _fail_at(tag, what, bad, got, ref, bound, name):
    i = tuple(int(v) for v in bad[0])
    pytest.fail(f"{tag}: {len(bad)} {what} outside the bar, first: {name(i)}: got {got[i]!r}, "
                f"reference {ref[i]!r}, bound {bound[i]!r}")


def _check(tag, what, got, ref, bound, name):
    """|got - ref| <= bound element by element (exactly equal where the bound
    is 0); returns the largest error / bound"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bad = np.argwhere(~(err <= bound))
    if len(bad):
        _fail_at(tag, what, bad, got, ref, bound, name)
    return float((err / np.where(bound > 0, bound, 1.0)).max())


def _forward_all(m, x, d, ind):
    """the three entry points on one input: (sigma, rgb, cache (n, 32) f16, geo (n, 16)) numpy"""
    n = len(x)
    sig, rgb = m(x, d, ind)
    feat = sig.grad_fn.feat
    with torch.no_grad():
        sig_ng, rgb_ng = m(x, d, ind)
        sig_d, geo = m.density(x, ind, return_feat=True)
        sig_o = m.density(x, ind)
    for name, a, b in (("no-grad forward sigma", sig_ng, sig), ("no-grad forward rgb", rgb_ng, rgb),
                       ("density(return_feat) sigma", sig_d, sig), ("density sigma", sig_o, sig)):
        if not torch.equal(a, b):
            i = int(torch.nonzero((a != b).reshape(n, -1).any(1))[0])
            pytest.fail(f"n {n} sub-NeRF {ind}: {name} differs from the grad-mode forward at sample {i}: "
                        f"{a[i].tolist()!r} vs {b[i].tolist()!r}")
    assert sig_ng.grad_fn is None
    return (sig.detach().cpu().numpy(), rgb.detach().cpu().numpy(),
            ER.decode_cache(feat.cpu().numpy(), n), geo.cpu().numpy(), feat)


def _check_forward(tag, f, sig, rgb, geo):
    gg = geo.astype(np.float64)
    bad = np.argwhere((gg < f.geo_lo) | (gg > f.geo_hi) | ~np.isfinite(gg))
    if len(bad):
        i, j = bad[0]
        pytest.fail(f"{tag}: {len(bad)} geo features outside the bar, first: sample {i} layer g2 row {j + 1}: "
                    f"stored {gg[i, j]!r}, reference {f.v_g[i, j + 1]!r} +- {f.a_g[i, j + 1]!r}, allowed "
                    f"[{f.geo_lo[i, j]!r}, {f.geo_hi[i, j]!r}]")
    r_s = _check(tag, "sigma", sig, f.sigma, f.sigma_bound, lambda i: f"sample {i[0]} layer g2 row 0 (g0 {f.g0[i[0]]!r})")
    r_c = _check(tag, "rgb", rgb, f.rgb, f.rgb_bound,
                 lambda i: f"sample {i[0]} layer r3 row {i[1]} (pre-activation {f.out[i]!r})")
    return r_s, r_c, float((gg != MR.rn16(f.v_g[:, 1:])).mean())


# ---------------------------------------------------------------------------
# (a)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_forward_per_activation(cuda, scale):
    """(a) rn_field_fwd (grad and no-grad mode) and rn_field_density at the
    first n of the adversarial positions, n in mlp_ref.COUNTS, and the full 600
    with a second set of directions.  The geo net is checked from the cache,
    the rgb net from [SH, the kernel's stored geo features].
    Measured on the MI355X (scale 0.5 / 16): sigma 0.48 / 0.31, rgb 0.49 / 0.48 of
    the bound; 5.2e-4 / 2.0e-3 of the geo features are the f16 neighbour of
    rn16(reference), none outside."""
    c, m = ER.case(scale), _model(cuda, scale)
    xt = torch.from_numpy(np.array(c.x[:N])).to(cuda)
    dirs = {s: MR.directions(N, s) for s in (0, 1)}
    worst = np.zeros(3)
    for group in _groups(MR.weight_sets()):
        _load(m, [flat for _, _, flat in group])
        for ind, name, flat in group:
            W = MR.split(flat)
            for n, dseed in [(n, 0) for n in MR.COUNTS] + [(N, 1)]:
                d = dirs[dseed][:n]
                sig, rgb, e16, geo, _ = _forward_all(m, xt[:n], torch.from_numpy(d).to(cuda), ind)
                f = MR.forward(e16, d, W, geo_given=geo)
                worst = np.maximum(worst, _check_forward(f"scale {scale} {name} n {n} directions {dseed}", f, sig, rgb, geo))
    print(f"forward scale {scale}: sigma {worst[0]:.3f}, rgb {worst[1]:.3f} of the bound; "
          f"geo features != rn16(ref) {worst[2]:.2e}")


# ---------------------------------------------------------------------------
# (b)
# ---------------------------------------------------------------------------
def test_sh_per_coefficient(cuda):
    """(b) With probe(shift) rgb_c = sigmoid(k relu(+-sh16_i)), k a signed power
    of two, so the f16 SH coefficient the kernel fed to the rgb net is
    logit(rgb_c) / k wherever that branch is live: it must lie in
    [rn16(Y - s), rn16(Y + s)] (exactly 0 where Y is exactly 0), cut by the
    relative interval of mlp_ref.sh_interval, which is what the reference
    assumes of the kernel's coefficient when it decides a mask.  logit of the
    fp32 rgb carries 2^-22 / (1 - y) + 2^-22 / y (sigmoidf's 4 ulp), so the
    recovered value is the interval x +- delta and has to meet the allowed
    one; two gains (1, 64) keep delta below half an f16 step for large and for
    small coefficients, and every (sample, coefficient) of f16-normal size
    must be recovered that sharply, on its sign's branch, by one of them.
    Where rgb_c == 0.5 exactly (the branch is dead, or |k sh16| < 2^-23, below
    which sigmoidf's expf rounds to 1) the allowed interval must hold such a
    value.  Directions: both sets of mlp_ref.directions (unit, long and short,
    axes, near-pole).
    Measured: 15 956 coefficients pinned to one f16 value, all inside the bar,
    458 of them the neighbour of rn16(Y)."""
    scale = 0.5
    c, m = ER.case(scale), _model(cuda, scale)
    xt = torch.from_numpy(np.array(c.x[:N])).to(cuda)
    sets = {(shift, gain): MR.probe(shift, rgb_gain=gain) for shift in MR.PROBE_SHIFTS for gain in (1.0, 64.0)}
    n_live = n_off = 0
    for dseed in (0, 1):
        d = MR.directions(N, dseed)
        dt = torch.from_numpy(d).to(cuda)
        Y, lo, hi = MR.sh_interval(d)          # the issue's interval cut by the relative one: never wider
        sharp = np.zeros((N, 16, 2), bool)
        for group in _groups(sets):
            _load(m, [flat for _, _, flat in group])
            for ind, (shift, gain), flat in group:
                with torch.no_grad():
                    _, rgb = m(xt, dt, ind)
                y = rgb.cpu().numpy().astype(np.float64)
                _, _, outs, mm = MR.probe_wiring(shift)
                for col, (u, sgn) in enumerate(outs):
                    i, neg = u % 16, u >= 32
                    k = sgn * gain * mm[u] * MR.probe_c(i) * (-1.0 if neg else 1.0)     # out = k sh16 where live
                    yc = y[:, col]
                    dead = yc == 0.5
                    # rgb is exactly 0.5 while |k sh16| < 2^-23 (expf rounds to 1) or the branch is dead:
                    # a value of +-sh16 that small, or <= 0, must be allowed
                    tiny = 2.0 ** -23 / abs(k)
                    bad = dead & ((-hi[:, i] > tiny) if neg else (lo[:, i] > tiny))
                    assert not bad.any(), (f"shift {shift} gain {gain} directions {dseed}: rgb {col} is 0.5 at sample "
                                           f"{int(np.flatnonzero(bad)[0])} but SH {i} cannot be {'>=' if neg else '<='} 0 or that small")
                    live = ~dead & (yc > 0) & (yc < 1)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        x = np.log(yc / (1 - yc)) / k
                        delta = (2.0 ** -22 / (1 - yc) + 2.0 ** -22 / yc) / abs(k)
                    with np.errstate(invalid="ignore"):
                        out = live & ((x + delta < lo[:, i]) | (x - delta > hi[:, i]))
                    if out.any():
                        j = int(np.flatnonzero(out)[0])
                        pytest.fail(f"shift {shift} gain {gain} directions {dseed}: SH coefficient {i} "
                                    f"({'-' if neg else '+'} branch, layer r1 row {u}) of sample {j} d={d[j].tolist()}: "
                                    f"recovered {x[j]!r} +- {delta[j]!r}, reference {Y[j, i]!r}, allowed "
                                    f"[{lo[j, i]!r}, {hi[j, i]!r}]")
                    xs = np.where(live, x, 0.0)
                    step = np.maximum(np.spacing(np.abs(xs).astype(np.float16)).astype(np.float64), 2.0 ** -24)
                    pinned = live & (delta < 0.5 * step)
                    sharp[:, i, int(neg)] |= pinned
                    n_live += int(pinned.sum())
                    n_off += int((pinned & (MR.rn16(xs) != MR.rn16(Y[:, i]))).sum())
        # every coefficient of every sample was pinned to one f16 value on the side it is non-zero
        need = np.stack([(lo > 0) & (Y >= 2.0 ** -14), (hi < 0) & (Y <= -2.0 ** -14)], 2)
        miss = np.argwhere(need & ~sharp)
        assert not len(miss), f"directions {dseed}: {len(miss)} (sample, coefficient) not recovered sharply, first {miss[0].tolist()}"
    print(f"SH: {n_live} coefficients pinned to one f16 value, all inside the bar; {n_off} of them the neighbour of rn16(Y)")


# ---------------------------------------------------------------------------
# (c), (d): the backward
# ---------------------------------------------------------------------------
def _bwd(m, x, d, ind, ds, dr, feat, blocks, grid=None):
    """rn_field_bwd as MNGP launches it; blocks=None: one block per 256-sample
    iteration (the module's choice at this size), 1: one block walks them all"""
    dw = torch.zeros_like(m.mlp_params)
    gg = torch.zeros_like(m.xyz_encoder.params) if grid is None else grid
    m._launch_field(False, x, d, ind, dsigma=ds, drgb=dr, grid_grad=gg, dw=dw, blocks=blocks, feat=feat)
    return dw.cpu().numpy(), gg


def _check_dw(tag, dw, ind, b):
    rest = np.delete(dw, ind, 0)
    assert np.all(rest == 0), f"{tag}: another sub-NeRF's MLP gradient is not exactly 0"
    return _check(tag, "dW elements", dw[ind], b.dW, b.dW_bound, lambda i: MR.where(i[0]))


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_dw_per_weight(cuda, scale):
    """(c) all 9472 dW elements of rn_field_bwd per sub-NeRF against the
    reference and its bound, dense and banded weights, every seed set of
    mlp_ref.seed_sets on the 600 samples (three iterations, the last ragged)
    with one block per iteration and with one block walking all three (the
    accumulators then persist and are rescaled between iterations), and
    N(0, 1) seeds at every prefix count.
    Measured, largest error / bound (scale 0.5 / 16): normal 0.41 / 0.35,
    dsigma_only 0.10 / 0.04, drgb_only and two_scales 0.41 / 0.35, zero_iter
    0.15 / 0.27, steps 0.44 / 0.46, its groups alone 0.14, 0.44, 0.27 / 0.26, 0.46,
    0.13, prefix counts 0.50 / 0.32 (0.50: an undecided ReLU mask, whose budget
    is exactly that unit's dY)."""
    c, m = ER.case(scale), _model(cuda, scale)
    xt = torch.from_numpy(np.array(c.x[:N])).to(cuda)
    d = MR.directions(N, 0)
    dt = torch.from_numpy(d).to(cuda)
    seeds = MR.seed_sets(N)
    worst = {}
    for group in _groups(MR.weight_sets()):
        _load(m, [flat for _, _, flat in group])
        for ind, name, flat in group:
            W = MR.split(flat)
            _, _, e16, geo, feat = _forward_all(m, xt, dt, ind)
            f = MR.forward(e16, d, W, geo_given=geo)
            for sname, (ds, dr) in seeds.items():
                b = MR.backward(f, W, ds, dr)
                dst, drt = torch.from_numpy(ds).to(cuda), torch.from_numpy(dr).to(cuda)
                for blocks in (None, 1):
                    dw, _ = _bwd(m, xt, dt, ind, dst, drt, feat, blocks)
                    r = _check_dw(f"scale {scale} {name} seeds {sname} blocks {blocks}", dw, ind, b)
                    worst[sname] = max(worst.get(sname, 0.0), r)
            ds, dr = seeds["normal"]
            for n in MR.COUNTS[:-1]:
                _, _, e16n, geon, featn = _forward_all(m, xt[:n], dt[:n], ind)
                fn = MR.forward(e16n, d[:n], W, geo_given=geon)
                b = MR.backward(fn, W, ds[:n], dr[:n])
                dw, _ = _bwd(m, xt[:n].contiguous(), dt[:n].contiguous(), ind, torch.from_numpy(ds[:n].copy()).to(cuda),
                             torch.from_numpy(dr[:n].copy()).to(cuda), featn, None)
                worst["prefix"] = max(worst.get("prefix", 0.0), _check_dw(f"scale {scale} {name} n {n}", dw, ind, b))
    print(f"dW scale {scale}, largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_dw_probe_saturated(cuda):
    """(c) probe weights with g0 beyond the TruncExp clamp (|g0| up to 36, both
    signs: sigma and the clamped backward) and with the rgb pre-activation up
    to +-48 (sigmoid' underflows in fp32).  dW per element within the
    reference's bound, which under probe weights (one term per dot product,
    powers of two: after the seed's rounding the chain is exact) is at most
    the tight (2^-9 + n 2^-23) sum |terms| of test_gpu_encode.py (c): measured
    0.07 of it in the median, 0.55 at most, for every element but 2 of 387 non-zero
    ones in the rgb- set, whose dY is an f16 subnormal at the block's scale (2^-25 / G
    on a column whose sum |terms| is tiny: 34 times the tight bound, 0.066 of
    sum |terms|).  Asserted here and, for both direction sets, in
    tests/test_mlp_ref.py::test_probe_bound_is_tight.  An element whose reference and bound are exactly zero (a row whose unit no
    output reads, a column whose unit is dead) must be exactly zero.
    Measured: largest error / bound 0.17; 45 112 elements exactly 0."""
    scale = 0.5
    c, m = ER.case(scale), _model(cuda, scale)
    xt = torch.from_numpy(np.array(c.x[:N])).to(cuda)
    d = MR.directions(N, 0)
    dt = torch.from_numpy(d).to(cuda)
    ds, dr = MR.seed_sets(N)["normal"]
    dst, drt = torch.from_numpy(ds).to(cuda), torch.from_numpy(dr).to(cuda)
    sets = MR.probe_saturated_sets()
    worst, zeros = 0.0, 0
    for group in _groups(sets):
        _load(m, [flat for _, _, flat in group])
        for ind, name, flat in group:
            W = MR.split(flat)
            sig, rgb, e16, geo, feat = _forward_all(m, xt, dt, ind)
            f = MR.forward(e16, d, W, geo_given=geo)
            if name[:2] == "g0":
                hot = f.g0 > 15 if name == "g0+" else f.g0 < -15
                assert hot.sum() >= 10 and np.abs(f.g0).max() < 80
            if name[:3] == "rgb":
                assert (np.abs(f.out) > 30).sum() >= 10
            _check_forward(f"probe {name}", f, sig, rgb, geo)
            b = MR.backward(f, W, ds, dr)
            # never looser than the tight bound plus the subnormal floor (see the docstring)
            tight = MR.probe_tight(b, N)
            over = b.dW_bound > tight
            assert over.sum() <= 1e-2 * (b.dW_mag > 0).sum() and np.all(b.dW_bound[over] <= 0.25 * b.dW_mag[over])
            zeros += int(((b.dW == 0) & (b.dW_bound == 0)).sum())
            for blocks in (None, 1):
                dw, _ = _bwd(m, xt, dt, ind, dst, drt, feat, blocks)
                worst = max(worst, _check_dw(f"probe {name} blocks {blocks}", dw, ind, b))
    print(f"dW probe: largest error / bound {worst:.3f}; {zeros} elements required to be exactly 0")


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_grid_and_input_gradients_live_mlp(cuda, scale):
    """(d) With a live MLP (dense, banded 1 and 6) the reference's dL/dencoding
    and dL/dSH, with their bounds, replace the known ones of test_gpu_encode.py
    (c) and (d).  Grid gradient of rn_field_bwd per entry:
    |g - sum w dE| <= sum w bound(dE) + n_e 2^-23 sum |w dE|, entries no sample
    touches exactly 0.  rn_field_dinput (per-tile scales: the reference runs
    with groups of 32): dL/dxyz per sample and axis within
    sum_j bound(dE_j) |D_j| + 2^-17 sum_j |dE_j| A_j (the re-gather's 48 fp32
    operations, doubled), exactly 0 on clipped axes; dL/ddir within the same
    form through the SH Jacobian and the projection (g - q (q.g)) / |d|
    (2^-17 of the terms' magnitudes for the fp32 Jacobian and projection).
    Measured (scale 0.5 / 16): grid gradient 0.50 / 0.49, dL/dxyz 0.14 / 0.17,
    dL/ddir 0.48 / 0.48 of the bound."""
    c, m = ER.case(scale), _model(cuda, scale)
    x = np.array(c.x[:N])
    d = MR.directions(N, 0)
    ds, dr = MR.seed_sets(N)["normal"]
    D, A = ER.dencode_dx_cells(c.cells, c.table)
    D, A = D[:N], A[:N]
    clipped = ((c.cells.v < 0) | (c.cells.v > 1))[:N]
    sets = {"dense": MR.dense(), "banded1": MR.banded(1), "banded6": MR.banded(6)}
    _load(m, list(sets.values()))
    worst = np.zeros(3)
    for ind, (name, flat) in enumerate(sets.items()):
        W = MR.split(flat)
        tag = f"scale {scale} {name}"
        m.zero_grad()
        xt = torch.from_numpy(x).to(cuda).requires_grad_(True)
        dt = torch.from_numpy(d).to(cuda).requires_grad_(True)
        sig, rgb = m(xt, dt, ind)
        e16 = ER.decode_cache(sig.grad_fn.feat.cpu().numpy(), N)
        with torch.no_grad():
            _, geo = m.density(xt, ind, return_feat=True)
        torch.autograd.backward([sig, rgb], [torch.from_numpy(ds).to(cuda), torch.from_numpy(dr).to(cuda)])
        f = MR.forward(e16, d, W, geo_given=geo.cpu().numpy())
        # grid gradient: block scales of 256
        b = MR.backward(f, W, ds, dr)
        g = m.xyz_encoder.params.grad.view(-1, 2)
        ent, ref, ab, cnt = ER.grid_grad_entries(c.cells, _pad(b.dE, len(c.x)), N)
        _, _, eb, _ = ER.grid_grad_entries(c.cells, _pad(b.dE_bound, len(c.x)), N)
        ent_t = torch.from_numpy(ent).to(cuda)
        got = g[ent_t].double().cpu().numpy()
        rest = g.clone()
        rest[ent_t] = 0
        assert not bool(rest.any()), f"{tag}: entries that no sample touches are non-zero"
        lv = c.lv
        worst[0] = max(worst[0], _check(tag, "grid gradient elements", got, ref, eb + (cnt * 2.0 ** -23)[:, None] * ab,
                                        lambda i: f"entry {int(ent[i[0]])} (level {int(np.searchsorted(lv['offset'], ent[i[0]], side='right') - 1)}) feature {i[1]}, {int(cnt[i[0]])} contributions"))
        # input gradients: per-tile scales
        bt = MR.backward(f, W, ds, dr, group=32)
        dx = xt.grad.cpu().numpy()
        assert np.all(dx[clipped] == 0), f"{tag}: gradient on a clipped axis"
        ref = (bt.dE[:, :, None] * D).sum(1)
        bound = (bt.dE_bound[:, :, None] * np.abs(D)).sum(1) + 2.0 ** -17 * (np.abs(bt.dE)[:, :, None] * A).sum(1)
        worst[1] = max(worst[1], _check(tag, "dL/dxyz components", dx, ref, bound,
                                        lambda i: f"sample {i[0]} x={x[i[0]].tolist()} axis {i[1]}"))
        J = MR.sh4_jac(f.q)                                        # (n, 16, 3)
        gq = (bt.dSH[:, :, None] * J).sum(1)
        bq = (bt.dSH_bound[:, :, None] * np.abs(J)).sum(1) + 2.0 ** -17 * (np.abs(bt.dSH)[:, :, None] * np.abs(J)).sum(1)
        q, nrm = f.q, f.dnorm[:, None]
        ref = (gq - q * (q * gq).sum(1, keepdims=True)) / nrm
        mag = np.abs(gq) + np.abs(q) * (np.abs(q) * np.abs(gq)).sum(1, keepdims=True)
        bound = (bq + np.abs(q) * (np.abs(q) * bq).sum(1, keepdims=True) + 2.0 ** -17 * mag) / nrm
        worst[2] = max(worst[2], _check(tag, "dL/ddir components", dt.grad.cpu().numpy(), ref, bound,
                                        lambda i: f"sample {i[0]} d={d[i[0]].tolist()} axis {i[1]}"))
    print(f"live MLP scale {scale}, largest error / bound: grid gradient {worst[0]:.3f}, dL/dxyz {worst[1]:.3f}, "
          f"dL/ddir {worst[2]:.3f}")


def _pad(a, n):
    out = np.zeros((n,) + a.shape[1:])
    out[:len(a)] = a
    return out


# ---------------------------------------------------------------------------
# (e), (f): the production chain on axis-aligned lattice rays
# ---------------------------------------------------------------------------
def _chain_scene(cuda, scale, flats):
    from radnerf_amd import layout as LY
    from radnerf_amd import synthetic as S
    from radnerf_amd.networks import Ray_Gate
    m = MNGP(scale, size=K, seed=3)
    g = Ray_Gate(K, seed=2)
    c = ER.case(scale)
    bits = S.bitfields(K, m.cascades, p=0.25)
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(c.table.astype(np.float32)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(np.stack(flats)))
        g.params.copy_(torch.from_numpy(S.mlp_params(1, LY.gate_params(K), seed=6)[0]))
    S.set_bitfields(m, bits)
    o, d = ER.lattice_rays(scale, c.lv)
    return m.to(cuda), g.to(cuda), o, d, S.noise(K, len(o)), S.loss_seeds(len(o), K)


def _ws_samples(w):
    """per sub-NeRF the workspace slots of its samples, in ray order, and their rays"""
    off, cnt = w.offsets.cpu().numpy(), w.counts.cpu().numpy()
    ray_of = w.ray_of.cpu().numpy()
    out = []
    for k in range(cnt.shape[0]):
        idx = np.concatenate([np.arange(off[k, r], off[k, r] + cnt[k, r]) for r in range(cnt.shape[1])]).astype(np.int64)
        out.append((idx, ray_of[idx]))
    return out


_SWITCHES = ("merged_fwd", "merged_encode", "level_fwd", "merged_bwd", "grid_fx", "grid_bin", "bin_f32_levels")
CHAIN_SETS = ("dense", "banded3", "banded6")


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_production_chain(cuda, scale):
    """(e) 24 axis-aligned lattice rays (encode_ref.lattice_rays) through
    ml_render_fused with a dense and two banded MLPs on the three sub-NeRFs.
    rgb, sigma and the encoding cache are bit-identical between
    rn_field_fwd_levels (the default), rn_field_fwd_merged and the per-model
    rn_field_fwd: the first time with an rgb that is not the constant 0.5.
    sigma and rgb are within bound (a) at the workspace's samples (the geo
    features are not stored there: the rgb net's bound runs from the cache,
    five layers).  The MLP gradient is checked per element for
    rn_field_bwd_merged with fp32 atomics (the default here), with the
    fixed-point grid scatter, and for rn_field_bwd_merged_det +
    rn_reduce_partials (deterministic=True); the reference takes the
    workspace's dsigma / drgb as given, and since the plan decides which
    samples share a block, the f16 subnormal floor is 2^-28 M, M the step's
    largest seed (mlp_ref.backward, floor=).
    Measured (scale 0.5 / 16): sigma 0.38 / 0.35, rgb 0.48 / 0.38 of the bound; dW
    0.004 / 0.012 in all three modes (the floor term dominates the bound)."""
    from radnerf_amd.fused import ml_render_fused, get_renderer
    sets = MR.weight_sets()
    flats = [sets[n] for n in CHAIN_SETS]
    m, g, o, d, noise, seeds = _chain_scene(cuda, scale, flats)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    esf = 1 / 256 if scale > 0.5 else 0.0
    render = lambda **kw: ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise), exp_step_factor=esf, **kw)
    r = get_renderer(m, g, len(o))
    saved = {k: getattr(r, k) for k in _SWITCHES}
    assert saved["level_fwd"] and saved["merged_fwd"] and saved["merged_bwd"]
    outs = []
    try:
        for merged, enc, lvf in ((saved["merged_fwd"], saved["merged_encode"], True), (True, True, False),
                                 (False, False, False)):
            r.merged_fwd, r.merged_encode, r.level_fwd = merged, enc, lvf
            render()
            w = r.ws
            smp = _ws_samples(w)
            top = max(int(idx.max()) for idx, _ in smp) + 1
            feat = ER.decode_cache(w.feat[:(top + 31) // 32 * 32].cpu().numpy(), top)
            sigma, rgb = w.sigma[:top].cpu().numpy(), w.rgb[:top].cpu().numpy().reshape(top, 3)
            outs.append([(feat[idx], sigma[idx], rgb[idx]) for idx, _ in smp])
    finally:
        for k, v in saved.items():
            setattr(r, k, v)
    worst = np.zeros(2)
    fwd = []
    for k in range(K):
        idx, rays = smp[k]
        assert len(idx) >= 500
        for name, other in zip(("merged", "per-model"), (outs[1][k], outs[2][k])):
            for what, a, b in zip(("cache", "sigma", "rgb"), other, outs[0][k]):
                assert np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32),
                                      b.view(np.uint16 if a.dtype == np.float16 else np.uint32)), \
                    f"scale {scale} sub-NeRF {k}: {what} of the {name} forward not bit-identical to the level forward"
        e16, sigma, rgb = outs[0][k]
        assert np.abs(rgb - 0.5).max() > 0.05
        f = MR.forward(e16, d[rays], MR.split(flats[k]))
        tag = f"scale {scale} chain sub-NeRF {k} ({CHAIN_SETS[k]})"
        worst[0] = max(worst[0], _check(tag, "sigma", sigma, f.sigma, f.sigma_bound, lambda i: f"sample {i[0]} ray {rays[i[0]]}"))
        worst[1] = max(worst[1], _check(tag, "rgb", rgb, f.rgb, f.rgb_bound, lambda i: f"sample {i[0]} ray {rays[i[0]]} layer r3 row {i[1]}"))
        fwd.append(f)

    def grads(rr, **kw):
        m.zero_grad(); g.zero_grad()
        res = render(**kw)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], [to(s) for s in seeds])
        w = rr.ws
        ds, dr = w.dsigma.cpu().numpy(), w.drgb.cpu().numpy().reshape(-1, 3)
        return m.mlp_params.grad.cpu().numpy().copy(), [(ds[idx], dr[idx]) for idx, _ in _ws_samples(w)]

    def check(tag, dw, sd):
        M = max(max(np.abs(s.astype(np.float64) * f.sigma).max(), 0.25 * np.abs(t).max()) for (s, t), f in zip(sd, fwd))
        worst_r = 0.0
        for k in range(K):
            b = MR.backward(fwd[k], MR.split(flats[k]), sd[k][0], sd[k][1], floor=2.0 ** -28 * M)
            worst_r = max(worst_r, _check(f"{tag} sub-NeRF {k} ({CHAIN_SETS[k]})", "dW elements", dw[k], b.dW, b.dW_bound,
                                          lambda i: MR.where(i[0])))
        return worst_r

    report = {}
    try:
        assert r.scatter_mode == "fp32-atomics"
        report["fp32 atomics"] = check(f"scale {scale} merged fp32", *grads(r))
        r.grid_fx = True
        grads(r)                                   # a workspace's first such backward runs fp32 and sets the scales
        report[r.scatter_mode] = check(f"scale {scale} merged {r.scatter_mode}", *grads(r))
    finally:
        for k, v in saved.items():
            setattr(r, k, v)
    rd = get_renderer(m, g, len(o), deterministic=True)
    assert rd.deterministic and rd is not r
    report["deterministic"] = check(f"scale {scale} deterministic", *grads(rd, deterministic=True))
    print(f"chain scale {scale}: {[len(i) for i, _ in smp]} samples; sigma {worst[0]:.3f}, rgb {worst[1]:.3f} of the bound; "
          "dW largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))


def test_scale_equivariance(cuda):
    """(f) deterministic=True, the loss seeds multiplied by 2^k, k in {-40, -8,
    8}: every MLP gradient element and every grid gradient entry is bitwise
    2^k times the unscaled run's, because every gradient scale in the chain is
    a power of two taken from the seeds.  This holds while nothing leaves the
    fp32 normal range; checked here on the unscaled gradients: the smallest
    non-zero magnitude times 2^-40 and the largest times 2^8 stay inside.  The
    CPU check on the reference's seeds, dY, scaled dY and dW for these k is
    tests/test_mlp_ref.py::test_scale_equivariance_stays_in_fp32_range."""
    from radnerf_amd.fused import ml_render_fused
    scale = 0.5
    sets = MR.weight_sets()
    m, g, o, d, noise, seeds = _chain_scene(cuda, scale, [sets[n] for n in CHAIN_SETS])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)

    def grads(k):
        m.zero_grad(); g.zero_grad()
        res = ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise), deterministic=True)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], [to(s * np.float32(2.0 ** k)) for s in seeds])
        return m.mlp_params.grad.clone(), m.xyz_encoder.params.grad.clone()

    base = grads(0)
    again = grads(0)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    for t in base:
        nz = t[t != 0].abs()
        assert float(nz.min()) * 2.0 ** -40 > 2.0 ** -100 and float(nz.max()) * 2.0 ** 8 < 2.0 ** 100 and len(nz) > 1000
    for k in (-40, -8, 8):
        got = grads(k)
        for name, a, b in zip(("MLP gradient", "grid gradient"), got, base):
            want = b * 2.0 ** k
            if not torch.equal(a, want):
                bad = torch.nonzero((a != want).reshape(-1))
                i = int(bad[0])
                where = MR.where(i % MR.FIELD_PARAMS) + f" sub-NeRF {i // MR.FIELD_PARAMS}" if name[0] == "M" else f"element {i}"
                pytest.fail(f"k {k}: {len(bad)} elements of the {name} are not 2^k times the unscaled run's, first: "
                            f"{where}: {float(a.reshape(-1)[i])!r} vs {float(want.reshape(-1)[i])!r}")
    print("scale equivariance: MLP and grid gradients bitwise 2^k times the unscaled run for k = -40, -8, 8")
