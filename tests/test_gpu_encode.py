"""The hash-grid encoding and its gradients, per feature / entry / sample,
against the fp64 reference tests/encode_ref.py at the positions where the
encode kernels have special cases (box faces, lattice planes and their one-ulp
neighbours, the dense levels' index wrap, runs of samples on one corner).

A field MLP with known dL/dfeature (encode_ref.transparent_mlp) makes the
grid and input gradients a function of the encoding alone.  Bars, derived
(DESIGN.md §2), with the measured maxima beside them in each test:

  (a) stored f16 feature in [rn16(ref - s), rn16(ref + s)], s = 2^-20 max|table|
  (b) sigma bit-identical between the entry points; vs exp(sum a_j e16_j) 2^-10
  (c) per entry |g - ref| <= (2^-9 + n_e 2^-23) A_e, untouched entries exactly 0
  (d) per sample and axis |dx - ref| <= 2^-9 sum_j |a_j dsigma sigma| sum|terms|
  (e) (a), (b) for the three production forwards on axis-aligned lattice rays
  (f) (c) for the production backward in each of its gradient modes
"""
import numpy as np
import pytest
import torch

import oracle
from oracle import field_oracle as fo
from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd import vren
from radnerf_amd.fused import ml_render_fused, get_renderer
from radnerf_amd.networks import MNGP, Ray_Gate

import encode_ref as ER

pytestmark = pytest.mark.gpu

SCALES = [0.5, 1.0, 4.0, 16.0]
K = 2
_MODELS = {}


def _model(cuda, scale):
    """As test_gpu_field._model (table synthetic.grid_params, amplitude 0.1)
    with the transparent MLPs; one per scale, shared and never modified."""
    if scale not in _MODELS:
        c = ER.case(scale)
        m = MNGP(scale, size=K, seed=3)
        assert m.xyz_encoder.n_entries == int(c.lv["n_entries"])
        with torch.no_grad():
            m.xyz_encoder.params.copy_(torch.from_numpy(c.table.astype(np.float32)).view(-1))
            m.mlp_params.copy_(torch.from_numpy(ER.transparent_mlp(K, ER.transparent_a(K))))
        _MODELS[scale] = m.to(cuda)
    return _MODELS[scale]


def _dirs(n, cuda):
    d = torch.zeros(n, 3, device=cuda)
    d[:, 0] = 1.0
    return d


def _where(c, i, j):
    """names sample i, feature column j of case c"""
    l, f = divmod(int(j), 2)
    return (f"sample {int(i)} x={c.x[i].tolist()} u={c.cells.u[i].tolist()} level {l} "
            f"({'dense' if ER.is_dense(c.lv, l) else 'hashed'}) feature {f} "
            f"cell fraction {c.cells.f[i, l].tolist()}")


def _check_features(got16, e, table, tag, where):
    """bar (a): got16 (n, 32) f16 against the fp64 features e.  Returns the
    share of the features stored as the f16 neighbour of rn16(ref) (the bar
    allows it only where ref is within s of the tie between the two)."""
    s = 2.0 ** -20 * float(np.abs(table.astype(np.float64)).max())
    got = got16.astype(np.float64)
    lo, hi = ER.rn16(e - s), ER.rn16(e + s)
    bad = np.argwhere((got < lo) | (got > hi) | ~np.isfinite(got))
    if len(bad):
        i, j = bad[0]
        pytest.fail(f"{tag}: {len(bad)} features outside the bar, first: {where(i, j)}: "
                    f"stored {got[i, j]!r}, reference {e[i, j]!r}, allowed [{lo[i, j]!r}, {hi[i, j]!r}]")
    return float((got != ER.rn16(e)).mean())


def _entry_name(lv, ent):
    l = int(np.searchsorted(lv["offset"], ent, side="right") - 1)
    return f"entry {int(ent)} = level {l} ({'dense' if ER.is_dense(lv, l) else 'hashed'}) index {int(ent - lv['offset'][l])}"


def _check_grid_grad(g, lv, ent, ref, ab, cnt, excl, tag, extra=None):
    """bar (c) on the device gradient g (entries, 2): every entry the reference
    does not touch is exactly 0.0; every touched entry outside excl is within
    (2^-9 + n_e 2^-23) A_e (+ extra (M, 2), a format's own rounding).  Returns
    (largest error / bound, entries excluded)."""
    ent_t = torch.from_numpy(ent).to(g.device)
    got = g[ent_t].double().cpu().numpy()
    rest = g.clone()
    rest[ent_t] = 0
    stray = torch.nonzero(rest.abs().sum(1))
    if len(stray):
        s = int(stray[0])
        pytest.fail(f"{tag}: {len(stray)} entries that no sample touches are non-zero, first: "
                    f"{_entry_name(lv, s)} = {rest[s].tolist()}")
    bound = (2.0 ** -9 + cnt * 2.0 ** -23)[:, None] * ab
    keep = ~np.isin(ent, excl)
    assert (~keep).sum() <= 1e-3 * len(ent), f"{tag}: {(~keep).sum()} of {len(ent)} entries excluded"
    err = np.abs(got - ref)
    if extra is not None:
        # measured only: what bar (c) without the format's term would give
        over = (~(err <= bound)) & keep[:, None]
        r0 = (err / np.where(bound > 0, bound, 1.0))[over]
        print(f"{tag}: without the added term {int(over.sum())} of {2 * int(keep.sum())} elements "
              f"exceed (c), largest {r0.max() if len(r0) else 0.0:.2f}x")
        bound = bound + extra
    bad = np.argwhere((~(err <= bound)) & keep[:, None])
    if len(bad):
        i, f = bad[0]
        pytest.fail(f"{tag}: {len(bad)} gradient elements outside the bar, first: "
                    f"{_entry_name(lv, ent[i])} feature {f}: got {got[i, f]!r}, reference {ref[i, f]!r}, "
                    f"bound {bound[i, f]!r}, {int(cnt[i])} contributions")
    ratio = err / np.where(bound > 0, bound, 1.0)
    return float(ratio[keep].max()), int((~keep).sum())


# ---------------------------------------------------------------------------
# (a), (b): forward of the per-model kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_encoding_per_feature(cuda, scale):
    """(a) rn_field_fwd's encoding cache, decoded, against encode() at every
    adversarial and sequence position, for the full set and each prefix count;
    nothing excluded, rows past n not compared.
    Measured: up to 2.5e-4 of the stored features are the f16 neighbour of
    rn16(ref) (ties within s), none outside the bar."""
    c, m = ER.case(scale), _model(cuda, scale)
    xt = torch.from_numpy(np.array(c.x)).to(cuda)
    worst = 0.0
    for n in (len(c.x),) + ER.PREFIXES:
        sig, _ = m(xt[:n], _dirs(n, cuda), 1)
        feat = sig.grad_fn.feat
        assert feat is not None and feat.shape == ((n + 31) // 32 * 32, 32)
        got = ER.decode_cache(feat.cpu().numpy(), n)
        worst = max(worst, _check_features(got, c.e[:n], c.table, f"scale {scale} n {n}",
                                           lambda i, j: _where(c, i, j)))
    print(f"encoding scale {scale}: largest share of features != rn16(ref) {worst:.2e}")


@pytest.mark.parametrize("scale", SCALES)
def test_entry_points_agree(cuda, scale):
    """(b) sigma of MNGP.density (rn_field_density) and of a no-grad forward
    bit-identical to the grad-mode forward's at every position and prefix
    count, for both sub-NeRFs; and sigma against exp(sum a_j e16_j), relative
    2^-10 (an f16 tie of one feature flipping: <= 2^-12 each way; the 64-term
    fp32 dot product and expf: below 2^-16).
    Measured: largest relative error / 2^-10 = 0.03-0.13."""
    c, m = ER.case(scale), _model(cuda, scale)
    xt = torch.from_numpy(np.array(c.x)).to(cuda)
    a = ER.transparent_a(K)
    worst = 0.0
    for ind in range(K):
        ref = ER.transparent_sigma(c.e, a[ind])
        for n in (len(c.x),) + ER.PREFIXES:
            x, d = xt[:n], _dirs(n, cuda)
            sig, rgb = m(x, d, ind)
            with torch.no_grad():
                sig_ng, _ = m(x, d, ind)
                sig_d = m.density(x, ind)
                sig_f, _ = m.density(x, ind, return_feat=True)
            for name, other in (("no-grad forward", sig_ng), ("density", sig_d),
                                ("density(return_feat)", sig_f)):
                if not torch.equal(other, sig):
                    i = int(torch.nonzero(other != sig)[0])
                    pytest.fail(f"scale {scale} sub-NeRF {ind} n {n}: {name} sigma differs from the "
                                f"grad-mode forward at sample {i} x={c.x[i].tolist()}: "
                                f"{float(other[i])!r} vs {float(sig[i])!r}")
            assert sig_ng.grad_fn is None
            rel = np.abs(sig.detach().cpu().numpy().astype(np.float64) - ref[:n]) / ref[:n]
            i = int(np.argmax(rel))
            assert rel[i] <= 2.0 ** -10, (f"scale {scale} sub-NeRF {ind} n {n}: sigma of sample {i} "
                                          f"x={c.x[i].tolist()} off by {rel[i]:.3e} relative")
            worst = max(worst, float(rel[i]))
            assert torch.allclose(rgb, torch.full_like(rgb, 0.5), atol=1e-6, rtol=0)
    print(f"sigma scale {scale}: largest relative error / 2^-10 = {worst * 1024:.3f}")


# ---------------------------------------------------------------------------
# (c), (d): backward of the per-model kernels
# ---------------------------------------------------------------------------
def _backward(cuda, c, m, sl, ind=1):
    """forward + backward of the samples c.x[sl] with the seeds dsigma_seeds,
    drgb = 0.  Returns (grid gradient (entries, 2) on the device, dL/dxyz
    numpy, reference dL/dfeature (N, 32; rows outside sl unused))."""
    a = ER.transparent_a(K)[ind]
    sig_ref = ER.transparent_sigma(c.e, a)
    ds = ER.dsigma_seeds(sig_ref, seed=5)
    m.zero_grad()
    xt = torch.from_numpy(np.array(c.x[sl])).to(cuda).requires_grad_(True)
    sig, rgb = m(xt, _dirs(len(xt), cuda), ind)
    sig.backward(torch.from_numpy(ds[sl]).to(cuda))
    assert m.mlp_params.grad[1 - ind].abs().max() == 0          # the other sub-NeRF's MLP
    assert m.mlp_params.grad[ind].abs().max() > 0
    dfeat = a[None, :] * (ds.astype(np.float64) * sig_ref)[:, None] * (ER.rn16(c.e) != 0)
    return m.xyz_encoder.params.grad.view(-1, 2), xt.grad.cpu().numpy(), dfeat


@pytest.mark.parametrize("scale", SCALES)
def test_grid_gradient_per_entry(cuda, scale):
    """(c) rn_field_bwd's grid gradient per entry, for the adversarial set,
    the ordered sequences (order kept) and every prefix count:
    |g - ref| <= (2^-9 + n_e 2^-23) A_e with ref = sum w dfeat, A_e = sum |w dfeat|
    and n_e the contributions.  2^-9 is twice the budget 2^-11 (the one f16
    rounding of the scaled seed) + 2^-12 (sigma: f16 ties of the features) +
    fp32 slack; n_e 2^-23 covers the fp32 atomic sum in any order.  Entries no
    sample touches are exactly 0.0.  Entries fed by a feature within 2^-20 of
    zero (ReLU' at an f16 zero) are excluded, at most 0.1 % of the touched.
    Measured: largest error / bound 0.240-0.243 at every scale (2^-11 / 2^-9:
    the seed's f16 rounding)."""
    c, m = ER.case(scale), _model(cuda, scale)
    worst = 0.0
    for name, sl in c.runs.items():
        g, _, dfeat = _backward(cuda, c, m, sl)
        ent, ref, ab, cnt = ER.grid_grad_entries(c.cells, dfeat, sl)
        ratio, n_ex = _check_grid_grad(g, c.lv, ent, ref, ab, cnt,
                                       ER.doubtful_entries(c.cells, c.e, sl), f"scale {scale} {name}")
        worst = max(worst, ratio)
    print(f"grid gradient scale {scale}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("scale", SCALES)
def test_input_gradient_per_sample(cuda, scale):
    """(d) rn_field_dinput's dL/dxyz per sample and axis on the same runs:
    |dx - ref| <= 2^-9 sum_j |a_j dsigma sigma| sum_corners |term|, ref =
    sum_j a_j dsigma sigma dencode_dx (right-sided at a lattice plane), and
    exactly zero on every axis whose unit coordinate was clipped (a sample on
    a face from inside is not).  Samples with a feature within 2^-20 of zero
    are left out, as in (c).
    Measured: largest error / bound 0.11-0.14."""
    c, m = ER.case(scale), _model(cuda, scale)
    D, A = ER.dencode_dx_cells(c.cells, c.table)
    clipped = (c.cells.v < 0) | (c.cells.v > 1)
    sure = ~ER.doubtful(c.e).any(1)
    assert (~sure).sum() <= 5e-3 * len(sure)
    worst = 0.0
    for name, sl in c.runs.items():
        _, dx, dfeat = _backward(cuda, c, m, sl)
        ref = (dfeat[sl, :, None] * D[sl]).sum(1)
        bound = 2.0 ** -9 * (np.abs(dfeat[sl])[:, :, None] * A[sl]).sum(1)
        assert np.all(dx[clipped[sl]] == 0), f"scale {scale} {name}: gradient on a clipped axis"
        err = np.abs(dx.astype(np.float64) - ref)
        bad = np.argwhere(~(err <= bound) & sure[sl][:, None])
        if len(bad):
            i, ax = bad[0]
            gi = i + sl.start
            pytest.fail(f"scale {scale} {name}: {len(bad)} components outside the bar, first: sample "
                        f"{gi} x={c.x[gi].tolist()} u={c.cells.u[gi].tolist()} axis {ax}: got "
                        f"{dx[i, ax]!r}, reference {ref[i, ax]!r}, bound {bound[i, ax]!r}")
        worst = max(worst, float((err / np.where(bound > 0, bound, 1.0))[sure[sl]].max()))
    print(f"input gradient scale {scale}: largest error / bound {worst:.3f}")


# ---------------------------------------------------------------------------
# (e), (f): the production chain on axis-aligned lattice rays
# ---------------------------------------------------------------------------
def _scene(cuda, scale):
    lv = fo.grid_levels(scale)
    m = MNGP(scale, size=K, seed=3)
    g = Ray_Gate(K, seed=2)
    table = S.grid_params(m.xyz_encoder.n_entries).astype(np.float16)
    bits = S.bitfields(K, m.cascades, p=0.25)
    with torch.no_grad():
        m.xyz_encoder.params.copy_(torch.from_numpy(table.astype(np.float32)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(ER.transparent_mlp(K, ER.transparent_a(K))))
        g.params.copy_(torch.from_numpy(S.mlp_params(1, LY.gate_params(K), seed=6)[0]))
    S.set_bitfields(m, bits)
    o, d = ER.lattice_rays(scale, lv)
    return lv, m.to(cuda), g.to(cuda), table, bits, o, d, S.noise(K, len(o))


def _fma32(t, d, o):
    """fp32 fma(t, d, o) through fp64 (load_sample<1>, csrc/rn_field.h)"""
    return (t.astype(np.float64)[:, None] * d.astype(np.float64) + o.astype(np.float64)).astype(np.float32)


def _samples(w, o, d):
    """Per sub-NeRF: (slot indices, positions) of the workspace's samples, in
    ray order, from ws.offsets / ws.counts / ws.ts / ws.ray_of."""
    off, cnt = w.offsets.cpu().numpy(), w.counts.cpu().numpy()
    ts, ray_of = w.ts.cpu().numpy(), w.ray_of.cpu().numpy()
    out = []
    for k in range(cnt.shape[0]):
        idx = np.concatenate([np.arange(off[k, r], off[k, r] + cnt[k, r]) for r in range(cnt.shape[1])])
        idx = idx.astype(np.int64)
        r = ray_of[idx]
        assert np.array_equal(r, np.repeat(np.arange(cnt.shape[1]), cnt[k]))
        out.append((idx, _fma32(ts[idx], d[r], o[r])))
    return out, cnt, off, ts


def _switches(r):
    return dict(merged_fwd=r.merged_fwd, merged_encode=r.merged_encode, level_fwd=r.level_fwd,
                merged_bwd=r.merged_bwd, grid_fx=r.grid_fx, grid_bin=r.grid_bin,
                bin_f32_levels=r.bin_f32_levels)


def _restore(r, saved):
    for k, v in saved.items():
        setattr(r, k, v)


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_production_forward_on_lattice_rays(cuda, scale):
    """(e) rn_field_fwd_levels (the default), rn_field_fwd_merged and
    rn_field_fwd inside ml_render_fused on 24 axis-aligned rays whose off-axis
    coordinates sit on lattice planes or one ulp off them.  First the box
    intersection and the march bit for bit against the oracle (no other test
    feeds a zero direction component); then ws.feat against bar (a) and
    ws.sigma against bar (b) at x = fma(t, d, o), per sub-NeRF with its own a;
    and the three forwards bit-identical to each other.
    Measured (scale 0.5 / 16): features stored as the f16 neighbour of
    rn16(ref) 1.8e-4 / 3.0e-4, none outside; sigma error / 2^-10 0.03 / 0.06."""
    lv, m, g, table, bits, o, d, noise = _scene(cuda, scale)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    esf = 1 / 256 if scale > 0.5 else 0.0
    ctr, half = np.zeros((1, 3), np.float32), np.full((1, 3), scale, np.float32)
    cnt_g, ht_g, hi_g = vren.ray_aabb_intersect(to(o), to(d), to(ctr), to(half), 1)
    cnt_o, ht_o, hi_o = oracle.ray_aabb_intersect(o, d, ctr, half, 1)
    assert np.all(cnt_o == 1)
    assert np.array_equal(cnt_g.cpu().numpy(), cnt_o) and np.array_equal(hi_g.cpu().numpy(), hi_o)
    assert np.array_equal(ht_g.cpu().numpy().view(np.uint32), ht_o.view(np.uint32))
    cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)
    ocnt, ostart, oxyz, ots, _, total = oracle.ml_march(o, d, np.zeros(3, np.float32),
                                                        np.full(3, scale, np.float32), noise, bits,
                                                        cascades, scale, esf)
    r = get_renderer(m, g, len(o))
    saved = _switches(r)
    a = ER.transparent_a(K)
    mn, ext = np.full(3, -scale, np.float32), np.full(3, 2 * scale, np.float32)
    outs = []
    try:
        # the default switches (level forward), the merged forward alone, the per-model forward
        for merged, enc, lvf in ((saved["merged_fwd"], saved["merged_encode"], saved["level_fwd"]),
                                 (True, True, False), (False, False, False)):
            r.merged_fwd, r.merged_encode, r.level_fwd = merged, enc, lvf
            ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise), exp_step_factor=esf)
            w = r.ws
            smp, cnt, off, ts = _samples(w, o, d)
            if not outs:
                # the march, bit for bit: counts, ts and positions per segment
                assert np.array_equal(cnt, ocnt) and 1000 <= cnt.sum(1).min()
                for k in range(K):
                    idx, x = smp[k]
                    sl = slice(int(ostart[k, 0]), int(ostart[k, 0]) + len(idx))
                    assert np.array_equal(ts[idx].view(np.uint32), ots[sl].view(np.uint32))
                    assert np.array_equal(x.view(np.uint32), oxyz[sl].view(np.uint32))
            top = max(int(idx.max()) for idx, _ in smp) + 1
            feat = ER.decode_cache(w.feat[:(top + 31) // 32 * 32].cpu().numpy(), top)
            sigma, rgb = w.sigma[:top].cpu().numpy(), w.rgb[:top].cpu().numpy()
            outs.append([(feat[idx], sigma[idx], rgb[idx]) for idx, _ in smp])
    finally:
        _restore(r, saved)
    assert saved["level_fwd"] and saved["merged_fwd"]
    room = rel_w = 0.0
    for k in range(K):
        idx, x = smp[k]
        cells = ER.Cells(x, lv, mn, ext)
        e = ER.encode_cells(cells, table)
        for name, (feat, sigma, rgb) in zip(("level", "merged", "per-model"), (o_[k] for o_ in outs)):
            tag = f"scale {scale} {name} forward sub-NeRF {k}"
            where = lambda i, j: (f"sample {i} (ray {np.searchsorted(np.cumsum(cnt[k]), i, 'right')}) "
                                  f"x={x[i].tolist()} level {j // 2} feature {j % 2} "
                                  f"cell fraction {cells.f[i, j // 2].tolist()}")
            room = max(room, _check_features(feat, e, table, tag, where))
            ref = ER.transparent_sigma(e, a[k])
            rel = np.abs(sigma.astype(np.float64) - ref) / ref
            assert rel.max() <= 2.0 ** -10, f"{tag}: sigma of sample {int(np.argmax(rel))} off by {rel.max():.3e}"
            rel_w = max(rel_w, float(rel.max()))
            for got, first in zip((feat, sigma, rgb), outs[0][k]):
                assert np.array_equal(got.view(np.uint16 if got.dtype == np.float16 else np.uint32),
                                      first.view(np.uint16 if got.dtype == np.float16 else np.uint32)), \
                    f"{tag}: not bit-identical to the level forward"
    print(f"lattice rays forward scale {scale}: {cnt.sum(1).tolist()} samples, share of features "
          f"!= rn16(ref) {room:.2e}, sigma error / 2^-10 = {rel_w * 1024:.3f}")


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_production_backward_on_lattice_rays(cuda, scale):
    """(f) the field backward inside the fused chain on the lattice rays, per
    entry: rn_field_bwd_merged with fp32 atomics (the default at this size),
    the per-model rn_field_bwd in-chain (merged_bwd off), and the merged
    backward in fixed point (int32, scale 0.5) or binned (e5m17 page records,
    scale 16, with the coarse levels [0, 8) by fp32 atomics and with none).
    The reference takes the per-sample ws.dsigma and ws.sigma the chain left
    behind, so only the field backward is under test.

    Bound: (c), plus two terms that (c)'s precondition made zero.
    * (c) holds the seeds within a factor 256, so that none is an f16
      subnormal at the block's gradient scale.  The composite's seeds are not
      held so, and at scale 16 bar (c) alone fails: 203 of 389 k elements, up
      to 5.3x the bound (the per-model kernel 219; none at scale 0.5; the
      test prints these figures).  Derivation: the
      block scale G maps the block's largest seed (sigma and rgb chains) into
      [8, 16), so G >= 8 / M with M the step's largest of |dsigma sigma| and
      sigmoid'(0) |drgb| = |drgb| / 4.  f16(gsig G) below 2^-14 is off by up
      to half a subnormal quantum, 2^-25, and so is f16(b_j .) of the next
      layer; times a_j resp. c_j and 1 / G: each contribution w dfeat_j may be
      off by w (a_j + c_j) 2^-25 / G <= w (a_j + c_j) 2^-28 M.  That sum per
      entry is added.  It is 2^-19 of a contribution from a seed of size M.
    * The fixed-point forms add what they round and nothing measured
      (csrc/rn_bin.h): a record of level l is rint(v 2^e_l), so
      half a unit 2^-e_l per record, and a run of samples on one corner is one
      record, so at most n_e of them; an e5m17 record keeps that half unit
      below 2^15 units and rounds its mantissa above, for which 2^-18 A_e is
      added (the format's worst case there is 2^-15 of a record, which the
      2^-9 term's slack also covers).
    Measured, largest error / bound: scale 0.5 fp32 atomics 0.249, per-model
    0.249, fixed point 0.998 (16 levels; one record's half unit is attained);
    scale 16 fp32 atomics 0.442, per-model 0.442, binned 0.984 with 8 and with
    16 levels binned."""
    lv, m, g, table, bits, o, d, noise = _scene(cuda, scale)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    esf = 1 / 256 if scale > 0.5 else 0.0
    seeds = [to(s) for s in S.loss_seeds(len(o), K)]
    r = get_renderer(m, g, len(o))
    saved = _switches(r)
    a = ER.transparent_a(K)
    mn, ext = np.full(3, -scale, np.float32), np.full(3, 2 * scale, np.float32)

    def step():
        m.zero_grad(); g.zero_grad()
        res = ml_render_fused(m, g, to(o), to(d), to(d), noise=to(noise), exp_step_factor=esf)
        torch.autograd.backward([res["rgb"], res["opacity"], res["depth"]], seeds)
        return m.xyz_encoder.params.grad.view(-1, 2).clone()

    def reference():
        """per-entry sums from the workspace's samples and seeds (both sub-NeRFs
        scatter into the one table)"""
        w = r.ws
        smp, cnt, _, _ = _samples(w, o, d)
        sig, dsig = w.sigma.cpu().numpy().astype(np.float64), w.dsigma.cpu().numpy().astype(np.float64)
        xs, df = [], []
        for k in range(K):
            idx, x = smp[k]
            xs.append(x)
            df.append((k, dsig[idx] * sig[idx]))
        cells = ER.Cells(np.concatenate(xs), lv, mn, ext)
        e = ER.encode_cells(cells, table)
        n0 = 0
        dfeat = np.zeros_like(e)
        for k, seed in df:
            sl = slice(n0, n0 + len(seed))
            dfeat[sl] = a[k][None, :] * seed[:, None] * (ER.rn16(e[sl]) != 0)
            n0 += len(seed)
        assert np.count_nonzero(dfeat) > 1000
        ent, ref, ab, cnt = ER.grid_grad_entries(cells, dfeat)
        # the f16 subnormal term: 2^-28 M sum_contributions w (a_j + c_j)
        used = np.concatenate([idx for idx, _ in smp])
        M = max(np.abs(dsig[used] * sig[used]).max(), 0.25 * np.abs(w.drgb.cpu().numpy()[used]).max())
        ac = np.concatenate([np.broadcast_to(a[k] + ER.transparent_c(), (len(sd), 32)) for k, sd in df])
        sub = 2.0 ** -28 * M * ER.grid_grad_entries(cells, ac)[2]
        return ent, ref, ab, cnt, ER.doubtful_entries(cells, e), sub

    level_of = lambda ent: np.searchsorted(lv["offset"], ent, side="right") - 1
    report = {}
    try:
        assert r.scatter_mode == "fp32-atomics" and r.merged_bwd
        grad = step()
        ent, ref, ab, cnt, excl, sub = reference()
        report["fp32-atomics"] = _check_grid_grad(grad, lv, ent, ref, ab, cnt, excl,
                                                  f"scale {scale} merged fp32", sub)[0]
        r.merged_bwd = False
        assert r.scatter_mode == "fp32-atomics"
        grad = step()
        ent, ref, ab, cnt, excl, sub = reference()
        report["per-model"] = _check_grid_grad(grad, lv, ent, ref, ab, cnt, excl,
                                               f"scale {scale} per-model", sub)[0]
        r.merged_bwd = True
        modes = [("fixed-point", 0)] if scale <= 0.5 else [("binned", 8), ("binned", 0)]
        for mode, n32 in modes:
            r.grid_fx, r.grid_bin, r.bin_f32_levels = True, mode == "binned", n32
            assert r.scatter_mode == mode
            step()                       # a workspace's first such backward runs fp32 and sets the scales
            grad = step()
            _, scales, _, redo = r.ws._fx
            assert int(redo[0]) == 0
            used = scales[1 - r.ws.fx_i].cpu().numpy().astype(np.float64)   # the step just run
            assert np.count_nonzero(used[:n32]) == 0 and np.count_nonzero(used) >= 4, used
            report[f"{mode} f32_levels={n32} levels"] = float(np.count_nonzero(used))
            ent, ref, ab, cnt, excl, sub = reference()
            unit = np.where(used > 0, 1.0 / np.where(used > 0, used, 1.0), 0.0)[level_of(ent)]
            extra = sub + (0.5 * unit * cnt)[:, None]
            if mode == "binned":
                extra = extra + 2.0 ** -18 * ab * (unit > 0)[:, None]
            report[f"{mode} f32_levels={n32}"] = _check_grid_grad(
                grad, lv, ent, ref, ab, cnt, excl, f"scale {scale} {mode} f32_levels={n32}", extra)[0]
    finally:
        _restore(r, saved)
    print(f"lattice rays backward scale {scale}: largest error / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in report.items()))
