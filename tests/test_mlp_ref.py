"""CPU: the fp64 reference of the field MLPs (tests/mlp_ref.py) against the
fp32 oracle, and the power of the per-element bars of tests/test_gpu_mlp.py:
which single-slot defects of the kernels they are guaranteed to see.

* Oracle agreement: on the GPU tests' inputs oracle.field_oracle (torch fp32,
  autograd) stays within 0.5 of every final bound, i.e. within the budget.
* Forward power: each of the 9472 weight slots, swapped with its neighbour in
  the fragment (the same row, column i ^ 1: element j ^ 1 of the lane) and,
  separately, zeroed, moves an observable of some sample by more than twice
  its bound in the slot's banded case (so the defective kernel, itself within
  one bound of the altered reference, cannot stay inside the bar).
* Backward power: the same for the transposed slots (the bwd half of
  layout.field_frag_index and the input-gradient fragments), observed in the
  next layer's dW row, dE or dSH; and every dW element exceeds its bound in
  some case, so writing it elsewhere leaves a detectable zero.
* Seeded defects of bwd_window restated in the reference, against the new
  bars and the per-layer 1e-3 relative L2 of test_gpu_field.py.
* Probe exactness.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import field_oracle as fo
from oracle.ml_oracle import _split_field

import encode_ref as ER
import mlp_ref as MR

N = MR.N_SAMPLES
SCALES = (0.5, 16.0)


@functools.lru_cache(maxsize=None)
def _inputs(scale, dseed=0):
    c = ER.case(scale)
    e16 = ER.rn16(c.e[:N])
    e16.setflags(write=False)
    return e16, MR.directions(N, dseed), MR.seed_sets(N)


@functools.lru_cache(maxsize=None)
def _fwd(scale, name, anchored=True, dseed=0):
    e16, d, _ = _inputs(scale, dseed)
    flat = MR.probe_saturated_sets()[name[6:]] if name.startswith("probe ") else MR.weight_sets()[name]
    W = MR.split(flat)
    # as the GPU tests: the rgb net from the stored geo features (here the reference's own)
    if not anchored:
        # for the oracle: its geo features are its own, and its SH is another fp32 evaluation than
        # sh_lane's, for which only the absolute s holds (mlp_ref.sh_interval)
        return flat, W, MR.forward(e16, d, W, sh_relative=False)
    return flat, W, MR.forward(e16, d, W, geo_given=MR.forward(e16, d, W).g16)


# ---------------------------------------------------------------------------
# oracle agreement
# ---------------------------------------------------------------------------
def _oracle(monkeypatch, e16, d, flat, ds, dr):
    """oracle.field_oracle.field_forward / density_forward fed the given f16
    encoding (hash_encode patched to return it), its own fp32 SH kept for dSH"""
    e = torch.from_numpy(e16.astype(np.float32)).requires_grad_(True)
    keep = {}
    real_sh = fo.sh4

    def sh(dd):
        keep["sh"] = real_sh(dd)
        keep["sh"].retain_grad()
        return keep["sh"]

    monkeypatch.setattr(fo, "hash_encode", lambda u, gp, lv: e)
    monkeypatch.setattr(fo, "sh4", sh)
    mp = torch.from_numpy(flat.copy()).requires_grad_(True)
    z = torch.zeros(len(e16), 3)
    box = (torch.full((1, 3), -1.0), torch.full((1, 3), 1.0))
    sig, rgb = fo.field_forward(z, torch.from_numpy(d).requires_grad_(True), None, _split_field(mp), None, *box)
    torch.autograd.backward([sig, rgb], [torch.from_numpy(ds), torch.from_numpy(dr)])
    with torch.no_grad():
        _, feat = fo.density_forward(z, None, _split_field(mp), None, *box)
    t = lambda a: a.detach().numpy().astype(np.float64)
    return dict(sigma=t(sig), rgb=t(rgb), feat=t(feat), sh=t(keep["sh"]), dW=t(mp.grad), dE=t(e.grad),
                dSH=t(keep["sh"].grad))


def _ratio(got, ref, bound):
    err = np.abs(got - ref)
    assert np.all(err[bound == 0] == 0)
    return float((err / np.where(bound > 0, bound, 1.0)).max())


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", list(MR.weight_sets()) + ["probe rgb-", "probe g0+"])
def test_oracle_within_half_of_every_bound(monkeypatch, scale, name):
    """Coverage: every weight set of the GPU tests' (a) and (c) and two of the
    saturated probe sets, both scales, the first direction set, the seed sets
    normal, two_scales, steps and zero_iter (the other five are restrictions
    of these to a part of the samples or of the outputs).  What the oracle
    cannot vouch for is the f16 rounding of the dY and the `floor=` form of
    _round_scaled: autograd has neither, so those two branches are compared
    with nothing independent on the CPU; the GPU tests are their check.
    The reference runs its backward unrounded here, as autograd does (r16
    passes gradients through); the bounds are otherwise those the kernels
    are held to.  Measured (largest oracle error / final bound over scales
    and sets): sigma 0.48, rgb 0.49, SH 0.47 s, dW 0.50, dE 0.45, dSH 0.50 (0.50
    is attained where the oracle's ReLU mask differs at an undecided unit: the
    budget is exactly that unit's dY); geo features all inside the budget
    interval."""
    e16, d, seeds = _inputs(scale)
    flat, W, f = _fwd(scale, name, anchored=False)
    worst = {}
    for sname in ("normal", "two_scales", "steps", "zero_iter"):
        ds, dr = seeds[sname]
        o = _oracle(monkeypatch, e16, d, flat, ds, dr)
        b = MR.backward(f, W, ds, dr, rounded=False)      # autograd does not round a dY
        lo, hi = MR.rn16(f.v_g[:, 1:] - f.a_g[:, 1:]), MR.rn16(f.v_g[:, 1:] + f.a_g[:, 1:])
        assert np.all((o["feat"] >= lo) & (o["feat"] <= hi)), "geo features outside the budget interval"
        r = {"sigma": _ratio(o["sigma"], f.sigma, f.sigma_bound), "rgb": _ratio(o["rgb"], f.rgb, f.rgb_bound),
             "sh": float(np.abs(o["sh"] - f.y_sh).max() / MR.SH_S),
             "dW": _ratio(o["dW"], b.dW, b.dW_bound), "dE": _ratio(o["dE"], b.dE, b.dE_bound),
             "dSH": _ratio(o["dSH"], b.dSH, b.dSH_bound)}
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 0.5, f"scale {scale} {name} seeds {sname}: oracle {k} at {v:.3f} of its bound"
    print(f"oracle / bound, scale {scale} {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------
# forward power
# ---------------------------------------------------------------------------
def _geo_seen(f, vg):
    """vg (n, m, 17) altered geo pre-activations -> (m) some observable of some
    sample is outside its bar by the margin of a second bound"""
    a2 = 2 * f.a_g[:, None, 1:]
    out = (MR.rn16(vg[:, :, 1:] - a2) > f.geo_hi[:, None]) | (MR.rn16(vg[:, :, 1:] + a2) < f.geo_lo[:, None])
    sig = np.abs(np.exp(vg[:, :, 0]) - f.sigma[:, None]) > 2.0 * f.sigma_bound[:, None]
    return out.any((0, 2)) | sig.any(0)


def _rgb_seen(f, out):
    """out (n, m, 3) altered rgb pre-activations"""
    return (np.abs(MR.sigmoid(out) - f.rgb[:, None]) > 2.0 * f.rgb_bound[:, None]).any((0, 2))


def _relu16(v):
    return np.maximum(MR.rn16(v), 0.0)


def _unit_seen(f, W, name, j, dv):
    """dv (n, m): m alterations of the pre-activation of unit / row j of layer
    `name`; (m) whether each is seen"""
    if name == "g2":
        vg = np.repeat(f.v_g[:, None, :], dv.shape[1], 1)
        vg[:, :, j] += dv
        return _geo_seen(f, vg)
    if name == "g1":
        dh = _relu16(f.v_h1[:, j, None] + dv) - f.h1[:, j, None]
        return _geo_seen(f, f.v_g[:, None, :] + dh[:, :, None] * W["g2"][:, j])
    if name == "r3":
        out = np.repeat(f.out[:, None, :], dv.shape[1], 1)
        out[:, :, j] += dv
        return _rgb_seen(f, out)
    if name == "r2":
        dr2 = _relu16(f.v_r2[:, j, None] + dv) - f.r2[:, j, None]
        return _rgb_seen(f, f.out[:, None, :] + dr2[:, :, None] * W["r3"][:, j])
    dr1 = _relu16(f.v_r1[:, j, None] + dv) - f.r1[:, j, None]
    r2 = _relu16(f.v_r2[:, None, :] + dr1[:, :, None] * W["r2"][:, j])
    return _rgb_seen(f, r2 @ W["r3"].T)


_INPUT = {"g1": "e", "g2": "h1", "r1": "xin", "r2": "r1", "r3": "r2"}


def _forward_power(f, W, masks):
    """per layer (rows, cols) bool: the slot's swap AND its zeroing are seen;
    only slots of `masks` are tried"""
    seen = {}
    for name, (rows, cols) in MR.SIZES.items():
        x = getattr(f, _INPUT[name])
        ok = np.zeros((rows, cols), bool)
        for j in range(rows):
            i = np.flatnonzero(masks[name][j])
            if not len(i):
                continue
            w, wn = W[name][j, i], W[name][j, i ^ 1]
            zero = -w * x[:, i]
            swap = (wn - w) * (x[:, i] - x[:, i ^ 1])
            s = _unit_seen(f, W, name, j, np.concatenate([zero, swap], 1))
            ok[j, i] = s[:len(i)] & s[len(i):]
        seen[name] = ok
    return seen


def test_forward_power_every_slot():
    """Condition: all 9472 forward slots are seen, swapped and zeroed, in their
    banded case, by the 600 samples of one of mlp_ref.INPUT_CASES (the GPU
    test runs them all).  Information: the share seen under the dense weights
    (measured: 9472 of 9472 banded; dense 0.998)."""
    total = {k: np.zeros(s, bool) for k, s in MR.SIZES.items()}
    for b in range(8):
        masks = {k: MR.banded_mask(k, b) for k in MR.SIZES}
        seen = {k: np.zeros(s, bool) for k, s in MR.SIZES.items()}
        for scale, dseed in MR.INPUT_CASES:
            _, W, f = _fwd(scale, f"banded{b}", dseed=dseed)
            for k, v in _forward_power(f, W, masks).items():
                seen[k] |= v
        for k in MR.SIZES:
            missed = np.argwhere(masks[k] & ~seen[k])
            assert not len(missed), f"band {b} layer {k}: {len(missed)} slots unseen, first {missed[0].tolist()}"
            total[k] |= seen[k]
    assert sum(int(v.sum()) for v in total.values()) == MR.FIELD_PARAMS
    dense = {k: np.zeros(s, bool) for k, s in MR.SIZES.items()}
    for scale, dseed in MR.INPUT_CASES:
        _, W, f = _fwd(scale, "dense", dseed=dseed)
        for k, v in _forward_power(f, W, {k: np.ones(s, bool) for k, s in MR.SIZES.items()}).items():
            dense[k] |= v
    share = sum(int(v.sum()) for v in dense.values()) / MR.FIELD_PARAMS
    print(f"forward power: 9472 of 9472 slots seen in their banded case; dense {share:.3f}")


# ---------------------------------------------------------------------------
# backward power
# ---------------------------------------------------------------------------
# transposed layer -> (its dY, the ReLU activation masking its output or None,
#                      what shows the altered output: the next dW's name and X, or dE / dSH)
def _bwd_views(f, b):
    return {"r3": (b.dO, f.r2, "r2", f.r1), "r2": (b.dR2, f.r1, "r1", f.xin),
            "r1": (b.dR1, None, "g2", f.h1), "g2": (b.dG, f.h1, "g1", f.e), "g1": (b.dH1, None, None, None)}


def _backward_power(f, W, b, masks):
    """per layer (rows, cols) bool: the transposed slot [o, i] (k index o, row
    i), swapped with its neighbour o ^ 1 and zeroed, is seen"""
    seen = {}
    views = _bwd_views(f, b)
    for name, (rows, cols) in MR.SIZES.items():
        dy, act, nxt, x = views[name]
        ok = np.zeros((rows, cols), bool)
        for i in range(cols):
            o = np.flatnonzero(masks[name][:, i])
            if not len(o):
                continue
            on = _g2_neighbour(o) if name == "g2" else np.where((o ^ 1) < rows, o ^ 1, -1)
            pad = on < 0                                  # a padding slot: weight 0, dY 0
            w, wn = W[name][o, i], np.where(pad, 0.0, W[name][on, i])
            dyn = np.where(pad, 0.0, dy[:, on])
            d = np.concatenate([-w * dy[:, o], (wn - w) * (dy[:, o] - dyn)], 1)            # (n, 2 m)
            if act is not None:
                d = d * (act[:, i, None] > 0)
            if name == "g1":
                s = (np.abs(d) > 2.0 * b.dE_bound[:, i, None]).any(0)
            elif name == "r1" and i < 16:
                s = (np.abs(d) > 2.0 * b.dSH_bound[:, i, None]).any(0)
            else:
                row = i - 15 if name == "r1" else i          # geo feature g -> dG column 1 + g
                bound = MR.mat(b.dW_bound, nxt)[row]
                s = (np.abs(d.T @ x) > 2.0 * bound).any(1)
            ok[o, i] = s[:len(o)] & s[len(o):]
        seen[name] = ok
    return seen


def _g2_neighbour(o):
    """k index of output o in the transposed geo fragments is acc row o - 1
    (row 16 for output 0): the neighbouring element is acc row (o - 1) ^ 1"""
    row = np.where(o == 0, 16, o - 1)
    nrow = row ^ 1                                # row 17 is padding
    return np.where(nrow == 17, -1, np.where(nrow == 16, 0, nrow + 1))


POWER_SEEDS = ("normal", "dsigma_only", "drgb_only")


def test_backward_power_every_slot_and_dw_element():
    """All transposed slots seen in their banded case, in one of
    mlp_ref.INPUT_CASES with one of the seed sets POWER_SEEDS (with both seeds
    live the sigma seed's rounding hides a slot of the rgb path in the geo
    layers' dW), every dW element above its bound in some banded or dense case.
    Measured: 9472 of 9472 transposed slots (the 1024 SH columns through dSH),
    9472 dW elements."""
    total = {k: np.zeros(s, bool) for k, s in MR.SIZES.items()}
    big = np.zeros(MR.FIELD_PARAMS, bool)
    for b in range(8):
        masks = {k: MR.banded_mask(k, b) for k in MR.SIZES}
        seen = {k: np.zeros(s, bool) for k, s in MR.SIZES.items()}
        for scale, dseed in MR.INPUT_CASES:
            _, W, f = _fwd(scale, f"banded{b}", dseed=dseed)
            for sname in POWER_SEEDS:
                bw = MR.backward(f, W, *_inputs(scale)[2][sname])
                big |= np.abs(bw.dW) > bw.dW_bound
                for k, v in _backward_power(f, W, bw, masks).items():
                    seen[k] |= v
        for k in MR.SIZES:
            missed = np.argwhere(masks[k] & ~seen[k])
            assert not len(missed), f"band {b} layer {k}: {len(missed)} transposed slots unseen, first {missed[0].tolist()}"
            total[k] |= seen[k]
    total = sum(int(v.sum()) for v in total.values())
    assert total == MR.FIELD_PARAMS
    for scale, dseed in MR.INPUT_CASES:
        _, W, f = _fwd(scale, "dense", dseed=dseed)
        for sname in POWER_SEEDS:
            bw = MR.backward(f, W, *_inputs(scale)[2][sname])
            big |= np.abs(bw.dW) > bw.dW_bound
    missed = np.flatnonzero(~big)
    assert not len(missed), f"{len(missed)} dW elements never above their bound, first {MR.where(missed[0])}"
    print(f"backward power: {total} transposed slots seen, {int(big.sum())} dW elements above their bound")


# ---------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------
def _old_bar(dw, ref):
    """test_gpu_field.py's bar: relative L2 per layer, the largest"""
    return max(float(np.linalg.norm(MR.mat(dw, k) - MR.mat(ref, k)) / max(np.linalg.norm(MR.mat(ref, k)), 1e-30))
               for k in MR.SIZES)


@pytest.mark.parametrize("defect,wname,sname", [
    ("mask_kstep", "dense", "normal"), ("mask_kstep", "banded2", "normal"),
    ("rgb_scale", "dense", "two_scales"), ("no_clamp", "hot", "normal"),
    ("no_remap", "dense", "normal"), ("no_remap", "banded2", "normal")])
def test_seeded_defects_are_flagged(defect, wname, sname):
    """Each defect of MR.DEFECTS, restated in the reference's backward, leaves
    the per-element bars (dW or dE) by more than a second bound.  Whether the
    per-layer 1e-3 relative L2 of test_gpu_field.py would have seen it
    (measured, largest layer): mask_kstep 0.96 (seen), rgb_scale 1.06 (seen
    with these seeds), no_clamp: not reachable there (|g0| <= 0.11 with its
    weights; 9.5e9 with the hot probe weights), no_remap 1.40 (seen).  The rgb3
    guard widened adds exact zeros (MR.backward docstring)."""
    e16, d, seeds = _inputs(0.5)
    flat = MR.probe(2, g0_gain=512.0) if wname == "hot" else MR.weight_sets()[wname]
    W = MR.split(flat)
    f = MR.forward(e16, d, W)
    if wname == "hot":
        assert (f.g0 > 15).sum() >= 10 and f.g0.max() < 80
    ds, dr = seeds[sname]
    good, bad = MR.backward(f, W, ds, dr), MR.backward(f, W, ds, dr, defect=defect)
    n_dw = int((np.abs(bad.dW - good.dW) > 2.0 * good.dW_bound).sum())
    n_de = int((np.abs(bad.dE - good.dE) > 2.0 * good.dE_bound).sum())
    old = _old_bar(bad.dW, good.dW)
    print(f"defect {defect} ({wname}, {sname}): {n_dw} dW elements and {n_de} dE values flagged; "
          f"old per-layer bar {old:.2e} ({'seen' if old > 1e-3 else 'NOT seen'})")
    assert n_dw + n_de > 0


# ---------------------------------------------------------------------------
# the probe bound, scale equivariance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dseed", [0, 1])
def test_probe_bound_is_tight(dseed):
    """Under the saturated probe sets of test_gpu_mlp.py the reference's dW
    bound is, for every element with a non-zero sum |terms|, at most the tight
    (2^-9 + n 2^-23) sum |terms|; the exceptions (an f16-subnormal dY at the
    block's scale, whose floor 2^-25 / G is absolute) are at most 1 % of the
    non-zero elements and stay below sum |terms| / 4.  No bound exceeds sum |terms|, so
    a kernel that wrote 0 or the wrong sign cannot pass; no ReLU mask of the
    rgb net is undecided (the relative SH interval decides the near-pole
    directions).  An element without terms has bound 0.
    Measured: median 0.07 of the tight bound, largest 0.55 and 0.95 (direction
    sets 0 and 1); exceptions 2 of
    387 non-zero elements in rgb- with either direction set (34 and 114 times
    the tight bound, 0.066 and 0.22 of sum |terms|)."""
    e16, d, seeds = _inputs(0.5, dseed)
    ds, dr = seeds["normal"]
    worst, n_over = 0.0, 0
    for name, flat in MR.probe_saturated_sets().items():
        W = MR.split(flat)
        f = MR.forward(e16, d, W, geo_given=MR.forward(e16, d, W).g16)
        for act in ("r1", "r2"):
            assert not ((getattr(f, "lo_" + act) > 0) != (getattr(f, "hi_" + act) > 0)).any(), f"{name}: undecided {act} mask"
        b = MR.backward(f, W, ds, dr)
        tight = MR.probe_tight(b, N)
        nz = b.dW_mag > 0
        assert np.all(b.dW_bound[~nz] == 0) and np.all(b.dW[~nz] == 0)
        over = b.dW_bound > tight
        assert over.sum() <= 1e-2 * nz.sum(), f"{name}: {int(over.sum())} bounds above the tight one"
        assert np.all(b.dW_bound[over] <= 0.25 * b.dW_mag[over])
        n_over += int(over.sum())
        worst = max(worst, float((b.dW_bound[nz & ~over] / tight[nz & ~over]).max()))
    print(f"probe bound directions {dseed}: largest bound / tight {worst:.3f} outside {n_over} subnormal-floor elements")


def test_scale_equivariance_stays_in_fp32_range():
    """test_gpu_mlp.py (f) multiplies the seeds by 2^k, k in {-40, -8, 8}.  On
    the reference's backward with seeds of the size of the chain's loss seeds
    (N(0, 1) 2^-10; the chain's per-sample seeds exist only on the GPU, where
    the test checks the range of the unscaled gradients): every non-zero
    seed, dY, dE and dW element times 2^k, and every scaled dY and scaled dW
    accumulator (times the block's gradient scale), stays a normal fp32
    number, and the reference itself is then exactly equivariant: dW and dE of
    the scaled seeds are bitwise 2^k times the unscaled ones."""
    e16, d, seeds = _inputs(0.5)
    _, W, f = _fwd(0.5, "dense")
    ds, dr = (s * np.float32(2.0 ** -10) for s in seeds["normal"])
    base = MR.backward(f, W, ds, dr)
    for k in (-40, -8, 8):
        b = MR.backward(f, W, ds * np.float32(2.0 ** k), dr * np.float32(2.0 ** k))
        assert np.array_equal(b.dW, base.dW * 2.0 ** k) and np.array_equal(b.dE, base.dE * 2.0 ** k)
        assert np.array_equal(b.R * 2.0 ** k, base.R) and np.array_equal(b.G * 2.0 ** k, base.G)
        scaled = [b.dO * b.R[:, None], b.dR2 * b.R[:, None], b.dR1 * b.R[:, None], b.dG * b.G[:, None],
                  b.dH1 * b.G[:, None], b.dW * b.R.max(), b.dW * b.G.min()]
        for v in [b.o, b.gsig, b.dO, b.dR2, b.dR1, b.dG, b.dH1, b.dE, b.dW, b.R, b.G] + scaled:
            nz = np.abs(v[v != 0])
            assert nz.min() >= 2.0 ** -126 and nz.max() < 2.0 ** 127, f"k {k}: a value leaves the fp32 normal range"


# ---------------------------------------------------------------------------
# probe exactness
# ---------------------------------------------------------------------------
def _pow2(r):
    m, _ = np.frexp(r)
    return np.all(np.abs(m) == 0.5)


@pytest.mark.parametrize("shift", MR.PROBE_SHIFTS)
def test_probe_hidden_values_are_inputs_times_powers_of_two(shift):
    e16, d, _ = _inputs(0.5)
    W = MR.split(MR.probe(shift))
    f = MR.forward(e16, d, W)
    for name, inp, hid in (("g1", f.e, f.h1), ("r1", f.xin, f.r1), ("r2", f.r1, f.r2)):
        nz = W[name] != 0
        assert np.all(nz.sum(1) == 1)
        col = nz.argmax(1)
        w = W[name][np.arange(len(col)), col]
        assert _pow2(w)
        assert np.array_equal(hid, np.maximum(w * inp[:, col], 0.0))      # bit-equal: no rounding happened
    for name in ("g2", "r3"):
        nz = W[name] != 0
        assert np.all(nz.sum(1) == 1) and _pow2(W[name][nz])
    u0, s0, outs, m = MR.probe_wiring(shift)
    assert np.array_equal(f.g0, W["g2"][0, u0] * f.h1[:, u0])
    for c, (u, s) in enumerate(outs):
        assert np.array_equal(f.out[:, c], W["r3"][c, u] * f.r2[:, u]) and m[u] > 0
    # both ReLU branches of each pair occur
    assert ((f.h1[:, :32] > 0) & (f.h1[:, 32:] == 0)).any() and ((f.h1[:, :32] == 0) & (f.h1[:, 32:] > 0)).any()


def test_probe_shifts_reach_every_sh_coefficient_with_each_sign():
    got = set()
    for shift in MR.PROBE_SHIFTS:
        got |= {u for u, _ in MR.probe_wiring(shift)[2]}
    assert got == set(MR.PROBE_UNITS)
