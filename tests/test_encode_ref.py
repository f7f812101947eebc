"""tests/encode_ref.py (the fp64 hash-encoding reference of test_gpu_encode.py)
against the independent torch oracle, and its inputs against what they were
built for.  CPU only."""
import numpy as np
import pytest
import torch

import oracle
from oracle import field_oracle as fo
from oracle import ml_oracle
from radnerf_amd import synthetic as S

import encode_ref as ER

SCALES = [0.5, 4.0, 16.0]


def _case(scale):
    """positions (adversarial set, then the ordered sequences), f16 table,
    reference cells and features of one scale"""
    c = ER.case(scale)
    return c.lv, c.x, c.table, c.cells, c.e


def _oracle_run(scale, ind=1, K=2):
    """field_forward with the transparent MLP of sub-NeRF `ind`, autograd on"""
    lv, x, table, cells, e = _case(scale)
    a = ER.transparent_a(K)
    mlp = torch.from_numpy(ER.transparent_mlp(K, a))
    gp = torch.from_numpy(table.astype(np.float32)).requires_grad_(True)
    xo = torch.from_numpy(np.array(x)).requires_grad_(True)
    d = torch.zeros(len(x), 3)
    d[:, 0] = 1.0
    sig, rgb = fo.field_forward(xo, d, gp, ml_oracle._split_field(mlp[ind]), lv,
                                torch.full((1, 3), -float(scale)), torch.full((1, 3), float(scale)))
    return a[ind], sig, rgb, gp, xo


@pytest.mark.parametrize("scale", SCALES)
def test_encode_matches_oracle(scale):
    """fp64 features vs hash_encode's fp32 fma chain: 2^-20 max|table| (8 corner
    products of at most three roundings each and 8 fma roundings, weights
    summing to 1: 12 * 2^-24 max|table|).  Measured 0.17-0.23 of the bar."""
    lv, x, table, cells, e = _case(scale)
    u = fo.unit_coords(torch.from_numpy(np.array(x)), torch.full((1, 3), -float(scale)),
                       torch.full((1, 3), float(scale)))
    assert np.array_equal(u.numpy(), cells.u)
    ref = fo.hash_encode(u, torch.from_numpy(table.astype(np.float32)), lv).numpy()
    bar = 2.0 ** -20 * float(np.abs(table.astype(np.float64)).max())
    err = np.abs(e - ref).max()
    print(f"encode vs oracle scale {scale}: max err / bar {err / bar:.3f}")
    assert err <= bar
    # the two public entry points agree with the precomputed form
    mn, ext = np.full(3, -scale, np.float32), np.full(3, 2 * scale, np.float32)
    assert np.array_equal(ER.encode(x[:100], table, lv, mn, ext), e[:100])
    for l in (0, 15):
        g, _ = ER.level_cells(cells.u, lv, l)
        assert np.array_equal(ER.corner_indices(lv, l, g) + int(lv["offset"][l]), cells.idx[:, l])


def test_decode_cache_roundtrip():
    """decode_cache inverts the kernels' cache layout, written out here from
    its description: lane c + 32 h, k-step s, element j <-> level
    2 h + (q & 1) + 4 (q >> 1) with q = 4 s + (j >> 1), feature j & 1."""
    n = 70
    want = np.arange(n * 32, dtype=np.float16).reshape(n, 32)
    feat = np.full((3, 64, 2, 8), -1, np.float16)
    for i in range(n):
        for h in range(2):
            for s in range(2):
                for j in range(8):
                    q = 4 * s + (j >> 1)
                    level = 2 * h + (q & 1) + 4 * (q >> 1)
                    feat[i // 32, i % 32 + 32 * h, s, j] = want[i, 2 * level + (j & 1)]
    assert np.array_equal(ER.decode_cache(feat.reshape(-1, 32), n), want)


@pytest.mark.parametrize("scale", SCALES)
def test_transparent_mlp(scale):
    """With transparent_mlp the oracle's sigma is exp(sum a_j r16(e_j)) (to the
    fp32 rounding of its 64-term dot product and expf) and its rgb exactly 0.5;
    the caps the GPU tests rely on hold."""
    lv, x, table, cells, e = _case(scale)
    # the oracle's own fp32 features: its f16 roundings, ties included
    e_o = fo.hash_encode(torch.from_numpy(cells.u), torch.from_numpy(table.astype(np.float32)),
                         lv).numpy()
    for ind in range(2):
        a, sig, rgb, _, _ = _oracle_run(scale, ind)
        ref = ER.transparent_sigma(e_o, a)
        mag = (np.abs(ER.rn16(e)) * a).sum(1)
        rel = np.abs(sig.detach().numpy() - ref) / ref
        assert np.all(rel <= 2.0 ** -18 * np.maximum(mag, 1.0) + 2.0 ** -22), rel.max()
        # against the fp64 features, an f16 tie may flip: the GPU tests' 2^-10
        rel = np.abs(sig.detach().numpy() - ER.transparent_sigma(e, a)) / ref
        print(f"transparent sigma scale {scale} sub-NeRF {ind}: rel {rel.max():.2e}")
        assert rel.max() <= 2.0 ** -10
        assert torch.all(rgb == 0.5)
        # TruncExp's backward clamp stays inactive
        assert mag.max() < 15
    a2 = ER.transparent_a(2)
    assert np.all(a2[0] != a2[1])
    assert np.all(a2[:, 1:] != a2[:, :-1]) and np.all(a2[:, 2:] != a2[:, :-2])
    assert np.all((a2 >= 0.25) & (a2 <= 4) & (np.log2(a2) % 1 == 0))


@pytest.mark.parametrize("scale", SCALES)
def test_gradients_match_autograd(scale):
    """grid_grad and dencode_dx vs autograd of the oracle with the transparent
    MLP: fp32 against fp64, so per entry (8 + n_e) 2^-23 of the magnitude sum
    (a few roundings per contribution and the fp32 sum in any order), and per
    sample and axis 2^-18 of the magnitude sum.  Samples with a feature at an
    f16 zero (ReLU' undefined) are left out on both sides."""
    lv, x, table, cells, e = _case(scale)
    a, sig, rgb, gp, xo = _oracle_run(scale)
    sig_o = sig.detach().numpy().astype(np.float64)
    ds = ER.dsigma_seeds(sig_o, seed=5)
    sig.backward(torch.from_numpy(ds))
    dfeat = a[None, :] * (ds.astype(np.float64) * sig_o)[:, None] * (ER.rn16(e) != 0)
    ent, g, ab, cnt = ER.grid_grad_entries(cells, dfeat)
    excl = ER.doubtful_entries(cells, e)
    keep = ~np.isin(ent, excl)
    og = gp.grad.numpy().astype(np.float64)
    ratio = np.abs(og[ent] - g) / np.maximum((8 + cnt)[:, None] * 2.0 ** -23 * ab, 1e-300)
    print(f"grid_grad vs autograd scale {scale}: max err / bar {ratio[keep].max():.3f}, "
          f"{len(excl)} of {len(ent)} entries excluded")
    assert ratio[keep].max() <= 1
    untouched = np.ones(len(og), bool)
    untouched[ent] = False
    assert np.all(og[untouched] == 0)
    # the dense forms
    mn, ext = np.full(3, -scale, np.float32), np.full(3, 2 * scale, np.float32)
    gd, cd = ER.grid_grad(x[:200], dfeat[:200], lv, mn, ext)
    e2, g2, a2, c2 = ER.grid_grad_entries(cells, dfeat, 200)
    assert np.array_equal(gd[e2], g2) and np.array_equal(cd[e2], c2) and cd.sum() == 200 * 128
    assert np.array_equal(ER.abs_grid_grad(x[:200], dfeat[:200], lv, mn, ext)[e2], a2)
    # input gradient
    D, A = ER.dencode_dx_cells(cells, table)
    dx = (dfeat[:, :, None] * D).sum(1)
    bar = 2.0 ** -18 * (np.abs(dfeat)[:, :, None] * A).sum(1)
    sure = ~ER.doubtful(e).any(1)
    err = np.abs(xo.grad.numpy() - dx)
    assert np.all(err[sure] <= bar[sure] + 1e-300), (err[sure] / np.maximum(bar[sure], 1e-300)).max()
    clipped = (cells.v < 0) | (cells.v > 1)
    assert np.all(dx[clipped] == 0) and clipped.sum() > 100
    assert np.abs(dx[sure]).max() > 0


@pytest.mark.parametrize("scale", SCALES + [1.0])
def test_inputs_hit_their_targets(scale):
    """At least 50 samples of each kind the construction aims at, and the
    caps of the GPU tests: seeds within a factor 256, at most 0.1 % of the
    touched entries excluded."""
    lv, x, table, cells, e = _case(scale)
    assert 3000 <= len(x) <= 4500
    dense = np.array([ER.is_dense(lv, l) for l in range(16)])
    assert 2 <= dense.sum() <= 8
    f0 = (cells.f == 0).any(2)                                # (N, 16)
    kinds = {
        "f == 0 on a dense level": f0[:, dense].any(1),
        "f == 0 on a hashed level": f0[:, ~dense].any(1),
        "u == 0": (cells.u == 0).any(1),
        "u == 1": (cells.u == 1).any(1),
        "dense index wraps": (cells.raw[:, dense] >= lv["hsize"][dense][None, :, None]).any((1, 2)),
        "f > 0.999": (cells.f > 0.999).any((1, 2)),
    }
    counts = {k: int(v.sum()) for k, v in kinds.items()}
    print(f"scale {scale}: {len(x)} points, {counts}")
    for k, c in counts.items():
        assert c >= 50, (k, c)
    # the wrap stays below 2 hsize (the kernels' one conditional subtract)
    for l in np.nonzero(dense)[0]:
        assert cells.raw[:, l].max() < 2 * int(lv["hsize"][l])
    for ind in range(2):
        sig = ER.transparent_sigma(e, ER.transparent_a(2)[ind])
        p = np.abs(ER.dsigma_seeds(sig, seed=5).astype(np.float64) * sig)
        assert p.max() / p.min() <= 8          # far inside the factor 256
    for name, sl in ER.case(scale).runs.items():
        excl = ER.doubtful_entries(cells, e, sl)
        touched = len(np.unique(cells.idx[sl]))
        if len(excl):
            print(f"scale {scale} {name}: {len(excl)} of {touched} touched entries excluded")
        assert len(excl) <= 1e-3 * touched, name


def test_ordered_sequences():
    for scale in (0.5, 16.0):
        lv = fo.grid_levels(scale)
        x = ER.ordered_sequences(scale, lv)
        mn, ext = np.full(3, -scale, np.float32), np.full(3, 2 * scale, np.float32)
        runs = [0, 2, 65, 129, 194, 494]
        for a, b in zip(runs[:-1], runs[1:]):
            assert np.all(x[a:b] == x[a]) and (b == 494 or np.any(x[b] != x[a]))
        g, _ = ER.level_cells(ER.unit_coords(x[494:], mn, ext), lv, 15)
        same, adj = g[:128], g[128:]
        assert len(adj) == 128 and np.all(same == same[0]) and np.any(x[494] != x[495])
        assert np.all(adj[0::2] == adj[0]) and np.all(adj[1::2] == adj[0] + [1, 0, 0])


@pytest.mark.parametrize("scale", [0.5, 16.0])
def test_lattice_rays(scale):
    """The axis-aligned rays: every one hits the box (no origin on a slab
    face), off-axis origins strictly inside, some on an exact lattice plane,
    and the oracle's march gives 1 k to 20 k samples per sub-NeRF."""
    lv = fo.grid_levels(scale)
    o, d = ER.lattice_rays(scale, lv)
    assert o.shape == (24, 3) and np.all((d != 0).sum(1) == 1) and np.all(d.sum(1) == 1)
    ax = np.argmax(d, 1)
    assert np.all(np.bincount(ax) == 8)
    off = d == 0
    assert np.all(np.abs(o[off]) < scale) and np.all(o[~off] == np.float32(-3 * scale))
    mn, ext = np.full(3, -scale, np.float32), np.full(3, 2 * scale, np.float32)
    u = ER.unit_coords(o, mn, ext)
    on_plane = np.zeros(24, bool)
    for l in range(16):
        _, f = ER.level_cells(u, lv, l)
        on_plane |= ((f == 0) & off).any(1)
    assert on_plane.sum() >= 4
    ht = ml_oracle._hits(o, d, scale)
    assert np.all(np.isfinite(ht)) and np.all(ht[:, 0] > 0) and np.all(ht[:, 1] > ht[:, 0])
    K = 2
    cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)
    bits = S.bitfields(K, cascades, p=0.25)
    noise = S.noise(K, 24)
    esf = 1 / 256 if scale > 0.5 else 0.0
    for k in range(K):
        _, xyzs, _, _, ts, total = oracle.raymarching_train(o, d, ht, bits[k], cascades, scale, esf,
                                                            noise[k])
        print(f"lattice rays scale {scale} sub-NeRF {k}: {total} samples")
        assert 1000 <= total <= 20000
        assert np.all(np.isfinite(xyzs)) and np.all(np.isfinite(ts))
