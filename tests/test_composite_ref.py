"""CPU: tests/composite_ref.py, the fp64 restatement of the compositing
kernels and its rounding bounds, before the GPU tests rely on it.

  1. its backward is the derivative of its forward (central differences in
     fp64), with dL_dws given, absent, and as the in-chain distortion gradient;
  2. the serial fp32 oracle stays inside every bound on the GPU tests' own
     inputs, at no more than half of it: a scale that misses a term would show
     here as a ratio near or above 1;
  3. three classic wave-scan defects seeded into the fp64 dsigma are flagged
     on every segment they touch, while each stays under the old absolute bar
     1e-4 max(1, |ref|max) on some touched segment.
"""
import numpy as np
import pytest

import composite_ref as CR
import oracle

F32 = np.float32


@pytest.fixture(scope="module")
def pool():
    return CR.make_segments()


@pytest.fixture(scope="module")
def full(pool):
    p = CR.prepare(CR.pack(pool))
    CR.check_conditions(p, p["orc"]["used"])
    return p


# ---------------------------------------------------------------------------
# 1. finite differences
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["plain", "dws", "dist"])
def test_backward_is_the_forwards_derivative(mode):
    rng = np.random.default_rng(4)
    for n in (1, 5, 70):
        dl = rng.uniform(5e-3, 2e-2, n)
        ts = np.cumsum(dl) + 0.4
        sig = rng.gamma(1.0, 2.0 / (n * dl.mean()), n)
        sig[rng.random(n) < 0.3] = 0.0
        rgbs = rng.random((n, 3))
        starts, counts, used = np.array([0]), np.array([n]), np.array([n])
        gO, gD, gR = rng.normal(0, 1, 1), rng.normal(0, 1, 1), rng.normal(0, 1, (1, 3))
        gw = rng.normal(0, 1, n)
        gdist = rng.normal(0, 1, 1)

        def run(s, c):
            f = CR.forward(1 - np.exp(-s * dl), c, ts, starts, counts, used)
            loss = gO[0] * f["opacity"][0] + gD[0] * f["depth"][0] + (gR[0] * f["rgb"][0]).sum()
            d = CR.distortion_fw(f["ws"], dl, ts, starts, counts, rel=True)
            if mode == "dws":
                loss += (gw * f["ws"]).sum()
            elif mode == "dist":
                loss += gdist[0] * d["loss"][0]
            return loss, f, d

        _, f, d = run(sig, rgbs)
        kw = {}
        if mode == "dws":
            kw = dict(gw=gw, ws=f["ws"])
        elif mode == "dist":
            kw = dict(gdist=gdist, dist=d["loss"], ws=f["ws"])
        b = CR.backward(1 - np.exp(-sig * dl), rgbs, dl, ts, starts, counts, used, f["opacity"],
                        f["depth"], f["rgb"], gO, gD, gR, **kw)
        h = 1e-6 / dl.mean()
        for i in sorted({0, n // 3, n - 1}):
            sp, sm = sig.copy(), sig.copy()
            sp[i] += h; sm[i] -= h
            fd = (run(sp, rgbs)[0] - run(sm, rgbs)[0]) / (2 * h)
            assert abs(fd - b["dsig"][i]) <= 1e-6 * b["scale"][i] + 1e-12, (mode, n, i)
            if mode == "plain":
                cp, cm = rgbs.copy(), rgbs.copy()
                cp[i, 1] += 1e-4; cm[i, 1] -= 1e-4
                fd = (run(sig, cp)[0] - run(sig, cm)[0]) / 2e-4
                assert abs(fd - b["drgb"][i, 1]) <= 1e-9 * max(1.0, abs(fd))


def test_distortion_gradient_is_the_loss_derivative():
    rng = np.random.default_rng(6)
    n = 40
    dl, w = rng.uniform(1e-3, 5e-3, n), rng.random(n) / n
    ts = np.cumsum(dl) + 2.0
    starts, counts, g = np.array([0]), np.array([n]), np.array([0.7])
    gw, _ = CR.distortion_bw(g, w, dl, ts, starts, counts)
    for rel in (False, True):
        loss = lambda v: g[0] * CR.distortion_fw(v, dl, ts, starts, counts, rel)["loss"][0]
        for i in (0, 13, n - 1):
            wp, wm = w.copy(), w.copy()
            wp[i] += 1e-6; wm[i] -= 1e-6
            assert abs((loss(wp) - loss(wm)) / 2e-6 - gw[i]) <= 1e-8


# ---------------------------------------------------------------------------
# 2. the fp32 oracle against the bounds
# ---------------------------------------------------------------------------


def _oracle_vs_bounds(p, seeds, out, tag=""):
    """forward, backward without / with dL_dws and the explicit distortion
    chain of the fp32 oracle on the packed set p, per-segment seeds given"""
    o, lay = p["orc"], p["lay"]
    gO, gD, gR, gO_ref, gD_ref, gR_ref, gO_abs = seeds
    args = (p["alpha"], p["rgbs"], p["ts"], p["starts"], p["counts"], o["used"])
    f = CR.forward(*args)
    CR.check(tag + "ws", o["ws"], f["ws"], CR.bar_ws(f["ws"], lay["k"]), out)
    for k in ("opacity", "depth", "rgb"):
        CR.check(tag + k, o[k], f[k], CR.bar_out(f[k], lay["m"]), out)
    rows = CR.rows_of(p)
    bargs = (p["alpha"], p["rgbs"], p["dl"], p["ts"], p["starts"], p["counts"], o["used"],
             o["opacity"], o["depth"], o["rgb"], gO_ref, gD_ref, gR_ref)
    rng = np.random.default_rng(9)
    gW = rng.normal(0, 1, p["cap"]).astype(F32)
    zero = np.zeros(p["cap"], F32)
    # the distortion loss's own chain: loss, dL_dws, then dL_dws as the given one
    gdist = rng.normal(0, 1, len(rows)).astype(F32)
    loss, wi, wti = oracle.distortion_loss_fw(o["ws"], p["dl"], p["ts"], rows)
    dws = oracle.distortion_loss_bw(gdist, wi, wti, o["ws"], p["dl"], p["ts"], rows)
    d = CR.distortion_fw(o["ws"], p["dl"], p["ts"], p["starts"], p["counts"], rel=False)
    CR.check(tag + "dist loss", loss, d["loss"], CR.bar_sum(d["scale"], lay["m"]), out)
    gw_ref, gw_scale = CR.distortion_bw(gdist, o["ws"], p["dl"], p["ts"], p["starts"], p["counts"])
    CR.check(tag + "dist dL_dws", dws, gw_ref, CR.bar_sum(gw_scale, lay["m_s"]), out)
    for name, gw in (("", None), (" (dL_dws)", gW), (" (dist chain)", dws)):
        dsig, drgb = oracle.composite_train_bw(gO, gD, gR, zero if gw is None else gw, p["sig"],
                                               p["rgbs"], o["ws"], p["dl"], p["ts"], rows,
                                               o["opacity"], o["depth"], o["rgb"], CR.THR)
        b = CR.backward(*bargs, gO_abs=gO_abs, **({} if gw is None else dict(gw=gw, ws=o["ws"])))
        CR.check(tag + "dsigma" + name, dsig, b["dsig"], CR.bar_sum(b["scale"], lay["m_s"]), out)
        CR.check(tag + "drgb", drgb, b["drgb"], CR.bar_drgb(b["drgb"], lay["k"]), out)


def test_oracle_within_bounds_rays_a(full):
    """Oracle error / bound, largest over the pool's 88 segments (printed):
    ws 0.25, opacity 0.17, depth 0.26, rgb 0.19, drgb 0.30, dsigma 0.096
    without dL_dws, 0.033 with N(0, 1) dL_dws, 0.096 with the distortion
    gradient, distortion loss 0.017, its dL_dws 0.035.  With the combine's
    folded seeds (the next test) at most 0.36; the test-time step at most 0.42."""
    out = {}
    gO, gD, gR = CR.seeds(len(full["counts"]), np.random.default_rng(8))
    _oracle_vs_bounds(full, (gO, gD, gR, gO, gD, gR, None), out)
    print("oracle / bound:", {k: f"{v:.2g}" for k, v in out.items()})
    assert max(out.values()) <= 0.5, out


@pytest.mark.parametrize("K,B", list(CR.ML_SHAPES))
def test_oracle_within_bounds_ml_seeds(pool, K, B):
    """the combine's folded seeds (fp32, the kernel's operation order) through
    the oracle against the fp64 fold with its |gO| + |bg . gRGB| scale"""
    p = CR.prepare(CR.ml_case(pool, K, B))
    CR.check_conditions(p, p["orc"]["used"], early=(K, B) == (4, 22))
    sd = CR.ml_seeds(K, B, np.random.default_rng(10 + K))
    out = {}
    for gdepth in (sd["gDepth"], None):
        gr, go, gd = CR.fold_seeds_f32(sd["gate"], sd["bg"], sd["gRGB"], sd["gO"], gdepth)
        r = CR.fold_seeds(sd["gate"], sd["bg"], sd["gRGB"], sd["gO"], gdepth)
        _oracle_vs_bounds(p, (go, gd, gr, r["gO"], r["gD"], r["gRGB"], r["gO_abs"]), out)
    print(f"K {K} B {B} oracle / bound:", {k: f"{v:.2g}" for k, v in out.items()})
    assert max(out.values()) <= 0.5, out


@pytest.mark.parametrize("n_alive", [1, 255, 257])
@pytest.mark.parametrize("n_samples", [1, 8, 64])
def test_oracle_within_bounds_test_step(n_alive, n_samples):
    c = CR.step_inputs(n_alive, n_samples, seed=100 + n_alive + n_samples)
    alive, op, de, rgb = c["alive"].copy(), c["opacity"].copy(), c["depth"].copy(), c["rgb"].copy()
    oracle.composite_test_fw(c["sig"], c["rgbs"], c["dl"], c["ts"], alive, CR.THR, c["n_eff"], op,
                             de, rgb)
    a = c["alive"]
    r = CR.composite_test(CR.alphas(c["sig"], c["dl"]), c["rgbs"], c["ts"], c["n_eff"],
                          c["opacity"][a], c["depth"][a], c["rgb"][a])
    assert np.array_equal(alive == -1, r["dead"])
    assert (c["n_eff"] == 0).any() or n_alive == 1
    assert (c["n_eff"] == n_samples).any()
    out = {}
    CR.check("opacity", op[a], r["opacity"], CR.bar_out(r["opacity"], r["m"]), out)
    CR.check("depth", de[a], r["depth"], CR.bar_out(r["depth"], r["m"]), out)
    CR.check("rgb", rgb[a], r["rgb"], CR.bar_out(r["rgb"], r["m"]), out)
    rest = np.setdiff1d(np.arange(len(op)), a)
    assert np.array_equal(op[rest], c["opacity"][rest]) and np.array_equal(rgb[rest], c["rgb"][rest])
    print(f"n_alive {n_alive} n_samples {n_samples} oracle / bound:",
          {k: f"{v:.2g}" for k, v in out.items()}, "dead", int(r["dead"].sum()))
    assert max(out.values()) <= 0.5, out


# ---------------------------------------------------------------------------
# 3. the checker flags what the absolute bar let through
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("defect", [("carry", 1), ("carry", 15), "exclusive", "nodepth"])
def test_bounds_flag_seeded_defects(full, defect):
    o, lay = full["orc"], full["lay"]
    gO, gD, gR = CR.seeds(len(full["counts"]), np.random.default_rng(8))
    args = (full["alpha"], full["rgbs"], full["dl"], full["ts"], full["starts"], full["counts"],
            o["used"], o["opacity"], o["depth"], o["rgb"], gO, gD, gR)
    good = CR.backward(*args)
    bad = CR.backward(*args, defect=defect)
    r = CR.ratios(bad["dsig"], good["dsig"], CR.bar_sum(good["scale"], lay["m_s"]))
    diff = np.abs(bad["dsig"] - good["dsig"])
    old_bar = 1e-4 * max(1.0, float(np.abs(good["dsig"]).max()))
    touched, flagged, under_old = 0, 0, 0
    for j, (a, n) in enumerate(zip(full["starts"], full["counts"])):
        if not diff[a:a + n].any():
            continue
        touched += 1
        flagged += bool(r[a:a + n].max() > 1.0)
        under_old += bool(diff[a:a + n].max() <= old_bar)
    print(f"{defect}: {touched} segments touched, {flagged} flagged by the bounds, {under_old} "
          f"of them under the old bar {old_bar:.1e}")
    assert touched >= 10 or defect == ("carry", 15)
    assert touched > 0 and flagged == touched
    assert under_old >= 1
