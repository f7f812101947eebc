"""GPU: every composite kernel of csrc/composite.hip per sample against the fp64
restatement tests/composite_ref.py, at the derived rounding bounds (eps = 2^-24,
k the sample's 1-based index, m the segment's contributing count):

    ws (k + 2) eps w;  opacity / depth / rgb (m + 2) eps value;
    drgb (k + 3) eps |g_c w|;  dsigma, distortion loss and its dL_dws
    (m + 16) eps scale, scale = the sum of |terms| (composite_ref's docstring);
    exact zeros where the reference is exactly zero.

Termination is asserted equal to the fp32 oracle's and then taken from it; the
backward kernels get their own forward's outputs, as the chain runs them, and
the reference takes the same fp32 arrays.  Every output buffer is pre-filled
with a sentinel: an unwritten slot and a write into padding both show.  No
sample, segment or output is left out of any comparison.  tests/
test_composite_ref.py holds the fp32 oracle to half of each bound on the same
inputs and shows the bounds flag a lost carry, an exclusive prefix and a
dropped depth term that the absolute bars of test_gpu_parity.py let pass.

Each test prints its largest error / bound ratio per quantity.
"""
import numpy as np
import pytest
import torch

import composite_ref as CR
import oracle
from radnerf_amd.fused import SEG_ALIGN
from radnerf_amd._lib import lib

pytestmark = pytest.mark.gpu

SENT = -7.0
# the first rows of the rays_a tests (a partial last block of 4 waves at 1, 3, 5
# rows): 1024 at optical depth 40, the break at the last sample of 128, an
# empty segment, the flushed exponent, 1023 at optical depth 12
FIRST_ROWS = (79, 83, 0, 86, 74)


@pytest.fixture(scope="module")
def pool():
    return CR.make_segments()


@pytest.fixture(scope="module")
def full(pool):
    p = CR.prepare(CR.pack(pool))
    CR.check_conditions(p, p["orc"]["used"])
    rng = np.random.default_rng(41)
    ns = len(p["counts"])
    rest = [j for j in rng.permutation(ns) if j not in FIRST_ROWS]
    p["order"] = np.array(list(FIRST_ROWS) + rest)          # row -> segment
    p["ray"] = rng.permutation(ns)                            # segment -> ray, ray != row
    p["seeds"] = CR.seeds(ns, np.random.default_rng(8))
    p["gW"] = rng.normal(0, 1, p["cap"]).astype(np.float32)
    return p


def _dev(cuda):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    full_ = lambda shape, dtype=torch.float32: torch.full(shape, SENT, device=cuda, dtype=dtype)
    return t, full_, torch.cuda.current_stream(cuda).cuda_stream


def _report(tag, out):
    print(f"{tag} kernel / bound: " + ", ".join(f"{k} {v:.2g}" for k, v in out.items()))


def _untouched(x, keep):
    """every slot outside `keep` still holds the sentinel"""
    x = x.cpu().numpy()
    return bool((x[~keep] == SENT).all())


@pytest.mark.parametrize("with_dws", [True, False])
@pytest.mark.parametrize("n_rows", [1, 3, 5, None])
def test_train_fw_bw(cuda, full, n_rows, with_dws):
    """rn_composite_train_fw / _bw.  Measured on an MI355X over the four row
    counts: ws 0.26, opacity 0.17, depth 0.26, rgb 0.17, drgb 0.30, dsigma
    0.035 with dL_dws, 0.096 without."""
    p, L = full, lib()
    t, filled, st = _dev(cuda)
    ns = len(p["counts"])
    idx = p["order"][:ns if n_rows is None else n_rows]         # the segments of the rows
    ray = p["ray"]
    rows = CR.rows_of(p, ray)[idx]
    sig, rgbs, dl, ts, g_rows = [t(p[k]) for k in ("sig", "rgbs", "dl", "ts")] + [t(rows)]
    tot = filled((ns,), torch.int64)
    op, de, rgb, ws = filled((ns,)), filled((ns,)), filled((ns, 3)), filled((p["cap"],))
    L.composite_train_fw(sig.data_ptr(), rgbs.data_ptr(), dl.data_ptr(), ts.data_ptr(),
                         g_rows.data_ptr(), len(rows), CR.THR, tot.data_ptr(), op.data_ptr(),
                         de.data_ptr(), rgb.data_ptr(), ws.data_ptr(), st)
    used = p["orc"]["used"][idx]
    assert np.array_equal(tot.cpu().numpy()[ray[idx]], used)            # termination bit-exact
    starts, counts = p["starts"][idx], p["counts"][idx]
    lay = CR.layout(p["cap"], starts, counts, used)
    seen = np.zeros(ns, bool)
    seen[ray[idx]] = True
    for x in (tot, op, de, rgb):
        assert _untouched(x, seen)
    assert _untouched(ws, lay["inside"])
    f = CR.forward(p["alpha"], p["rgbs"], p["ts"], starts, counts, used)
    out = {}
    k_ws = np.where(lay["inside"], ws.cpu().numpy(), 0.0)
    CR.check("ws", k_ws, f["ws"], CR.bar_ws(f["ws"], lay["k"]), out)
    k_op, k_de, k_rgb = (x.cpu().numpy()[ray[idx]] for x in (op, de, rgb))
    CR.check("opacity", k_op, f["opacity"], CR.bar_out(f["opacity"], lay["m"]), out)
    CR.check("depth", k_de, f["depth"], CR.bar_out(f["depth"], lay["m"]), out)
    CR.check("rgb", k_rgb, f["rgb"], CR.bar_out(f["rgb"], lay["m"]), out)

    gO, gD, gR = (a[idx] for a in p["seeds"])
    by_ray = lambda a: np.ascontiguousarray(a[np.argsort(ray)])      # seeds are indexed by ray
    g_gO, g_gD, g_gR = (t(by_ray(a)) for a in p["seeds"])
    gW = t(p["gW"]) if with_dws else None
    dsig, drgb = filled((p["cap"],)), filled((p["cap"], 3))
    L.composite_train_bw(g_gO.data_ptr(), g_gD.data_ptr(), g_gR.data_ptr(),
                         gW.data_ptr() if with_dws else None, sig.data_ptr(), rgbs.data_ptr(),
                         ws.data_ptr(), dl.data_ptr(), ts.data_ptr(), g_rows.data_ptr(), len(rows),
                         op.data_ptr(), de.data_ptr(), rgb.data_ptr(), CR.THR, dsig.data_ptr(),
                         drgb.data_ptr(), st)
    assert _untouched(dsig, lay["inside"]) and _untouched(drgb, lay["inside"])
    kw = dict(gw=p["gW"], ws=k_ws.astype(np.float32)) if with_dws else {}
    b = CR.backward(p["alpha"], p["rgbs"], p["dl"], p["ts"], starts, counts, used, k_op, k_de,
                    k_rgb, gO, gD, gR, **kw)
    inside = lay["inside"]
    CR.check("drgb", np.where(inside[:, None], drgb.cpu().numpy(), 0.0), b["drgb"],
             CR.bar_drgb(b["drgb"], lay["k"]), out)
    CR.check("dsigma", np.where(inside, dsig.cpu().numpy(), 0.0), b["dsig"],
             CR.bar_sum(b["scale"], lay["m_s"]), out)
    _report(f"rays_a rows {len(rows)} dL_dws {with_dws}:", out)


def _ml_forward(L, cuda, p, dist):
    t, filled, st = _dev(cuda)
    K, B, cap = p["K"], p["B"], p["cap"]
    g = {k: t(p[k]) for k in ("sig", "rgbs", "dl", "ts", "counts", "starts")}
    o = dict(used=filled((K, B), torch.int32), op=filled((K, B)), de=filled((K, B)),
             rgb=filled((K, B, 3)), ws=filled((cap,)))
    args = (g["sig"].data_ptr(), g["rgbs"].data_ptr(), g["dl"].data_ptr(), g["ts"].data_ptr(),
            g["counts"].data_ptr(), g["starts"].data_ptr(), B, K, CR.THR, o["used"].data_ptr(),
            o["op"].data_ptr(), o["de"].data_ptr(), o["rgb"].data_ptr(), o["ws"].data_ptr())
    if dist:
        o["dist"] = filled((K, B))
        L.ml_composite_dist_fw(*args, o["dist"].data_ptr(), st)
    else:
        L.ml_composite_fw(*args, st)
    return g, o


def _check_ml_forward(p, o, out):
    lay, used = p["lay"], p["orc"]["used"]
    assert np.array_equal(o["used"].cpu().numpy().reshape(-1), used)        # termination bit-exact
    assert _untouched(o["ws"], lay["inside"])                                 # padding left alone
    f = CR.forward(p["alpha"], p["rgbs"], p["ts"], p["starts"], p["counts"], used)
    k = dict(ws=np.where(lay["inside"], o["ws"].cpu().numpy(), 0.0).astype(np.float32),
             op=o["op"].cpu().numpy().reshape(-1), de=o["de"].cpu().numpy().reshape(-1),
             rgb=o["rgb"].cpu().numpy().reshape(-1, 3))
    CR.check("ws", k["ws"], f["ws"], CR.bar_ws(f["ws"], lay["k"]), out)
    CR.check("opacity", k["op"], f["opacity"], CR.bar_out(f["opacity"], lay["m"]), out)
    CR.check("depth", k["de"], f["depth"], CR.bar_out(f["depth"], lay["m"]), out)
    CR.check("rgb", k["rgb"], f["rgb"], CR.bar_out(f["rgb"], lay["m"]), out)
    return k


def _ml_case(pool, K, B):
    assert CR.SEG_ALIGN == SEG_ALIGN
    p = CR.prepare(CR.ml_case(pool, K, B))
    CR.check_conditions(p, p["orc"]["used"], early=(K, B) == (4, 22))
    assert (p["starts"].reshape(K, B)[:, 0] % SEG_ALIGN == 0).all() and p["cap"] % SEG_ALIGN == 0
    sd = CR.ml_seeds(K, B, np.random.default_rng(10 + K))
    assert K * B == 1 or (sd["gate"] == 0).sum() == 1
    return p, sd


@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("K,B", list(CR.ML_SHAPES))
def test_ml_fw_bw(cuda, pool, K, B, with_depth):
    """rn_ml_composite_fw / _bw with the combine's seeds folded in the kernel.
    Measured on an MI355X over the four shapes: ws 0.26, opacity 0.17, depth
    0.26, rgb 0.17, drgb 0.36, dsigma 0.057 with gDepth, 0.074 without."""
    p, sd = _ml_case(pool, K, B)
    L = lib()
    t, filled, st = _dev(cuda)
    g, o = _ml_forward(L, cuda, p, dist=False)
    out = {}
    k = _check_ml_forward(p, o, out)
    s = {n: t(a) for n, a in sd.items()}
    dsig, drgb = filled((p["cap"],)), filled((p["cap"], 3))
    L.ml_composite_bw(s["gRGB"].data_ptr(), s["gO"].data_ptr(),
                      s["gDepth"].data_ptr() if with_depth else None, s["gate"].data_ptr(),
                      s["bg"].data_ptr(), g["sig"].data_ptr(), g["rgbs"].data_ptr(),
                      g["dl"].data_ptr(), g["ts"].data_ptr(), g["counts"].data_ptr(),
                      g["starts"].data_ptr(), o["op"].data_ptr(), o["de"].data_ptr(),
                      o["rgb"].data_ptr(), B, K, CR.THR, dsig.data_ptr(), drgb.data_ptr(), st)
    lay = p["lay"]
    assert _untouched(dsig, lay["inside"]) and _untouched(drgb, lay["inside"])
    r = CR.fold_seeds(sd["gate"], sd["bg"], sd["gRGB"], sd["gO"], sd["gDepth"] if with_depth else None)
    b = CR.backward(p["alpha"], p["rgbs"], p["dl"], p["ts"], p["starts"], p["counts"],
                    p["orc"]["used"], k["op"], k["de"], k["rgb"], r["gO"], r["gD"], r["gRGB"],
                    gO_abs=r["gO_abs"])
    inside = lay["inside"]
    CR.check("drgb", np.where(inside[:, None], drgb.cpu().numpy(), 0.0), b["drgb"],
             CR.bar_drgb(b["drgb"], lay["k"]), out)
    CR.check("dsigma", np.where(inside, dsig.cpu().numpy(), 0.0), b["dsig"],
             CR.bar_sum(b["scale"], lay["m_s"]), out)
    _report(f"ml K {K} B {B} gDepth {with_depth}:", out)


@pytest.mark.parametrize("K,B", [(2, 7), (4, 22)])
def test_ml_dist_fw_bw(cuda, pool, K, B):
    """rn_ml_composite_dist_fw / _bw (t relative to the first sample) and the
    explicit rn_distortion_loss_fw / _bw (absolute t) on the same ws.  Measured
    on an MI355X: in-chain loss 0.032, dsigma 0.057 (seed buffer and
    constant); explicit loss 0.017, its scans 0.35, dL_dws 0.027."""
    p, sd = _ml_case(pool, K, B)
    L = lib()
    t, filled, st = _dev(cuda)
    g, o = _ml_forward(L, cuda, p, dist=True)
    lay, inside, ns = p["lay"], p["lay"]["inside"], K * B
    out = {}
    k = _check_ml_forward(p, o, out)
    dist = o["dist"].cpu().numpy().reshape(-1)
    d = CR.distortion_fw(k["ws"], p["dl"], p["ts"], p["starts"], p["counts"], rel=True)
    CR.check("loss (in-chain)", dist, d["loss"], CR.bar_sum(d["scale"], lay["m"]), out)

    s = {n: t(a) for n, a in sd.items()}
    rng = np.random.default_rng(12)
    gdist = rng.normal(0, 1, ns).astype(np.float32)
    r = CR.fold_seeds(sd["gate"], sd["bg"], sd["gRGB"], sd["gO"], sd["gDepth"])
    for name, seed in (("buffer", gdist), ("constant", np.full(ns, 0.25, np.float32))):
        buf = t(seed) if name == "buffer" else None
        dsig, drgb = filled((p["cap"],)), filled((p["cap"], 3))
        L.ml_composite_dist_bw(s["gRGB"].data_ptr(), s["gO"].data_ptr(), s["gDepth"].data_ptr(),
                               buf.data_ptr() if buf is not None else None,
                               0.0 if buf is not None else 0.25, s["gate"].data_ptr(),
                               s["bg"].data_ptr(), g["sig"].data_ptr(), g["rgbs"].data_ptr(),
                               g["dl"].data_ptr(), g["ts"].data_ptr(), o["ws"].data_ptr(),
                               g["counts"].data_ptr(), g["starts"].data_ptr(), o["op"].data_ptr(),
                               o["de"].data_ptr(), o["rgb"].data_ptr(), o["dist"].data_ptr(), B, K,
                               CR.THR, dsig.data_ptr(), drgb.data_ptr(), st)
        assert _untouched(dsig, inside) and _untouched(drgb, inside)
        b = CR.backward(p["alpha"], p["rgbs"], p["dl"], p["ts"], p["starts"], p["counts"],
                        p["orc"]["used"], k["op"], k["de"], k["rgb"], r["gO"], r["gD"], r["gRGB"],
                        gO_abs=r["gO_abs"], gdist=seed, dist=dist, ws=k["ws"])
        CR.check(f"dsigma (seed {name})", np.where(inside, dsig.cpu().numpy(), 0.0), b["dsig"],
                 CR.bar_sum(b["scale"], lay["m_s"]), out)
        CR.check("drgb", np.where(inside[:, None], drgb.cpu().numpy(), 0.0), b["drgb"],
                 CR.bar_drgb(b["drgb"], lay["k"]), out)

    # the explicit form on the same ws: rows in segment order
    rows = t(CR.rows_of(p))
    e_loss, wi, wti, dws = filled((ns,)), filled((p["cap"],)), filled((p["cap"],)), filled((p["cap"],))
    L.distortion_loss_fw(o["ws"].data_ptr(), g["dl"].data_ptr(), g["ts"].data_ptr(), rows.data_ptr(),
                         ns, e_loss.data_ptr(), wi.data_ptr(), wti.data_ptr(), st)
    g_gdist = t(gdist)
    L.distortion_loss_bw(g_gdist.data_ptr(), wi.data_ptr(), wti.data_ptr(), o["ws"].data_ptr(),
                         g["dl"].data_ptr(), g["ts"].data_ptr(), rows.data_ptr(), ns, dws.data_ptr(),
                         st)
    for x in (wi, wti, dws):
        assert _untouched(x, inside)
    e = CR.distortion_fw(k["ws"], p["dl"], p["ts"], p["starts"], p["counts"], rel=False)
    CR.check("loss (explicit)", e_loss.cpu().numpy(), e["loss"], CR.bar_sum(e["scale"], lay["m"]), out)
    for name, x, ref in (("ws_incl", wi, e["ws_incl"]), ("wts_incl", wti, e["wts_incl"])):
        CR.check(name, np.where(inside, x.cpu().numpy(), 0.0), ref, CR.bar_ws(ref, lay["k"]), out)
    gw_ref, gw_scale = CR.distortion_bw(gdist, k["ws"], p["dl"], p["ts"], p["starts"], p["counts"])
    CR.check("dL_dws (explicit)", np.where(inside, dws.cpu().numpy(), 0.0), gw_ref,
             CR.bar_sum(gw_scale, lay["m_s"]), out)
    _report(f"distortion K {K} B {B}:", out)


@pytest.mark.parametrize("n_samples", [1, 8, 64])
@pytest.mark.parametrize("n_alive", [1, 255, 257])
def test_test_step(cuda, n_alive, n_samples):
    """rn_composite_test_fw: one step on prior opacity in [0, 0.9999).  Measured
    on an MI355X over the nine shapes: opacity 0.34, depth 0.42, rgb 0.42 (the
    kernel folds serially like the oracle)."""
    c = CR.step_inputs(n_alive, n_samples, seed=100 + n_alive + n_samples)
    t, _, st = _dev(cuda)
    g = {k: t(c[k]) for k in ("sig", "rgbs", "dl", "ts", "alive", "n_eff", "opacity", "depth", "rgb")}
    lib().composite_test_fw(g["sig"].data_ptr(), g["rgbs"].data_ptr(), g["dl"].data_ptr(),
                            g["ts"].data_ptr(), n_alive, n_samples, g["alive"].data_ptr(), CR.THR,
                            g["n_eff"].data_ptr(), g["opacity"].data_ptr(), g["depth"].data_ptr(),
                            g["rgb"].data_ptr(), st)
    o_alive, o_op, o_de, o_rgb = (c[k].copy() for k in ("alive", "opacity", "depth", "rgb"))
    oracle.composite_test_fw(c["sig"], c["rgbs"], c["dl"], c["ts"], o_alive, CR.THR, c["n_eff"],
                             o_op, o_de, o_rgb)
    assert np.array_equal(g["alive"].cpu().numpy(), o_alive)          # the -1 pattern, the rest kept
    a = c["alive"]
    r = CR.composite_test(CR.alphas(c["sig"], c["dl"]), c["rgbs"], c["ts"], c["n_eff"],
                          c["opacity"][a], c["depth"][a], c["rgb"][a])
    assert np.array_equal(o_alive == -1, r["dead"])
    assert (c["n_eff"] == n_samples).any() and (n_alive == 1 or (c["n_eff"] == 0).any())
    k_op, k_de, k_rgb = (g[k].cpu().numpy() for k in ("opacity", "depth", "rgb"))
    out = {}
    CR.check("opacity", k_op[a], r["opacity"], CR.bar_out(r["opacity"], r["m"]), out)
    CR.check("depth", k_de[a], r["depth"], CR.bar_out(r["depth"], r["m"]), out)
    CR.check("rgb", k_rgb[a], r["rgb"], CR.bar_out(r["rgb"], r["m"]), out)
    rest = np.setdiff1d(np.arange(len(k_op)), a)                     # rays not alive: bits kept
    for got, was in ((k_op, c["opacity"]), (k_de, c["depth"]), (k_rgb, c["rgb"])):
        assert np.array_equal(got[rest], was[rest])
    _report(f"test step n_alive {n_alive} n_samples {n_samples}:", out)
