"""No GPU: the case table of the nn, field-metric and SSIM edge tests (tests/eval_cases.py).
  * Completeness: the table reaches each of the 16 entry points the three headers declare (the size queries through the rows whose
    harness asks them), and passes the argument count the header has.
  * Branch facts: every entry of a row's ``reach`` holds when recomputed from the extents, and the facts the issue names are present
    (sk = 1 with every thread live, a chunk with sk > K, idle threads behind a ragged chunk, Z > 1024, whole column blocks, B one off the
    32 row threads, a second trip of the inference row loop, 7 and 17 workgroups of the remap, 272 tiles, OH == 32 and 33, M > 256 ...).
  * Reference run: the restatements run on every row in fp64 and in their fp32 twin; the twin is within the row's guard of fp64; the
    inputs are read-only and seeded (a second build gives the same bits); a loose row has its twin's inputs.
  * Hostile rows: non-finite values exactly where ``eval_cases.nonfinite`` says and nowhere else; everything else equal to the clean twin.
  * The rollout rows meet the drift condition of test_gpu_nn.py (tolerance < 1e-4 max|fp64|).
  * Mutations of profiles/eval_edge_tests.md that the restatement can emulate: the row named there tells the difference."""
import numpy as np
import pytest

import eval_cases as ec
import field_metrics_ref as fref
import nn_ref as R
import ssim_ref as sref
from deep_fluids_amd import _lib

F32, F64 = np.float32, np.float64
E32 = float(np.finfo(F32).eps)


def test_table_reaches_every_entry_point():
    declared = set(_lib.NN_SIGNATURES) | set(_lib.METRICS_SIGNATURES) | set(_lib.SSIM_SIGNATURES)
    assert len(_lib.NN_SIGNATURES) == 10 and len(_lib.METRICS_SIGNATURES) == 3 and len(_lib.SSIM_SIGNATURES) == 3
    named = set(ec.entry_point(r) for r in ec.ROWS) | set(ec.QUERY[r["op"]] for r in ec.ROWS if r["op"] in ec.QUERY)
    assert named == declared, sorted(named ^ declared)
    assert set(r["op"] for r in ec.ROWS) == set(ec.ENTRY) == set(ec.RULE)


def test_branch_facts_hold():
    for r in ec.ROWS:
        assert ec.facts(r) == r["reach"], (r["name"], ec.facts(r), r["reach"])
    # ---- the bn block: every B and N at least twice, the three pairs, whole blocks, B around the 32 row threads
    for op in ("bn_fwd", "bn_bwd"):
        pairs = [(r["B"], r["N"]) for r in ec.rows(op)]
        assert {(32, 32), (33, 1024), (65, 1056)} <= set(pairs)
        for B in ec.BN_B:
            assert sum(1 for p in pairs if p[0] == B) >= 2, B
        for N in ec.BN_N:
            assert sum(1 for p in pairs if p[1] == N) >= 2, N
        reach = [r["reach"] for r in ec.rows(op)]
        assert any(f["whole_blocks"] and f["col_blocks"] == 33 for f in reach) and any(f["whole_blocks"] and f["col_blocks"] == 1 for f in reach)
        assert {(1, 0), (1, 1), (2, 1), (2, 2), (3, 2)} <= set(f["row_trips"] for f in reach)      # B = 31, 32, 33, 64, 65
    assert {r["keep"] for r in ec.rows("bn_fwd")} >= {1.0, 0.5} and {r["decay"] for r in ec.rows("bn_fwd")} >= {0.0, 1.0, R.DECAY}
    assert ec.rows("bn_fwd", B=1) and ec.rows("bn_bwd", B=1) and ec.rows("bn_bwd", const_col=7)
    assert {r["hostile"][0] for r in ec.rows("bn_fwd") if r["hostile"]} == {"nan", "inf"}
    inf = {r["name"]: r["reach"] for r in ec.rows("bn_infer")}
    assert inf["bn_infer-B1025-N257"] == dict(col_blocks=2, grid_rows=1024, row_trips=2) and inf["bn_infer-B2049-N1"]["row_trips"] == 3
    # ---- elementwise
    for op in ("adv_fwd", "adv_bwd"):
        assert {r["B"] * (r["Z"] + r["P"]) for r in ec.rows(op)} >= {255, 256, 257}
        assert any(r["P"] == r["Z"] for r in ec.rows(op)) and any(r["P"] == 1 for r in ec.rows(op))
    assert any(r["i"] == r["W"] - 2 and r["W"] > 2 for r in ec.rows("adv_fwd")) and any(r["W"] == 2 for r in ec.rows("adv_fwd"))
    assert {r["null"] for r in ec.rows("adv_bwd")} == {(), ("gx",), ("gy",), ("gx", "gy")}
    assert {(r["B"] * r["Z"], r["ss"] - r["Z"], r["ds"] - r["Z"]) for r in ec.rows("rows_copy")} == {(n, s, d) for n in (255, 257) for s in (0, 1, 7)
                                                                                                  for d in (0, 1, 7)}
    for op in ("mse_fwd", "mse_bwd"):
        assert {r["n"] for r in ec.rows(op)} == set(ec.MSE_N) and ec.rows(op, same=True)
    assert ec.BY_NAME["mse_fwd-n%d" % (256 * 1024 + 1)]["reach"] == dict(blocks=257, last=1, final_trips=2)
    assert ec.offsets(ec.BY_NAME["mse_fwd-ws-off2"])["d"] == 2
    # ---- the rollout: what each row of the issue's table reaches
    ro = {r["name"][len("rollout-"):]: r for r in ec.rows("rollout")}
    assert all(r["reach"]["lds"] <= ec.LDS_LIMIT for r in ro.values())
    L = lambda n: ro[n]["reach"]["layers"]      # noqa: E731
    assert (ro["own-widths"]["N1"], ro["own-widths"]["N2"]) == (1024, 512) and L("own-widths")[0] == ((1024, 1, 0),) and L("own-widths")[1] == ((512, 2, 0),)
    assert L("second-chunk")[0][1] == (1, 1024, 0) and 1024 > ro["second-chunk"]["Z"] + ro["second-chunk"]["P"]      # sk > K: parts beyond K add nothing
    assert L("ragged-tail")[0][1] == (476, 2, 72) and L("ragged-tail")[1] == ((600, 1, 424),)
    assert ro["long-code"]["reach"]["code_trips"] == 2 and len(L("long-code")[2]) == 2
    assert ro["all-parameters"]["P"] == ro["all-parameters"]["Z"] and (ro["one-step"]["F"], ro["one-step"]["S"]) == (2, 1) and ro["scenes"]["S"] == 3
    # ---- metrics
    totals = {r["reach"]["nblk_total"]: r["reach"]["xcd"] for r in ec.rows("metrics")}
    assert totals[7] == (7, 0) and totals[17] == (1, 2)
    assert ec.BY_NAME["metrics-7x5x7"]["reach"]["nblk"] == 1 and ec.BY_NAME["metrics-1x5x59x59"]["shape"][1:] == (5, 59, 59) and 5 * 59 * 59 == 17 * 1024 - 3
    for r in ec.rows("metrics", off=0):                                     # every row runs twice
        loose = ec.BY_NAME[r["name"] + "-loose"]
        assert ec.offsets(loose) == dict(f=1, m=3, d=0) and loose["aligned"] == r["name"] and ec.offsets(r) == dict(f=0, m=0, d=0)
    for r in ec.rows("metrics"):
        m = ec.inputs(r)["mask"]
        if r["mask"]:
            assert set(np.unique(m)) >= {0, 2, 255}
    # ---- ssim
    s = {r["name"]: r for r in ec.rows("ssim")}
    assert all("ssim-%dx%d-c4" % shape in s for shape, _ in sref.SSIM_SHAPES)
    assert any(r["hostile"] and r["hostile"][0] == "nan-all" for r in ec.rows("metrics"))
    assert {(r["C"], r["off"]) for r in s.values()} >= {(1, 1), (2, 1), (3, 1), (4, 1), (4, 2)}
    assert s["ssim-42x42-c3"]["reach"]["OH"] == 32 and s["ssim-42x42-c3"]["reach"]["tiles"] == (1, 1)
    assert s["ssim-43x43-c3"]["reach"]["OH"] == 33 and s["ssim-43x43-c3"]["reach"]["last_tile"] == (1, 1)
    assert s["ssim-1x40-c3"]["reach"]["pooled"] == (1, 20) and s["ssim-40x1-c3"]["reach"]["pooled"] == (20, 1) and s["ssim-2x2-c3"]["reach"]["S"] == 2
    assert s["ssim-44x75-c3"]["reach"]["odd"] == (0, 1) and s["ssim-43x43-c3"]["reach"]["odd"] == (1, 1)
    assert {r["reach"]["S"] for r in s.values()} >= {1, 2, 3, 6, 7, 10, 11}
    big = s["ssim-554x522-c1"]["reach"]
    assert big["tiles"] == (17, 16) and big["final_trips"] == 2 and big["last_tile"] == (32, 32)
    assert any(not r["maps"] and r["pools"] for r in s.values()) and any(r["maps"] and not r["pools"] for r in s.values())
    assert {(r["G"], r["M"]) for r in ec.rows("group_mean")} == {(1, 1), (3, 5), (1, 257), (2, 300)}
    assert ec.BY_NAME["group_mean-G1-M257"]["reach"] == dict(trips=2, last=1)


def _guard(r, name, want64):
    """the largest distance the twin may have from fp64 (eval_cases.GUARD: roundings on the longest chain, in eps of the largest magnitude)"""
    if r["op"] in ("ssim", "group_mean") and name in ("ssim_map", "cs_map", "mean", "mean_cs"):
        return ec.SSIM_GUARD
    if r["op"] == "ssim":
        return 2 * E32 * float(np.abs(want64).max())                      # a pooled quad: three additions and a product by a power of two
    return ec.GUARD[r["op"]] * E32 * float(np.abs(want64).max())


@pytest.mark.parametrize("op", sorted(ec.ENTRY))
def test_reference_runs(op):
    for r in ec.rows(op):
        i = ec.inputs(r)
        again = ec._build(r)                                               # seeded: a second build gives the same bits; read-only
        for k, v in i.items():
            if isinstance(v, np.ndarray):
                assert not v.flags.writeable, (r["name"], k)
                assert v.tobytes() == again[k].tobytes(), (r["name"], k)
        if r["twin"] and not r["hostile"]:                                   # a loose row computes what its twin computes
            tw = ec.inputs(ec.BY_NAME[r["twin"]])
            assert all(v is None and tw[k] is None or v.tobytes() == tw[k].tobytes() for k, v in i.items()), r["name"]
        a, b = ec.expected(r, F32), ec.expected(r, F64)
        for name in b:
            x, y = np.asarray(a[name]), np.asarray(b[name])
            assert x.shape == y.shape, (r["name"], name)
            if y.dtype.kind != "f" or name in ("rows", "sum", "sum_cs", "sigma"):
                if name not in ("rows", "sum", "sum_cs", "sigma", "size"):
                    np.testing.assert_array_equal(x, y, err_msg="%s %s" % (r["name"], name))      # what is counted does not depend on the precision
                continue
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(y)
                assert (np.isnan(x) == np.isnan(y)).all() and (np.isinf(x) == np.isinf(y)).all(), (r["name"], name)
            if not fin.any():
                continue
            if r["op"] == "rollout":                                         # no guard in eps holds through three layers and F frames: the drift test below is the check
                continue
            d = float(np.abs(x.astype(F64) - y)[fin].max())
            print("%-34s %-14s twin - fp64 %.3e  guard %.3e" % (r["name"], name, d, _guard(r, name, y[fin])))
            assert d <= _guard(r, name, y[fin]), (r["name"], name, d)


def test_elu_sweep_walks_the_series_edges():
    r = ec.BY_NAME["bn_infer-elu-sweep"]
    i = ec.inputs(r)
    beta = ec.elu_sweep()
    with np.errstate(over="ignore"):
        pre = ((i["x"] - i["moving_mean"]) * F32(3.0)) * i["gamma"] + i["beta"]
    assert (pre.view(np.int32) == np.broadcast_to(beta, pre.shape).view(np.int32)).all()      # the pre-activation is beta, bit for bit, -0 too
    assert np.signbit(beta[1]) and beta[1] == 0 and not np.signbit(beta[0])
    assert beta[2] == np.nextafter(F32(0), F32(1)) and beta[7] == F32(-17.5) and beta[6] > beta[7] > beta[8]
    n = np.rint(beta[12:].reshape(25, 2) * F32(1.44269502))
    assert (n[:, 0] == -np.arange(1, 26)).all() and (n[:, 1] == n[:, 0] - 1).all()                                    # rintf flips between the two neighbours
    t32, t64 = ec.expected(r, F32)["out"], ec.expected(r, F64)["out"]
    assert (t32[:, beta < F32(-17.5)] == -1).all() and np.isfinite(t32).all()
    # the header: "about 2 ulp in all" of a value of magnitude at most 1, whose ulp is at most eps -- and y is beta exactly.  Not
    # nn_ref.tolerance, which is relative to this very distance: a twin that goes wrong at an edge must not widen the GPU test's bound
    worst = float(np.abs(t32.astype(F64) - t64).max())
    print("elu sweep: twin - fp64 %.3e = %.2f eps" % (worst, worst / E32))
    assert worst <= 2 * E32
    # the header's steps give +0 for both zeros: r = (y - n * c1) - n * c2 is +0 for y = -0, p = r + (r * r) * q and 1 * p + (1 - 1) too
    assert not np.signbit(t32[:, :2]).any() and (t32[:, :2] == 0).all() and (t64[:, :2] == 0).all()


@pytest.mark.parametrize("name", [r["name"] for r in ec.ROWS if r["hostile"]])
def test_hostile_rows(name):
    r = ec.BY_NAME[name]
    clean = ec.BY_NAME[r["twin"]]
    where = ec.nonfinite(r)
    for dt in (F32, F64):
        got, base = ec.expected(r, dt), ec.expected(clean, dt)
        for k, bad in where.items():
            v = np.asarray(got[k], F64)
            if np.asarray(got[k]).dtype.kind == "i":                      # an integer word: `bad` says where it differs from the clean run
                assert ((v != np.asarray(base[k], F64)) == bad).all(), (name, k)
                continue
            assert (~np.isfinite(v) == bad).all(), (name, k, int((~np.isfinite(v)).sum()), int(bad.sum()))
            np.testing.assert_array_equal(v[~bad], np.asarray(base[k], F64)[~bad], err_msg="%s %s" % (name, k))
        assert any(b.any() for b in where.values()) or r["hostile"][1] is True
    if r["op"] == "metrics":
        e, cell, k = ec.nan_cell(r["shape"])
        i, m = ec.inputs(r), ec.inputs(r)["mask"]
        assert not np.isfinite(i["g"].reshape(r["shape"][0], -1, i["g"].shape[-1])[e, cell, k])
        t = ec.expected(r, F32)
        if r["hostile"][1]:                                                # under a zero byte, its readers too: every word is the clean masked run's
            assert not m.reshape(r["shape"][0], -1)[e, ec.readers(r["shape"], cell)].any()
            np.testing.assert_array_equal(fref.raw_words(t), fref.raw_words(ec.expected(clean, F32)))
        elif r["hostile"][0] in ("nan", "nan-all"):                         # a NaN never wins `mm > m`: max_abs and argmax are the clean run's
            c = ec.expected(clean, F32)
            assert t["argmax"][e] == c["argmax"][e] != cell and t["max_abs"][e] == c["max_abs"][e] and t["count"][e] == c["count"][e]
        else:
            assert t["argmax"][e] == cell and np.isposinf(t["max_abs"][e])
    if r["op"] == "ssim":
        assert where["ssim_map"].sum() == min(r["reach"]["S"], 21) * r["reach"]["S"] and where["pool_a"].sum() == 1


@pytest.mark.parametrize("name", ec.names("rollout"))
def test_rollout_rows_meet_the_drift_condition(name):
    r = ec.BY_NAME[name]
    r32, r64 = ec.expected(r, F32)["z_out"], ec.expected(r, F64)["z_out"]
    tol = R.tolerance(r64, r32)
    print("%s: tolerance %.3e, 1e-4 max|fp64| %.3e" % (name, tol, 1e-4 * np.abs(r64).max()))
    assert tol < 1e-4 * np.abs(r64).max(), "the twin's fp32 and fp64 rollouts drifted apart: the weights are too large for this check"
    i = ec.inputs(r)                                                        # the parameter entries come from the data, exactly
    Z, P = r["Z"], r["P"]
    np.testing.assert_array_equal(r32[:, :, Z - P:], R.z_gt(i["x_test"], i["y_test"], r["S"], r["F"], Z, ec.CODE_STD, ec.OUT_STD)[:, :, Z - P:])


# ---- mutations the restatement can emulate -------------------------------------------------------------------------------------------------
class _DropsTail(R.Ops32):
    """matvec without its tail chunk: the columns behind the last whole chunk of 1024 keep the bias alone"""

    def matvec(self, v, w, b):
        out = R.Ops32.matvec(self, v, w, b)
        whole = (w.shape[1] // 1024) * 1024
        if 0 < whole < w.shape[1]:
            out[whole:] = b[whole:]
        return out


class _SkOne(R.Ops32):
    """matvec that believes sk == 1 in every chunk: the parts q >= 1 of k are never added"""

    def matvec(self, v, w, b):
        out = np.zeros(w.shape[1], F32)
        for n0, nb, sk, _ in R.matvec_chunks(*w.shape):
            acc = np.zeros(nb, F32)
            for k in range(0, w.shape[0], sk):
                acc = acc + v[k] * w[k, n0:n0 + nb]
            out[n0:n0 + nb] = acc + b[n0:n0 + nb]
        return out


@pytest.mark.parametrize("mutant,row", [(_DropsTail, "rollout-ragged-tail"), (_DropsTail, "rollout-second-chunk"), (_DropsTail, "rollout-long-code"),
                                        (_SkOne, "rollout-own-widths")])
def test_a_wrong_matvec_is_told_apart(mutant, row):
    r = ec.BY_NAME[row]
    i = ec.inputs(r)
    r32, r64 = ec.expected(r, F32)["z_out"], ec.expected(r, F64)["z_out"]
    bad = R.rollout(mutant(), {k: i[k] for k in R.NAMES}, i["x_test"], i["y_test"], r["S"], r["F"], r["Z"], ec.CODE_STD, ec.OUT_STD)
    err, tol = float(np.abs(bad.astype(F64) - r64).max()), R.tolerance(r64, r32)
    print("%s %s: |mutant - fp64| %.3e, tolerance %.3e" % (mutant.__name__, row, err, tol))
    assert err > tol


def test_elu_without_its_cut_is_told_apart():
    """without `y < -17.5 -> -1` the series runs on -1e30: s = 2^n is 0, p overflows, 0 * inf is a NaN where the row wants -1"""
    beta = ec.elu_sweep()
    y = beta[beta < F32(-17.5)]
    with np.errstate(all="ignore"):
        n = np.rint(y * F32(1.44269502))
        rr = (y - n * F32(0.693359375)) - n * F32(-2.12194440e-4)
        q = np.full_like(rr, F32(2.48015873e-5))
        for c in (1.98412698e-4, 1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5):
            q = q * rr + F32(c)
        p = rr + (rr * rr) * q
        s = np.ldexp(F32(1), np.clip(n, -200, 200).astype(np.int32)).astype(F32)
        e = s * p + (s - F32(1))
    assert np.isnan(e[y == F32(-1e30)]).all()
    assert (ec.expected(ec.BY_NAME["bn_infer-elu-sweep"], F32)["out"][0, beta == F32(-1e30)] == -1).all()


def test_a_final_sum_over_the_first_256_tiles_is_told_apart():
    """ssim_final_kernel without its stride loop adds tiles 0..255 of 272: the row's total differs in the second digit"""
    r = ec.BY_NAME["ssim-554x522-c1"]
    t = ec.expected(r, F32)
    val = t["ssim_map"]
    tiles = sref._waves                                   # the per-tile sums, by the module's own steps
    N, OH, OW = val.shape
    p = val.reshape(N, 17, 8, 4, 16, 32)
    th = np.zeros((N, 17, 8, 16, 32), F32)
    for k in range(4):
        th = th + p[:, :, :, k]
    part = tiles(th.transpose(0, 1, 3, 2, 4).reshape(N, 272, 256).astype(F64))
    np.testing.assert_array_equal(sref._strided(part), t["sum"])
    short = sref._strided(part[:, :256])
    assert abs(float(short[0] - t["sum"][0])) > 0.01 * abs(float(t["sum"][0]))
    assert F32(short[0] / t["count"]) != t["mean"][0]


def test_a_nan_that_wins_the_maximum_is_told_apart():
    """np.maximum (a NaN propagates) in place of fmaxf and `mm > m`: the NaN rows would report max_abs = NaN and its cell"""
    r = ec.BY_NAME["metrics-3x5x7x9-nan"]
    i = ec.inputs(r)
    e, cell, _ = ec.nan_cell(r["shape"])
    d = np.abs(i["g"] - i["x"]).reshape(r["shape"][0], -1, 3)
    with np.errstate(invalid="ignore"):
        m = np.maximum(np.maximum(d[..., 0], d[..., 1]), d[..., 2])
    assert np.isnan(m[e].max()) and int(np.argmax(m[e])) == cell
    t = ec.expected(r, F32)
    assert np.isfinite(t["max_abs"][e]) and t["argmax"][e] != cell
