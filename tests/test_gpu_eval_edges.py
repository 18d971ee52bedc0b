"""-m gpu: the entry points of csrc/nn.hip (df_nn_*), csrc/metrics.hip (df_field_metrics*) and csrc/ssim.hip (df_ssim*) through the raw
C ABI, one row of tests/eval_cases.py per call (tests/test_eval_cases_host.py keeps the table complete against the three headers, checks
the branch each row states it reaches, and runs the restatements on every row without a GPU).  The feature tests (test_gpu_nn.py,
test_gpu_field_metrics.py, test_gpu_ssim.py) run on 256-byte aligned tensors, at the widths 16 / 8 and 80 / 40, on finite values.  They do
not see a record at a 4-byte aligned address, a second column chunk or a ragged one in the rollout, a code longer than the workgroup, a
whole number of column blocks, a second trip of a row or tile loop, the block counts 7 and 17 of the remap, C = 4, a pooled image one
pixel high, or what a NaN does to a maximum.

Harness: every operand and every output is a guarded buffer (gpu_util.Guarded, GuardedBytes) at the row's payload offset; outputs hold
the fill before the call.  After the call: return code 0, all guards intact (inputs too), the inputs unchanged bit for bit, and a second
call from the same state gives the same bits.  Nothing here relies on the device faulting.

Reference, no tolerance of its own: bit for bit the fp32 twin wherever the header fixes the order (a NaN must be a NaN; its payload is
the hardware's); nn_ref.tolerance against fp64 for everything behind an ELU (act / out, the inference block, the rollout).
profiles/eval_edge_tests.md holds the measured maxima.

Relations, all exact: a loose row gives the bits of its aligned twin; a hostile row gives the bits of its clean twin wherever
eval_cases.nonfinite does not name the element; a scene alone gives the bits of the scene in its batch; an absent output changes nothing."""
import ctypes

import numpy as np
import pytest
import torch

import eval_cases as ec
import field_metrics_ref as fref
import nn_ref as R
import ssim_ref as sref
from gpu_util import NAN_BITS, Guarded, GuardedBytes, host

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EPS32 = float(np.finfo(F32).eps)
RATIOS = {}                         # op -> (worst distance / bound under the tolerance rule, row): printed by the last test


def _lib():
    from deep_fluids_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scalar(a):
    return float(a) if isinstance(a, (np.floating, float)) else (int(a) if isinstance(a, np.integer) else a)


def _rc(name, *args):
    """the entry point's return code, nothing raised"""
    L = _lib()
    return getattr(L._handle(name), name)(*([_scalar(a) for a in args] + [_stream()]))


class Bufs(object):
    """the guarded buffers of one call"""

    def __init__(self, r):
        self.r, self.b, self.data = r, {}, {}
        self.off = ec.offsets(r)

    def inp(self, name, arr, off=None):
        arr = np.ascontiguousarray(arr, F32)
        self.b[name] = Guarded(arr.shape, arr, self.off["f"] if off is None else off)
        self.data[name] = arr
        return self.b[name].ptr

    def inout(self, name, arr):
        self.b[name] = Guarded(arr.shape, np.ascontiguousarray(arr, F32), self.off["f"])
        return self.b[name].ptr

    def out(self, name, shape, off=None):
        self.b[name] = Guarded(shape, None, self.off["f"] if off is None else off)
        return self.b[name].ptr

    def call(self, name, *args):
        rc = _rc(name, *args)
        assert rc == 0, (self.r["name"], rc, _lib().lib().df_last_error())
        return self.done()

    def done(self):
        """guards intact, inputs unchanged -> {name: the payload's int32 words} of everything that is not a pure input"""
        torch.cuda.synchronize()
        for n, g in self.b.items():
            g.check_guards("%s %s" % (self.r["name"], n))
        for n, a in self.data.items():
            got = self.b[n].raw() if isinstance(self.b[n], Guarded) else host(self.b[n].payload()).reshape(a.shape)
            assert (got == (a.view(np.int32) if a.dtype == F32 else a)).all(), "%s: the input %s was changed" % (self.r["name"], n)
        return dict((n, g.raw().copy()) for n, g in self.b.items() if n not in self.data)


def _same_bits(what, words, want):
    """bit for bit; where the twin holds a NaN the kernel must hold one (the payload is the hardware's); no fill left"""
    want = np.ascontiguousarray(want, F32)
    assert words.shape == want.shape, (what, words.shape, want.shape)
    assert not (words == np.int32(NAN_BITS)).any(), "%s: %d elements were never written" % (what, int((words == np.int32(NAN_BITS)).sum()))
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(words.view(F32)), words != want.view(np.int32))
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, at,
                                                                                             words.view(F32)[at], want[at]))


def _close(r, what, words, ref64, twin32):
    """nn_ref.tolerance: 4 x the twin's own deviation from fp64, floored at 4 roundings; non-finite values must agree exactly"""
    got = words.view(F32).astype(F64)
    assert not (words == np.int32(NAN_BITS)).any(), "%s: elements were never written" % what
    ref64, twin32 = np.asarray(ref64, F64), np.asarray(twin32, F64)
    fin = np.isfinite(ref64)
    assert (np.isnan(got) == np.isnan(ref64)).all() and (got[~fin & ~np.isnan(ref64)] == ref64[~fin & ~np.isnan(ref64)]).all(), what
    if not fin.any():
        return
    tol = R.tolerance(ref64[fin], twin32[fin])
    err = float(np.abs(got[fin] - ref64[fin]).max())
    print("%-34s %-8s |gpu - fp64| %.3e  tolerance %.3e" % (r["name"], what, err, tol))
    if err / tol > RATIOS.get(r["op"], (0.0, ""))[0]:
        RATIOS[r["op"]] = (err / tol, r["name"])
    assert err <= tol, (r["name"], what, err, tol)


# ---- one call per op: -> {output: int32 words} -----------------------------------------------------------------------------------------------
def _exec(r, i):
    op, b = r["op"], Bufs(r)
    if op == "bn_fwd":
        B, N = r["B"], r["N"]
        return b.call(ec.ENTRY[op], b.inp("x", i["x"]), b.inp("gamma", i["gamma"]), b.inp("beta", i["beta"]), b.inout("moving_mean", i["moving_mean"]),
                      b.inout("moving_var", i["moving_var"]), b.out("act", (B, N)), b.out("out", (B, N)), b.out("mean", (N,)), b.out("rstd", (N,)), B, N,
                      ec.EPS, r["decay"], r["keep"], ec.SEED, ec.STEP, ec.WINDOW, 1)
    if op == "bn_bwd":
        B, N = r["B"], r["N"]
        return b.call(ec.ENTRY[op], *([b.inp(n, i[n]) for n in ("x", "act", "gout", "gamma", "mean", "rstd")] +
                                      [b.out("gx", (B, N)), b.out("ggamma", (N,)), b.out("gbeta", (N,)), B, N, r["keep"], ec.SEED, ec.STEP, ec.WINDOW, 1]))
    if op == "bn_infer":
        B, N = r["B"], r["N"]
        return b.call(ec.ENTRY[op], *([b.inp(n, i[n]) for n in ("x", "gamma", "beta", "moving_mean", "moving_var")] + [b.out("out", (B, N)), B, N, ec.EPS]))
    if op == "adv_fwd":
        return b.call(ec.ENTRY[op], b.inp("x", i["x"]), b.inp("y", i["y"]), b.inp("xw", i["xw"]), b.out("x_next", i["x"].shape), r["B"], r["W"], r["Z"],
                      r["P"], r["i"], ec.RATIO)
    if op == "adv_bwd":
        g = b.inp("gx_next", i["gx_next"])
        gx, gy = b.out("gx", i["gx_next"].shape), b.out("gy", (r["B"], r["Z"]))      # an absent output: the buffer exists and is not passed
        got = b.call(ec.ENTRY[op], g, None if "gx" in r["null"] else gx, None if "gy" in r["null"] else gy, r["B"], r["Z"], r["P"], ec.RATIO)
        for n in r["null"]:
            assert b.b[n].untouched(), "%s: %s was not passed and was written" % (r["name"], n)
            del got[n]
        return got
    if op == "rows_copy":
        B, Z = r["B"], r["Z"]
        return b.call(ec.ENTRY[op], b.inp("src", i["src"]), r["ss"], b.out("dst", ((B - 1) * r["ds"] + Z,)), r["ds"], B, Z)
    if op == "mse_fwd":
        need = _lib().query(ec.QUERY[op], r["n"])
        assert need == 8 * r["reach"]["blocks"]
        got = b.call(ec.ENTRY[op], b.inp("a", i["a"]), b.inp("b", i["b"]), r["n"], b.out("out", (1,)), b.out("ws", (need // 4,), b.off["d"]), need)
        del got["ws"]
        return got
    if op == "mse_bwd":
        return b.call(ec.ENTRY[op], b.inp("a", i["a"]), b.inp("b", i["b"]), b.inp("gout", i["gout"]), b.out("ga", (r["n"],)), r["n"])
    if op == "rollout":
        order = ["x_test", "y_test"] + [R.NAMES[k] for k in (0, 1, 3, 2, 4, 5, 6, 7, 9, 8, 10, 11, 12, 13)]      # w, b, gamma, beta, mm, mv per layer
        return b.call(ec.ENTRY[op], *([b.inp(n, i[n]) for n in order] + [b.out("z_out", (r["S"], r["F"], r["Z"])), r["S"], r["F"], r["Z"], r["P"],
                                                                         r["N1"], r["N2"], ec.EPS, ec.CODE_STD, ec.OUT_STD]))
    if op == "metrics":
        shape = r["shape"]
        D = len(shape) - 1
        ext = (1,) * (4 - len(shape)) + shape[1:]
        need = _lib().query(ec.QUERY[op], D, shape[0], *ext)
        assert need == 80 * r["reach"]["nblk_total"]
        mask = i["mask"]
        mp = None
        if mask is not None:
            b.b["mask"] = GuardedBytes(mask.shape, np.array(mask), b.off["m"])
            b.data["mask"] = mask
            mp = b.b["mask"].ptr
        got = b.call(ec.entry_point(r), b.inp("g", i["g"]), b.inp("x", i["x"]), mp, 0 if mask is None else int(mask.ndim == len(shape)),
                     b.out("out", (shape[0], fref.WORDS)), b.out("ws", (need // 4,), b.off["d"]), need, *shape)
        del got["ws"]
        return got
    if op == "ssim":
        N, (H, W), C = r["N"], r["shape"], r["C"]
        S, sigma = ec.ssim_sigma(r)
        taps = (ctypes.c_float * S)(*[float(v) for v in sref.taps(S, sigma, F32)])
        need = _lib().query(ec.QUERY[op], N, H, W, r["filter_size"])
        f = r["reach"]
        assert need == 16 * N * f["tiles"][0] * f["tiles"][1]
        a, bb = b.inp("a", i["a"]), b.inp("b", i["b"])
        maps = [b.out(n, (N, f["OH"], f["OW"])) for n in ("ssim_map", "cs_map")]
        pools = [b.out(n, (N,) + f["pooled"] + (C,)) for n in ("pool_a", "pool_b")]
        absent = ([] if r["maps"] else ["ssim_map", "cs_map"]) + ([] if r["pools"] else ["pool_a", "pool_b"])
        d = sref.DEFAULTS
        got = b.call(ec.ENTRY[op], a, bb, ctypes.cast(taps, ctypes.c_void_p), *((maps if r["maps"] else [None, None]) + (pools if r["pools"] else [None, None]) +
                                                                            [b.out("out", (N, sref.WORDS), 0), b.out("ws", (need // 4,), 0), need, N, H, W, C,
                                                                             r["filter_size"], d["k1"], d["k2"], d["min_val"], d["max_val"]]))
        for n in absent:
            assert b.b[n].untouched(), "%s: %s was not passed and was written" % (r["name"], n)
            del got[n]
        del got["ws"]
        return got
    if op == "group_mean":
        G, M = r["G"], r["M"]
        rows = _exec(ec.group_mean_ssim_row(r), i)["out"]                                          # the rows df_ssim writes for G * M images of 11 x 11
        src = Guarded(rows.shape, None, 0)
        src.bits[src.lo:src.lo + src.n] = torch.from_numpy(rows.reshape(-1)).cuda()
        b.b["mean"] = Guarded((G, 4), None, 0)
        rc = _rc(ec.ENTRY[op], src.ptr, b.b["mean"].ptr, G, M)
        assert rc == 0, (r["name"], rc)
        got = b.done()
        src.check_guards("rows")
        assert (src.raw() == rows).all()
        return dict(got, rows=rows)
    raise KeyError(op)


_RESULTS = {}


def _run(r):
    """the row on the device, twice from the same state: the second call must repeat the first.  Returns the outputs of the first."""
    if r["name"] not in _RESULTS:
        first, second = _exec(r, ec.inputs(r)), _exec(r, ec.inputs(r))
        for n in first:
            assert (first[n] == second[n]).all(), "%s: the second call changed %s" % (r["name"], n)
        _RESULTS[r["name"]] = first
    return _RESULTS[r["name"]]


def _equal(a, b, what):
    assert set(a) == set(b), what
    for n in a:
        assert a[n].shape == b[n].shape and (a[n] == b[n]).all(), "%s: %s differs in %d elements" % (what, n, int((a[n] != b[n]).sum()))


def _check(r):
    got = _run(r)
    t32, t64 = ec.expected(r, F32), ec.expected(r, F64)
    for n, words in got.items():
        what = "%s %s" % (r["name"], n)
        if ec.RULE[r["op"]] == "tolerance" or n in ec.TOLERANCE_OUTPUTS.get(r["op"], ()):
            _close(r, n, words, t64[n], t32[n])
        elif r["op"] == "rows_copy":                                         # the gaps still hold the fill
            gap = np.isnan(t32[n])
            assert (words[gap] == np.int32(NAN_BITS)).all(), "%s: %d gap elements of dst were written" % (what, int((words[gap] != np.int32(NAN_BITS)).sum()))
            assert gap.sum() == (r["B"] - 1) * r["reach"]["gap"]
            _same_bits(what, words[~gap], t32[n][~gap])
        else:
            _same_bits(what, words, t32[n])
    return got, t32


def _hostile(r, got, outputs):
    """non-finite exactly where eval_cases.nonfinite says; every other element has the bits of the clean twin's run"""
    clean = _run(ec.BY_NAME[r["twin"]])
    for n, bad in ec.nonfinite(r).items():
        if n not in outputs:
            continue
        a, c = outputs[n](got), outputs[n](clean)
        if a.dtype.kind == "i":
            assert ((a != c) == bad).all(), (r["name"], n)
            continue
        assert (~np.isfinite(a) == bad).all(), "%s %s: %d non-finite elements, %d expected" % (r["name"], n, int((~np.isfinite(a)).sum()), int(bad.sum()))
        assert (a.view(np.int32 if a.dtype == F32 else np.int64)[~bad] == c.view(np.int32 if c.dtype == F32 else np.int64)[~bad]).all(), \
            "%s %s: an element away from the poison differs from the clean run" % (r["name"], n)


# ---- nn ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.names("bn_fwd") + ec.names("bn_bwd"))
def test_bn_block(name):
    r = ec.BY_NAME[name]
    got, t32 = _check(r)
    if r["op"] == "bn_fwd":                                                # the mask pattern: exact whatever the ELU gives
        kept = ec.inputs(r)["kept"]
        act, out = got["act"].view(F32), got["out"]
        assert (out[~kept] == 0).all(), name + ": a dropped element is not +0"
        inv = F32(1) / F32(r["keep"])
        with np.errstate(invalid="ignore"):
            want = (act[kept] * inv)
        ok = np.where(np.isnan(want), np.isnan(out.view(F32)[kept]), out[kept] == want.view(np.int32))
        assert ok.all(), name + ": a kept element is not act * inv"
        if r["keep"] == 1.0:
            assert kept.all() and (out == got["act"]).all()
        if r["decay"] == 1.0:
            assert (got["moving_mean"] == ec.inputs(r)["moving_mean"].view(np.int32)).all()
        if r["B"] == 1:
            assert (got["rstd"].view(F32) == F32(1.0 / np.sqrt(F64(F32(ec.EPS))))).all()
        if r["hostile"]:
            _hostile(r, got, {n: (lambda g, n=n: g[n].view(F32)) for n in ("act", "out", "mean", "rstd", "moving_mean", "moving_var")})
    if r["const_col"] is not None and r["op"] == "bn_fwd":
        c = r["const_col"]
        assert got["rstd"].view(F32)[c] == F32(1.0 / np.sqrt(F64(F32(ec.EPS)))) and got["mean"].view(F32)[c] == F32(0.75)


@pytest.mark.parametrize("name", ec.names("bn_infer"))
def test_bn_infer(name):
    r = ec.BY_NAME[name]
    got, t32 = _check(r)
    if r["sweep"]:
        out, beta = got["out"].view(F32), ec.elu_sweep()
        assert (out[:, beta < F32(-17.5)] == -1).all(), "below -17.5 the header says -1 exactly"
        assert (got["out"][:, :2] == 0).all(), "elu(+-0) is +0 by the header's steps: %r" % (out[:, :2],)
        assert (out[:, beta > 0].view(np.int32) == beta[beta > 0].view(np.int32)).all()      # y > 0 is y, the smallest subnormal too
        print("%s: %d of %d elements differ from the twin in a bit" % (name, int((got["out"] != t32["out"].view(np.int32)).sum()), out.size))


@pytest.mark.parametrize("name", ec.names("adv_fwd") + ec.names("adv_bwd") + ec.names("rows_copy") + ec.names("mse_fwd") + ec.names("mse_bwd"))
def test_window_step_rows_copy_and_mse(name):
    r = ec.BY_NAME[name]
    got, t32 = _check(r)
    if r["op"] == "adv_bwd":
        assert set(got) == {"gx", "gy"} - set(r["null"])
    if r.get("same"):
        assert not got["out" if r["op"] == "mse_fwd" else "ga"].any(), name + ": a == b gives exactly +0"
    if r["twin"]:
        _equal(got, _run(ec.BY_NAME[r["twin"]]), "%s against %s" % (name, r["twin"]))


@pytest.mark.parametrize("name", ec.names("rollout"))
def test_rollout(name):
    r = ec.BY_NAME[name]
    got, t32 = _check(r)
    i, Z, P = ec.inputs(r), r["Z"], r["P"]
    z = got["z_out"].view(F32)
    np.testing.assert_array_equal(z[:, :, Z - P:], R.z_gt(i["x_test"], i["y_test"], r["S"], r["F"], Z, ec.CODE_STD, ec.OUT_STD)[:, :, Z - P:])
    if r["S"] == 3:                                                        # each scene alone gives the bits of the scene in the batch
        F = r["F"]
        for s in range(3):
            one = dict(i, x_test=i["x_test"][s * (F - 1):(s + 1) * (F - 1)], y_test=i["y_test"][s * (F - 1):(s + 1) * (F - 1)])
            alone = _exec(dict(r, name="%s/scene%d" % (name, s), S=1), one)["z_out"]
            assert (alone[0] == got["z_out"][s]).all(), "%s: scene %d depends on its batch" % (name, s)


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.names("metrics"))
def test_field_metrics(name):
    r = ec.BY_NAME[name]
    raw = _run(r)["out"]
    t32, t64 = ec.expected(r, F32), ec.expected(r, F64)
    want = fref.raw_words(t32)
    for q in fref.INTS + fref.MAXES + fref.SUMS:
        w = fref.WORD[q]
        nan = np.isnan(t32[q]) if q not in fref.INTS else np.zeros(len(raw), bool)
        ok = np.where(nan, np.isnan(raw[:, w].view(F32)), raw[:, w] == want[:, w])
        assert ok.all(), "%s %s: got %r, twin %r" % (name, q, raw[:, w].view(F32) if q not in fref.INTS else raw[:, w], t32[q])
    rest = [w for w in range(fref.WORDS) if w not in fref.WORD.values()]
    assert not raw[:, rest].any(), name + ": a reserved word is not 0"
    if not r["hostile"]:                                                   # and the feature test's second rule: 4 x the twin's own deviation from fp64
        for q in fref.SUMS:
            e_gpu, e_twin = np.abs(raw[:, fref.WORD[q]].view(F32).astype(F64) - t64[q]), np.abs(t32[q].astype(F64) - t64[q])
            assert (e_gpu <= 4 * e_twin).all(), (name, q)
    if r["off"]:
        _equal(dict(out=raw), dict(out=_run(ec.BY_NAME[r["aligned"]])["out"]), "%s against %s" % (name, r["aligned"]))
    if r["hostile"]:
        word = lambda q: (lambda g: g["out"][:, fref.WORD[q]] if q in fref.INTS else g["out"][:, fref.WORD[q]].view(F32))      # noqa: E731
        _hostile(r, dict(out=raw), {q: word(q) for q in fref.INTS + fref.MAXES + fref.SUMS})
        if r["hostile"][1]:                                                # under a zero byte: every word is the clean masked run's
            assert (raw == _run(ec.BY_NAME[r["twin"]])["out"]).all()


# ---- ssim --------------------------------------------------------------------------------------------------------------------------------------
def _ssim_fields(rows):
    c = sref.CONST
    f64 = lambda w: np.ascontiguousarray(rows[:, w:w + 2]).view(F64)[:, 0]      # noqa: E731
    return dict(mean=rows[:, c["mean"]].view(F32), mean_cs=rows[:, c["mean_cs"]].view(F32), sum=f64(c["sum"]), sum_cs=f64(c["sum_cs"]))


@pytest.mark.parametrize("name", ec.names("ssim"))
def test_ssim(name):
    r = ec.BY_NAME[name]
    got = _run(r)
    t32 = ec.expected(r, F32)
    for n in (["ssim_map", "cs_map"] if r["maps"] else []) + (["pool_a", "pool_b"] if r["pools"] else []):
        _same_bits("%s %s" % (name, n), got[n], t32[n])
    assert set(got) == {"out"} | ({"ssim_map", "cs_map"} if r["maps"] else set()) | ({"pool_a", "pool_b"} if r["pools"] else set())
    rows, want = got["out"], sref.raw_words(t32)
    assert not (rows == np.int32(NAN_BITS)).any(), name + ": a word of out was never written"
    f, w = _ssim_fields(rows), _ssim_fields(want)
    assert (rows[:, [sref.CONST["count"], 3]] == want[:, [sref.CONST["count"], 3]]).all()
    for k in f:
        nan = np.isnan(w[k])
        assert np.where(nan, np.isnan(f[k]), f[k].view(np.int32 if f[k].dtype == F32 else np.int64) == w[k].view(np.int32 if f[k].dtype == F32 else np.int64)).all(), \
            "%s %s: got %r, twin %r" % (name, k, f[k], w[k])
    if r["twin"] and not r["hostile"]:                                     # a loose row, an absent output: the bits of the twin's run
        tw = _run(ec.BY_NAME[r["twin"]])
        _equal(got, {n: tw[n] for n in got}, "%s against %s" % (name, r["twin"]))
    if r["hostile"]:
        outs = {n: (lambda g, n=n: g[n].view(F32)) for n in ("ssim_map", "cs_map", "pool_a", "pool_b")}
        outs.update({k: (lambda g, k=k: _ssim_fields(g["out"])[k]) for k in ("mean", "mean_cs", "sum", "sum_cs")})
        _hostile(r, got, outs)


@pytest.mark.parametrize("name", ec.names("group_mean"))
def test_ssim_group_mean(name):
    r = ec.BY_NAME[name]
    got = _run(r)
    t32 = ec.expected(r, F32)
    np.testing.assert_array_equal(got["rows"], t32["rows"])                 # the rows df_ssim wrote are the twin's
    mean = np.ascontiguousarray(got["mean"]).view(F64)
    np.testing.assert_array_equal(mean.view(np.int64), np.ascontiguousarray(t32["mean"]).view(np.int64))      # the fixed-order fp64 sum, bit for bit


# ---- refusals the feature tests lack -------------------------------------------------------------------------------------------------------
def _refused(name, code, bufs, *args):
    rc = _rc(name, *args)
    assert rc == code, (name, rc, code, _lib().lib().df_last_error())
    torch.cuda.synchronize()
    for g in bufs:
        assert g.untouched(), "%s: a refused call wrote to a buffer" % name


def test_refusals_alignment():
    L = _lib()
    n = 64
    t = [Guarded((n,)) for _ in range(17)]
    p = [g.ptr for g in t]
    bwd = p[:9] + [4, 8, 0.5, 1, 2, 3, 0]
    inf = p[:6] + [4, 8, R.EPS]
    adv = p[:4] + [2, 2, 2, 1, 0, 0.5]
    adb = p[:3] + [2, 2, 1, 0.5]
    roll = p[:17] + [1, 2, 2, 1, 4, 4, R.EPS, 1.0, 1.0]
    for name, args, ptrs in (("df_nn_bn_elu_dropout_bwd", bwd, 9), ("df_nn_bn_elu_infer", inf, 6), ("df_nn_window_advance_fwd", adv, 4),
                             ("df_nn_window_advance_bwd", adb, 3), ("df_nn_rollout", roll, 17)):
        for k in range(ptrs):                                              # a 2-byte-misaligned float pointer, operand by operand
            _refused(name, L.DF_EALIGN, t, *(args[:k] + [args[k] + 2] + args[k + 1:]))
    for k in (0, 2):
        _refused("df_nn_rows_copy", L.DF_EALIGN, t, *[p[0] + (2 if k == 0 else 0), 3, p[1] + (2 if k == 2 else 0), 3, 2, 3])
    for k in (0, 1, 3):
        a = [p[0], p[1], 16, p[2], p[3], 8]
        a[k] += 2
        _refused("df_nn_mse_fwd", L.DF_EALIGN, t, *a)
    for k in range(4):
        a = p[:4] + [16]
        a[k] += 2
        _refused("df_nn_mse_bwd", L.DF_EALIGN, t, *a)
    # ---- metrics: g, x, out at 2 bytes; the 8-byte workspace at 4
    big = [Guarded((2 * 4 * 5 * 6 * 3,)) for _ in range(2)] + [Guarded((2 * 16,)), Guarded((2 * 20,))]
    g, x, out, ws = [b.ptr for b in big]
    m3 = lambda g, x, out, ws: [g, x, None, 0, out, ws, 160, 2, 4, 5, 6]      # noqa: E731
    for a in (m3(g + 2, x, out, ws), m3(g, x + 2, out, ws), m3(g, x, out + 2, ws), m3(g, x, out, ws + 4)):
        _refused("df_field_metrics3d", L.DF_EALIGN, big, *a)
    _refused("df_field_metrics2d", L.DF_EALIGN, big, g, x, None, 0, out, ws + 4, 80, 1, 4, 5)
    # ---- ssim: images, maps, pools at 2 bytes; out, ws and mean at 4
    N, H, W, C = 1, 12, 17, 1
    s = [Guarded((N * H * W * C,)) for _ in range(2)] + [Guarded((N * 2 * 7,)) for _ in range(2)] + [Guarded((N * 6 * 9 * C,)) for _ in range(2)] + \
        [Guarded((8,)), Guarded((4,))]
    taps = (ctypes.c_float * 11)(*[float(v) for v in sref.taps(11, 1.5, F32)])
    tp = ctypes.cast(taps, ctypes.c_void_p)
    base = [g_.ptr for g_ in s]
    ss = lambda q: [q[0], q[1], tp, q[2], q[3], q[4], q[5], q[6], q[7], 16, N, H, W, C, 11, 0.01, 0.03, -1.0, 1.0]      # noqa: E731
    for k in range(8):
        q = list(base)
        q[k] += 2 if k < 6 else 4
        _refused("df_ssim", L.DF_EALIGN, s, *ss(q))
    _refused("df_ssim_group_mean", L.DF_EALIGN, s, base[6] + 4, base[7], 1, 1)
    _refused("df_ssim_group_mean", L.DF_EALIGN, s, base[6], base[7] + 4, 1, 1)


def test_refusals_overlap():
    """every pair the two libraries list: out / ws against each other and against every input (metrics); any two buffers of which one is
    written (ssim; a against b is allowed: both are read)"""
    L = _lib()
    B, Z, Y, X = 2, 4, 5, 6
    n = B * Z * Y * X
    # one allocation per role with room to slide the others into it
    g, x, out, ws = Guarded((3 * n,)), Guarded((3 * n,)), Guarded((B * 16 + 64,)), Guarded((B * 20 + 64,))
    mask = GuardedBytes((n + 256,))
    allb = [g, x, out, ws]
    ok = dict(g=g.ptr, x=x.ptr, mask=mask.ptr, out=out.ptr, ws=ws.ptr)
    call = lambda a: [a["g"], a["x"], a["mask"], 1, a["out"], a["ws"], 160, B, Z, Y, X]      # noqa: E731
    for moved, onto in (("out", "ws"), ("ws", "out"), ("out", "g"), ("out", "x"), ("out", "mask"), ("ws", "g"), ("ws", "x"), ("ws", "mask")):
        a = dict(ok)
        a[moved] = ok[onto] + 8                                            # inside the other buffer, 8-byte aligned
        _refused("df_field_metrics3d", L.DF_EINVAL, allb, *call(a))
        assert b"overlaps" in L.lib().df_last_error()
        assert bool((mask.bits == mask.fill).all())
    a = dict(ok, out=ok["g"] + 8)
    _refused("df_field_metrics2d", L.DF_EINVAL, allb, a["g"], a["x"], None, 0, a["out"], a["ws"], 80, 1, 4, 5)
    # ---- ssim
    N, H, W, C = 1, 12, 17, 1
    sizes = dict(a=N * H * W * C, b=N * H * W * C, ssim_map=14, cs_map=14, pool_a=54, pool_b=54, out=8, ws=4)
    order = ["a", "b", "ssim_map", "cs_map", "pool_a", "pool_b", "out", "ws"]
    bufs = {k: Guarded((3 * v + 8,)) for k, v in sizes.items()}
    taps = (ctypes.c_float * 11)(*[float(v) for v in sref.taps(11, 1.5, F32)])
    tp = ctypes.cast(taps, ctypes.c_void_p)
    args = lambda q: [q["a"], q["b"], tp, q["ssim_map"], q["cs_map"], q["pool_a"], q["pool_b"], q["out"], q["ws"], 16, N, H, W, C, 11, 0.01, 0.03,      # noqa: E731
                      -1.0, 1.0]
    ok = {k: v.ptr for k, v in bufs.items()}
    pairs = 0
    for i_, u in enumerate(order):
        for v in order[i_ + 1:]:
            if (u, v) == ("a", "b"):
                continue
            q = dict(ok)
            q[v] = ok[u] + 8                                               # v starts inside u
            _refused("df_ssim", L.DF_EINVAL, list(bufs.values()), *args(q))
            assert b"overlaps" in L.lib().df_last_error(), (u, v)
            pairs += 1
    assert pairs == 27
    assert _rc("df_ssim", *args(dict(ok, b=ok["a"]))) == 0                  # a against itself: both are read
    torch.cuda.synchronize()
    for k in ("a", "b"):
        assert bufs[k].untouched()
    rows, mean = Guarded((16,)), Guarded((8,))
    _refused("df_ssim_group_mean", L.DF_EINVAL, [rows, mean], rows.ptr, rows.ptr + 8, 1, 1)


def test_rollout_lds_bound_from_both_sides():
    """2 Z + P + 2 N1 + 2 N2 = 15361 is refused with DF_ESHAPE before any launch; 15360 runs (one scene, one step)"""
    L = _lib()
    Z, N1, N2 = 7000, 400, 279
    for P, code in ((3, L.DF_ESHAPE), (2, 0)):
        assert 2 * Z + P + 2 * N1 + 2 * N2 == (15361 if code else 15360)
        sizes = [(Z + P,), (Z,), (Z + P, N1), (N1,), (N1,), (N1,), (N1,), (N1,), (N1, N2), (N2,), (N2,), (N2,), (N2,), (N2,), (N2, Z), (Z,), (2, Z)]
        if code:
            t = [Guarded((8,)) for _ in sizes]                            # refused on the extents alone: nothing is read
            _refused("df_nn_rollout", code, t, *([g.ptr for g in t] + [1, 2, Z, P, N1, N2, R.EPS, 1.0, 1.0]))
            assert b"LDS" in L.lib().df_last_error()
            continue
        rng = np.random.RandomState(5)
        t = [Guarded(s, rng.uniform(0.5, 1.5, s) if len(s) == 1 else rng.uniform(-0.01, 0.01, s)) for s in sizes[:-1]] + [Guarded(sizes[-1])]
        assert _rc("df_nn_rollout", *([g.ptr for g in t] + [1, 2, Z, P, N1, N2, R.EPS, 1.0, 1.0])) == 0
        torch.cuda.synchronize()
        for g in t:
            g.check_guards("rollout at the LDS bound")
        assert np.isfinite(t[-1].get("z_out at the LDS bound")).all()


def test_zz_report():
    """(last in the file) the worst distance / bound per op under the tolerance rule, for profiles/eval_edge_tests.md"""
    for op, (ratio, row) in sorted(RATIOS.items()):
        print("%-10s worst |gpu - fp64| / tolerance %.3f  (%s)" % (op, ratio, row))
    print("%d rows on the device" % len(_RESULTS))
