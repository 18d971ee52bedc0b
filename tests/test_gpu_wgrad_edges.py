"""-m gpu: the five weight-gradient entry points of csrc/conv_wgrad.hip -- df_conv_wgrad / _algo, df_conv_wgrad_bf16x3, df_upconv_wgrad /
_algo, df_upconv_wgrad_bf16x3, df_conv_s2_wgrad -- called through the raw C ABI, one row of tests/wgrad_cases.py per branch of their
host code (every kernel instantiation of the release library; tests/test_wgrad_cases_host.py keeps that complete), which the tests
through _ConvSame3 / _UpGenBlock on fresh 256-byte aligned tensors at the layers' shapes cannot reach.

Harness: every operand, output and workspace is a gpu_util.Guarded buffer.  gw, gb and the workspace hold one NaN bit pattern before
the call; the workspace is exactly as large as the entry point's *_workspace_bytes query says (whole floats, payload offset 0: the C ABI
wants it 16-byte aligned) and that value is what the call gets.  After the call: return code 0, guards intact, no NaN left in gw / gb
(so nothing was read from the workspace before it was written: NaN * 0 is NaN), inputs bit-identical, and a second call on a re-poisoned
workspace gives the same bits.

Reference: oracle/df_oracle.py::conv_same_bwd in fp64 (on upscale_nn(xc) for the up-sampling entry points, stride 2 for df_conv_s2_wgrad)
on an lrelu-distributed x, as tests/test_gpu_wgrad_staged.py.  Bounds (the suite's own): fp32 kernels relative L-inf < TOL = 2e-5 for gw
and gb; the split-operand bf16x3 kernel gw < 1e-4, gb < TOL (test_conv_bf16x3_mode).

Operand alignment (rows *_x<a>_g<b>: payload offsets in floats).  Every kernel reads x / gy through types whose natural alignment the
dispatcher must guarantee: float (4 bytes; wgrad_kernel<false, ..>, wgrad_small_n_kernel), f32x2 (8 bytes; every other streaming kernel),
f32x4 and 16-byte raw buffer loads (16 bytes: pad_rows_kernel, wgrad_wxyz_staged_kernel, wgrad_thin_mfma_kernel; the 27-point
up-sampling form is kept at 16 bytes as well).  The kernel guides say nothing that would make a vector access off its natural alignment
legal, so none is launched: the dispatcher was changed where it allowed one (staged kernel at 8 bytes; the whole fallback chain of
upconv_wgrad_impl, bf16x3 included, at 4 bytes), and the rows test the changed behaviour -- the oracle bound everywhere, the aligned
row's bits where the offset call runs the same kernel or the staged kernel's documented bit-identical twin."""
import numpy as np
import pytest
import torch

import df_oracle as orc
import wgrad_cases as wc
from gpu_util import Guarded, assert_bits, rel_linf

pytestmark = pytest.mark.gpu
TOL = 2e-5          # tests/test_gpu_layers.py::TOL
TOL_BF16X3 = 1e-4   # tests/test_gpu_layers.py::test_conv_bf16x3_mode (gw of the split-operand kernel)
EINVAL, ESHAPE, EALIGN, EWORKSPACE = -1, -2, -3, -4

ENTRY = {"conv": ("df_conv_wgrad", "df_conv_wgrad_algo"), "conv_bf16x3": ("df_conv_wgrad_bf16x3", None),
         "up": ("df_upconv_wgrad", "df_upconv_wgrad_algo"), "up_bf16x3": ("df_upconv_wgrad_bf16x3", None), "s2": ("df_conv_s2_wgrad", None)}
WS_QUERY = {"conv": "df_conv_wgrad_workspace_bytes", "conv_bf16x3": "df_conv_wgrad_workspace_bytes", "up": "df_upconv_wgrad_workspace_bytes",
            "up_bf16x3": "df_upconv_wgrad_workspace_bytes", "s2": "df_conv_s2_wgrad_workspace_bytes"}
FP32_TWIN = {"conv_bf16x3": "conv", "up_bf16x3": "up"}


@pytest.fixture(scope="module")
def k():
    """(library handle, stream)"""
    from deep_fluids_amd import _lib
    from deep_fluids_amd.ops import _stream
    return _lib.lib(), _stream()


def _kind(entry):
    return "up" if entry.startswith("up") else "s2" if entry == "s2" else "conv"


def _shapes(kind, shape, cin, cout, kz):
    """(x shape, gy shape) of an entry point whose extents argument is ``shape``"""
    B, D, H, W = shape
    if kind == "up":
        return (B, D, H, W, cin), (B, 2 * D if kz == 3 else 1, 2 * H, 2 * W, cout)
    if kind == "s2":
        return (B, 2 * D if kz == 3 else 1, 2 * H, 2 * W, cin), (B, D, H, W, cout)
    return (B, D, H, W, cin), (B, D, H, W, cout)


_CACHE = {}


def _problem(kind, shape, cin, cout, kz):
    """inputs (fp32) and the fp64 reference of one problem, computed once and shared by every row and relation that uses it; read-only"""
    key = (kind, shape, cin, cout, kz)
    if key not in _CACHE:
        xs, gs = _shapes(kind, shape, cin, cout, kz)
        rng = np.random.RandomState((sum(shape) * 131 + cin * 7 + cout * 3 + kz + len(kind)) % (2 ** 31))
        x = rng.uniform(-1, 1, xs).astype(np.float32)
        x = np.where(x > 0, x, 0.2 * x).astype(np.float32)      # lrelu-distributed input, full-mantissa values
        g = rng.uniform(-1, 1, gs).astype(np.float32)
        dw, db = _oracle(kind, x, g, kz)
        for a in (x, g, dw, db):
            a.setflags(write=False)
        _CACHE[key] = (x, g, dw, db)
    return _CACHE[key]


def _oracle(kind, x, g, kz):
    cin, cout = x.shape[-1], g.shape[-1]
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    if kz == 1:
        x64, g64 = x64[:, 0], g64[:, 0]
    if kind == "up":
        x64 = orc.upscale_nn(x64)
    nd = 3 if kz == 3 else 2
    _, dw, db = orc.conv_same_bwd(x64, np.zeros((3,) * nd + (cin, cout)), g64, stride=2 if kind == "s2" else 1, need_dx=False)
    return dw.reshape(kz * 9, cin, cout), db


class Call(object):
    """one entry-point call on Guarded buffers; keeps them alive until the results have been read"""

    def __init__(self, k, entry, shape, cin, cout, kz, algo, bias, x, g, xoff=0, goff=0):
        self.h, self.s = k
        self.entry, self.algo = entry, algo
        self.name = ENTRY[entry][0] if algo is None else ENTRY[entry][1]
        self.dims = tuple(shape) + (cin, cout, kz)
        self.nb = getattr(self.h, WS_QUERY[entry])(*self.dims)
        assert self.nb > 0 and self.nb % 4 == 0, (self.name, self.nb)
        self.x0, self.g0 = x, g
        self.X, self.G = Guarded(x.shape, x, offset=xoff), Guarded(g.shape, g, offset=goff)
        self.GW = Guarded((kz * 9, cin, cout))
        self.GB = Guarded((cout,)) if bias else None
        self.WS = Guarded((self.nb // 4,))
        assert self.WS.ptr % 16 == 0

    def raw(self, nb=None, ws_ptr=None):
        args = [self.X.ptr, self.G.ptr, self.GW.ptr, self.GB.ptr if self.GB else None] + list(self.dims)
        args += [self.WS.ptr if ws_ptr is None else ws_ptr, self.nb if nb is None else nb]
        if self.algo is not None:
            args.append(self.algo)
        rc = getattr(self.h, self.name)(*(args + [self.s]))
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        rc = self.raw()
        assert rc == 0, "%s: %s returned %d: %s" % (what, self.name, rc, self.h.df_last_error().decode())
        self.WS.check_guards(what + " workspace")
        gw = self.GW.get(what + " gw")
        gb = self.GB.get(what + " gb") if self.GB else None
        assert_bits(self.X.get(what + " x"), self.x0, what + ": x changed")
        assert_bits(self.G.get(what + " gy"), self.g0, what + ": gy changed")
        return gw, gb

    def poison(self):
        self.WS.refill(); self.GW.refill()
        if self.GB:
            self.GB.refill()

    def outputs_untouched(self):
        return self.GW.untouched() and (self.GB is None or self.GB.untouched()) and self.WS.untouched()


def _call_row(k, row, entry=None, algo="row", xoff=None, goff=None):
    rid, rentry, shape, cin, cout, kz, ralgo, bias, rx, rg = row[:10]
    x, g, dw, db = _problem(_kind(rentry), shape, cin, cout, kz)
    c = Call(k, entry or rentry, shape, cin, cout, kz, ralgo if algo == "row" else algo, bias, x, g, rx if xoff is None else xoff,
             rg if goff is None else goff)
    return c, dw, db


def _same(a, b):
    return bool((np.ascontiguousarray(a).view(np.int32) == np.ascontiguousarray(b).view(np.int32)).all())


OK_ROWS = [r for r in wc.ALL_ROWS if r[11] != "EALIGN"]


@pytest.mark.parametrize("row", OK_ROWS, ids=[r[0] for r in OK_ROWS])
def test_row_against_oracle(k, row):
    """the row's call against the fp64 oracle, twice on a poisoned workspace; bf16x3 rows against the fp32 entry point (different bits on
    the split-operand kernel -- the proof that it ran --, the same bits where the row says the mode keeps an fp32 kernel); offset rows
    against their aligned twin"""
    rid, entry, shape, cin, cout, kz, algo, bias = row[:8]
    split = row[11][0].startswith("wgrad_bf16x3_kernel")
    c, dw, db = _call_row(k, row)
    gw, gb = c.run(rid)
    ew = rel_linf(gw, dw)
    eb = rel_linf(gb, db) if bias else 0.0
    bound = TOL_BF16X3 if split else TOL
    print("%s: %s -> %s  gw %.3e (< %.0e)  gb %s (< %.0e)" % (rid, c.name, "+".join(row[11]), ew, bound, "%.3e" % eb if bias else "NULL", TOL))
    assert ew < bound and eb < TOL, (rid, ew, eb)
    # a second call on a re-poisoned workspace and re-poisoned outputs: the same bits
    c.poison()
    gw2, gb2 = c.run(rid + " (second call)")
    assert_bits(gw2, gw, rid + ": gw of the second call")
    if bias:
        assert_bits(gb2, gb, rid + ": gb of the second call")
    if entry in FP32_TWIN:
        # (algo 1 where the row names the vector-ALU thin kernel: the fp32 default there is the matrix-core form, which this mode skips)
        f, _, _ = _call_row(k, row, entry=FP32_TWIN[entry], algo=1 if row[11][0].startswith("wgrad_small_n_kernel") else 0)
        fw, fb = f.run(rid + " (fp32 entry point)")
        if split:
            assert not _same(gw, fw), rid + ": the bf16x3 entry point returned the fp32 kernel's bits -- the split-operand kernel did not run"
        else:
            assert_bits(gw, fw, rid + ": this mode keeps the fp32 kernel here")
            if bias:
                assert_bits(gb, fb, rid + ": gb, fp32 kernel")
    if row[12] is not None:
        t, _, _ = _call_row(k, wc._row(row[12][0]))
        tw, tb = t.run(rid + " (aligned twin)")
        dwv = rel_linf(gw, tw)
        print("%s: against the aligned twin %s: gw %.3e (%s)" % (rid, row[12][0], dwv, row[12][1]))
        if row[12][1] == "bits":
            assert_bits(gw, tw, rid + ": gw against the aligned call")
            if bias:
                assert_bits(gb, tb, rid + ": gb against the aligned call")


def test_bf16x3_up_entry_equals_fp32_entry_where_the_27_point_form_exists(k):
    """upconv_wgrad_impl: "both precision modes take it" -- df_upconv_wgrad_bf16x3 == df_upconv_wgrad_algo(..., 0) bit for bit"""
    row = wc._row("ubf_xyz")
    assert row[11][0].startswith("wgrad_wxyz_up_fused_kernel")
    a, _, _ = _call_row(k, row)
    b, _, _ = _call_row(k, row, entry="up", algo=0)
    (aw, ab), (bw, bb) = a.run("bf16x3"), b.run("fp32")
    assert_bits(aw, bw, "gw"); assert_bits(ab, bb, "gb")


@pytest.mark.parametrize("rid,Wp", wc.PADDED, ids=[p[0] for p in wc.PADDED])
def test_padded_row_shape_equals_the_call_on_zero_padded_copies(k, rid, Wp):
    """W = 28 | 14: conv_wgrad_impl pads x and gy to rows of Wp inside the workspace and calls ITSELF with (B, D, H, Wp, channels, kz,
    precision mode, the same algo argument); make_plan sees the same arguments as for a caller-made padded tensor and the padded copies
    are 256-byte aligned like the caller's, so the same kernel runs over the same ranges: equal bit for bit."""
    rid, entry, shape, cin, cout, kz, algo, bias = wc._row(rid)[:8]
    x, g, dw, db = _problem("conv", shape, cin, cout, kz)
    B, D, H, W = shape
    xp = np.zeros((B, D, H, Wp, cin), np.float32); xp[:, :, :, :W] = x
    gp = np.zeros((B, D, H, Wp, cout), np.float32); gp[:, :, :, :W] = g
    a = Call(k, entry, shape, cin, cout, kz, algo, bias, x, g)
    b = Call(k, entry, (B, D, H, Wp), cin, cout, kz, algo, bias, xp, gp)
    (aw, ab), (bw, bb) = a.run(rid), b.run(rid + " padded by the caller")
    print("%s: gw %.3e against the oracle" % (rid, rel_linf(aw, dw)))
    assert rel_linf(bw, dw) < TOL
    assert_bits(aw, bw, rid + " gw")
    if bias:
        assert_bits(ab, bb, rid + " gb")


@pytest.mark.parametrize("rid", wc.BATCH_ROWS)
def test_one_sample_within_a_batch_of_three(k, rid):
    """the row's problem at B = 1 (its first sample) against B = 3 with that sample in the middle and zeros around it: the same sums
    over other voxel ranges, so equal up to TOL, not bitwise"""
    rid, entry, shape, cin, cout, kz, algo, bias = wc._row(rid)[:8]
    x, g, _, _ = _problem(_kind(entry), shape, cin, cout, kz)
    x1, g1 = np.ascontiguousarray(x[:1]), np.ascontiguousarray(g[:1])
    x3 = np.zeros((3,) + x.shape[1:], np.float32); x3[1] = x1[0]
    g3 = np.zeros((3,) + g.shape[1:], np.float32); g3[1] = g1[0]
    one = Call(k, entry, (1,) + tuple(shape[1:]), cin, cout, kz, algo, bias, x1, g1)
    three = Call(k, entry, (3,) + tuple(shape[1:]), cin, cout, kz, algo, bias, x3, g3)
    (w1, b1), (w3, b3) = one.run(rid + " B=1"), three.run(rid + " B=3")
    ew = rel_linf(w3, w1)
    eb = rel_linf(b3, b1) if bias else 0.0
    bound = TOL_BF16X3 if wc._row(rid)[11][0].startswith("wgrad_bf16x3_kernel") else TOL
    print("%s: B=3 against B=1: gw %.3e (< %.0e) gb %.3e (< %.0e)" % (rid, ew, bound, eb, TOL))
    assert ew < bound and eb < TOL, (rid, ew, eb)


CONTRACT = ["stg_w32", "dir_w64", "cbf_w16", "uxyz_w16_c128", "up2_w16", "ubf_w16", "s2_w16", "thin_128_3", "pad_w28_c128"]


@pytest.mark.parametrize("rid", CONTRACT)
def test_workspace_contract(k, rid):
    """one byte less than the query's value: DF_EWORKSPACE, df_last_error names the entry point's family, nothing written;
    a workspace that is not 16-byte aligned: DF_EALIGN, nothing written"""
    row = wc._row(rid)
    c, _, _ = _call_row(k, row)
    assert c.raw(nb=c.nb - 1) == EWORKSPACE, rid
    msg = c.h.df_last_error().decode()
    family = {"conv": "df_conv_wgrad", "up": "df_upconv_wgrad", "s2": "df_conv_s2_wgrad"}[_kind(row[1])]
    assert msg.startswith(family + ":") and "workspace too small" in msg, msg
    assert c.outputs_untouched(), rid + ": written to after DF_EWORKSPACE"
    for off in (1, 2):
        assert c.raw(ws_ptr=c.WS.ptr + 4 * off) == EALIGN, (rid, off)
        assert c.h.df_last_error().decode().startswith(family + ":")
        assert c.outputs_untouched(), rid + ": written to after DF_EALIGN"


@pytest.mark.parametrize("entry,algo", [("up", None), ("up", 0), ("up", 1), ("up_bf16x3", None)])
@pytest.mark.parametrize("cin,cout", [(5, 6), (6, 7)])
def test_upconv_wgrad_refuses_odd_channel_counts(k, entry, algo, cin, cout):
    shape, kz = (1, 1, 2, 8), 1
    xs, gs = _shapes("up", shape, cin, cout, kz)
    c = Call(k, entry, shape, cin, cout, kz, algo, True, np.ones(xs, np.float32), np.ones(gs, np.float32))
    assert c.raw() == ESHAPE
    assert c.h.df_last_error().decode().startswith("df_upconv_wgrad:")
    assert c.outputs_untouched()


@pytest.mark.parametrize("Wo,cin,cout", [(12, 32, 32), (24, 32, 32), (128, 32, 32), (7, 32, 32), (16, 31, 32), (16, 32, 16)])
def test_s2_wgrad_refuses_rows_and_channels_without_a_kernel(k, Wo, cin, cout):
    """df_conv_s2_wgrad_workspace_bytes answers 0 for them, the call DF_ESHAPE whatever workspace it is given"""
    h, s = k
    dims = (1, 1, 2, Wo, cin, cout, 1)
    assert h.df_conv_s2_wgrad_workspace_bytes(*dims) == 0
    xs, gs = _shapes("s2", dims[:4], cin, cout, 1)
    X, G = Guarded(xs, np.ones(xs, np.float32)), Guarded(gs, np.ones(gs, np.float32))
    GW, GB, WS = Guarded((9, cin, cout)), Guarded((cout,)), Guarded((1 << 16,))
    rc = h.df_conv_s2_wgrad(X.ptr, G.ptr, GW.ptr, GB.ptr, *(dims + (WS.ptr, 4 << 16, s)))
    torch.cuda.synchronize()
    assert rc == ESHAPE and h.df_last_error().decode().startswith("df_conv_s2_wgrad:")
    assert GW.untouched() and GB.untouched() and WS.untouched()


EALIGN_ROWS = [r for r in wc.ALL_ROWS if r[11] == "EALIGN"]


@pytest.mark.parametrize("row", EALIGN_ROWS, ids=[r[0] for r in EALIGN_ROWS])
def test_s2_wgrad_refuses_operands_that_are_not_8_byte_aligned(k, row):
    c, _, _ = _call_row(k, row)
    assert c.raw() == EALIGN
    assert c.h.df_last_error().decode().startswith("df_conv_s2_wgrad:")
    assert c.outputs_untouched()
