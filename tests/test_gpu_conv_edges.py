"""-m gpu: the direct conv forward and input-gradient entry points -- df_conv_fwd (pack modes 0 and 1), df_conv_s2_fwd, df_conv_s2_dgrad,
df_upconv_fwd, df_upconv_dgrad and the bf16x3 twins, with their pack calls -- through the raw C ABI, one row of tests/conv_cases.py per
branch of the host code of csrc/conv.hip, csrc/conv_small.hip and csrc/conv_bf16.hip (every kernel instantiation of the release library:
tests/test_conv_cases_host.py keeps that complete and observes, without a GPU, which kernels each row launches).  The tests through
_ConvSame3 / _UpGenBlock / _ConvSame3S2 run on fresh 256-byte aligned tensors at the layers' shapes and never see the wide N tiles at
small sizes, the scalar-load twins, the fallbacks of the thin matrix-core kernels or a non-zero accumulator.

Harness: every operand, the packed weights and the output are gpu_util.Guarded buffers at the row's payload offsets.  The packed buffer is
exactly as large as the *_packed_elems query says and NaN before the pack call (so the pack kernel wrote all of it, padding included).
Outputs hold the NaN pattern before the call; the accumulator of df_upconv_dgrad holds seeded random data (a class that overwrote instead
of adding would lose it).  After the call: return code 0, all guards intact, no NaN left in the output, inputs and packed weights
unchanged bit for bit, and a second call gives the same bits.

Reference: oracle/df_oracle.py in fp64 -- conv_same (stride 2 for df_conv_s2_fwd, on upscale_nn(xc) for df_upconv_fwd), conv_same_bwd dx for
the mode-1 rows and df_conv_s2_dgrad, upscale_nn_bwd of that dx plus the initial acc for df_upconv_dgrad -- then the epilogue in the
kernels' order: bias, lrelu, residual, mask with the slope mask_src > 0 ? 1 : leak of the header (mask_src carries planted +0.0, -0.0 and
denormals of both signs).  Inputs are lrelu-distributed full-mantissa values, weights scaled by 1 / sqrt(taps * Cin).  Bounds (the
suite's own): fp32 kernels relative L-inf < TOL = 2e-5; bf16x3 kernels < 1e-4 and > 1e-7 (the split kernel really ran)."""
import numpy as np
import pytest
import torch

import conv_cases as cc
import df_oracle as orc
from gpu_util import Guarded, assert_bits, rel_linf

pytestmark = pytest.mark.gpu
TOL = 2e-5                          # tests/test_gpu_layers.py::TOL
BF_HI, BF_LO = 1e-4, 1e-7           # tests/test_gpu_layers.py::test_conv_bf16x3_mode
LEAK = 0.2
NAME = {"fwd": "df_conv_fwd", "fwd_bf16x3": "df_conv_fwd_bf16x3", "s2_fwd": "df_conv_s2_fwd", "s2_dgrad": "df_conv_s2_dgrad", "up_fwd": "df_upconv_fwd",
        "up_fwd_bf16x3": "df_upconv_fwd_bf16x3", "up_dgrad": "df_upconv_dgrad", "up_dgrad_bf16x3": "df_upconv_dgrad_bf16x3"}


@pytest.fixture(scope="module")
def k():
    """(library handle, stream)"""
    from deep_fluids_amd import _lib
    from deep_fluids_amd.ops import _stream
    return _lib.lib(), _stream()


def _kind(entry):
    return entry[:-7] if entry.endswith("_bf16x3") else entry


def _fine(shape, kz):
    B, D, H, W = shape
    return (B, 2 * D if kz == 3 else 1, 2 * H, 2 * W)


def _geometry(kind, shape, cin, cout, kz, mode):
    """(x shape, y shape, (weights' cin, cout))"""
    shape = tuple(shape)
    if kind == "fwd":
        return shape + (cin,), shape + (cout,), ((cin, cout) if mode == 0 else (cout, cin))
    if kind == "s2_fwd":
        return _fine(shape, kz) + (cin,), shape + (cout,), (cin, cout)
    if kind == "s2_dgrad":
        return shape + (cout,), _fine(shape, kz) + (cin,), (cin, cout)
    if kind == "up_fwd":
        return shape + (cin,), _fine(shape, kz) + (cout,), (cin, cout)
    return _fine(shape, kz) + (cout,), shape + (cin,), (cin, cout)      # up_dgrad


_CACHE = {}


def _problem(r):
    """inputs (fp32) and the fp64 result before the epilogue of one problem, computed once and shared by every row and relation that uses it;
    read-only.  Keys: x, w [taps, cin, cout], bias, residual, mask_src, acc0 (df_upconv_dgrad: the accumulator before the call), core"""
    kind, kz = _kind(r["entry"]), r["kz"]
    key = (kind, r["shape"], r["cin"], r["cout"], kz, r["mode"])
    if key in _CACHE:
        return _CACHE[key]
    xs, ys, (wci, wco) = _geometry(kind, r["shape"], r["cin"], r["cout"], kz, r["mode"])
    rng = np.random.RandomState((sum(r["shape"]) * 131 + r["cin"] * 7 + r["cout"] * 3 + kz + 17 * len(kind) + r["mode"]) % (2 ** 31))
    x = rng.uniform(-1, 1, xs).astype(np.float32)
    x = np.where(x > 0, x, 0.2 * x).astype(np.float32)      # lrelu-distributed input, full-mantissa values
    taps = 9 * kz
    w = (rng.uniform(-1, 1, (taps, wci, wco)) / np.sqrt(taps * wci)).astype(np.float32)
    p = dict(x=x, w=w, bias=rng.uniform(-0.3, 0.3, (ys[-1],)).astype(np.float32), residual=rng.uniform(-1, 1, ys).astype(np.float32),
             acc0=rng.uniform(-1, 1, ys).astype(np.float32))
    m = rng.uniform(-1, 1, ys).astype(np.float32).reshape(-1)
    plant = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45], np.float32)      # the slope is mask_src > 0 ? 1 : leak, exactly
    idx = rng.choice(m.size, size=min(m.size, 4 * plant.size), replace=False)
    m[idx] = np.resize(plant, idx.size)
    p["mask_src"] = m.reshape(ys)
    # ---- fp64 reference, before the epilogue ----
    nd = 3 if kz == 3 else 2
    sq = (lambda a: a[:, 0]) if kz == 1 else (lambda a: a)
    x64, w64 = sq(x.astype(np.float64)), w.astype(np.float64).reshape((3,) * nd + (wci, wco))
    if kind == "fwd" and r["mode"] == 0:
        core = orc.conv_same(x64, w64)
    elif kind == "fwd":
        core = orc.conv_same_bwd(np.zeros(x64.shape[:-1] + (wci,)), w64, x64, need_dx=True)[0]
    elif kind == "s2_fwd":
        core = orc.conv_same(x64, w64, stride=2)
    elif kind == "s2_dgrad":
        core = orc.conv_same_bwd(np.zeros(sq(np.empty(ys, np.bool_)).shape), w64, x64, stride=2, need_dx=True)[0]
    elif kind == "up_fwd":
        core = orc.conv_same(orc.upscale_nn(x64), w64)
    else:
        core = orc.upscale_nn_bwd(orc.conv_same_bwd(np.zeros(x64.shape[:-1] + (wci,)), w64, x64, need_dx=True)[0])
    p["core"] = core.reshape(ys)
    for a in p.values():
        a.setflags(write=False)
    _CACHE[key] = p
    return p


def _image0(p):
    """the problem of the first image alone"""
    return dict((n, a if n in ("w", "bias") else np.ascontiguousarray(a[:1])) for n, a in p.items())


def _reference(r, p):
    """the epilogue in fp64 in the kernels' order: bias, lrelu, residual, mask"""
    kind, fl = _kind(r["entry"]), r["flags"]
    v = p["core"].astype(np.float64)
    if kind in ("s2_dgrad", "up_dgrad"):
        return v + p["acc0"] if kind == "up_dgrad" else v
    if fl & cc.BIAS:
        v = v + p["bias"].astype(np.float64)
    if fl & cc.LRELU:
        v = np.maximum(v, LEAK * v)
    if fl & cc.RESIDUAL:
        v = v + p["residual"]
    if fl & cc.MASK:
        v = np.where(p["mask_src"] > 0, v, LEAK * v)
    return v


class Call(object):
    """one entry-point call on Guarded buffers (kept alive until the results have been read); the weights are packed by the entry point's
    own pack call into a buffer of exactly the queried size"""

    def __init__(self, k, r, p, entry=None, pack=True):
        self.h, self.s = k
        self.r, self.p, self.entry = r, p, entry or r["entry"]
        kind, kz, fl, off = _kind(self.entry), r["kz"], r["flags"], r["off"]
        B = p["x"].shape[0]
        self.dims = (B,) + tuple(r["shape"][1:]) + (r["cin"], r["cout"], kz)
        self.X = Guarded(p["x"].shape, p["x"], offset=off["x"])
        ys = p["core"].shape
        self.Y = Guarded(ys, p["acc0"] if kind == "up_dgrad" else None, offset=off["y"])
        takes_all = kind == "fwd"
        self.BIAS = Guarded(p["bias"].shape, p["bias"], offset=off["bias"]) if fl & cc.BIAS and "dgrad" not in kind else None
        self.RES = Guarded(ys, p["residual"], offset=off["residual"]) if fl & cc.RESIDUAL and takes_all else None
        self.MSK = Guarded(ys, p["mask_src"], offset=off["mask_src"]) if fl & cc.MASK and takes_all else None
        self.W = Guarded(p["w"].shape, p["w"])
        bf = "_bf16x3" if self.entry.endswith("bf16x3") else ""
        taps, (wci, wco) = 9 * kz, p["w"].shape[1:]
        if kind in ("fwd", "s2_fwd"):
            q, qa, pk = "df_conv_packed_elems" + bf, (taps, wci, wco, r["mode"]), "df_conv_pack_weights" + bf
        else:
            mode = 0 if kind == "up_fwd" else 2 if kind == "s2_dgrad" else 1
            q, qa, pk = "df_upconv_packed_elems" + bf, (wci, wco, kz, mode), "df_upconv_pack_weights" + bf
        self.WP = Guarded((getattr(self.h, q)(*qa) if pack else 1 << 20,), offset=off["wp"])
        self.wp_bits = None
        if pack:
            rc = getattr(self.h, pk)(*((self.W.ptr, self.WP.ptr) + qa + (self.s,)))
            torch.cuda.synchronize()
            assert rc == 0, "%s: %s returned %d: %s" % (r["id"], pk, rc, self.h.df_last_error().decode())
            self.wp_bits = self.WP.get(r["id"] + " packed weights").copy()      # guards intact, every element written

    def ptr(self, g, slot):
        return None if g is None or slot in self.r["null"] else g.ptr

    def raw(self):
        kind, fl = _kind(self.entry), self.r["flags"]
        x, wp, y = self.ptr(self.X, "x"), self.ptr(self.WP, "wp"), self.ptr(self.Y, "y")
        b, res, m = self.ptr(self.BIAS, "bias"), self.ptr(self.RES, "residual"), self.ptr(self.MSK, "mask_src")
        if kind == "fwd":
            args = (x, wp, b, res, m, y) + self.dims + (fl, LEAK)
        elif kind in ("s2_fwd", "up_fwd"):
            args = (x, wp, b, y) + self.dims + (fl, LEAK)
        else:
            args = (x, wp, y) + self.dims
        rc = getattr(self.h, NAME[self.entry])(*(args + (self.s,)))
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        rc = self.raw()
        assert rc == 0, "%s: %s returned %d: %s" % (what, NAME[self.entry], rc, self.h.df_last_error().decode())
        y = self.Y.get(what + " y")
        for g, name in ((self.X, "x"), (self.BIAS, "bias"), (self.RES, "residual"), (self.MSK, "mask_src"), (self.W, "w")):
            if g is not None:
                assert_bits(g.get(what + " " + name), self.p["w" if name == "w" else name], what + ": %s changed" % name)
        assert_bits(self.WP.get(what + " packed weights"), self.wp_bits, what + ": the packed weights changed")
        return y

    def reset(self):
        """the output back to what it held before the call"""
        if _kind(self.entry) == "up_dgrad":
            self.Y.payload().copy_(torch.from_numpy(self.p["acc0"]).cuda().reshape(-1))
        else:
            self.Y.refill()


def _split(r):
    return r["reaches"][0] == "bf16"


OK_IDS = [r["id"] for r in cc.OK_ROWS]


@pytest.mark.parametrize("rid", OK_IDS)
def test_row_against_oracle(k, rid):
    """the row's call against the fp64 oracle, twice; rows with a twin against the twin's call on the same data: the same bits where only
    VEC differs, within TOL for another kernel"""
    r = cc.by_id(rid)
    p = _problem(r)
    c = Call(k, r, p)
    y = c.run(rid)
    err = rel_linf(y, _reference(r, p))
    print("%s: %s -> %s  %.3e" % (rid, NAME[r["entry"]], "+".join(r["names"]), err))
    if _split(r):
        assert BF_LO < err < BF_HI, (rid, err)
    else:
        assert err < TOL, (rid, err)
    c.reset()
    assert_bits(c.run(rid + " (second call)"), y, rid + ": second call")
    if r["twin"]:
        t = cc.by_id(r["twin"][0])
        yt = Call(k, t, p).run(rid + " (twin %s)" % t["id"])
        if r["twin"][1] == "bits":
            assert_bits(y, yt, "%s against %s" % (rid, t["id"]))
        else:
            d = rel_linf(y, yt)
            print("%s against %s: %.3e" % (rid, t["id"], d))
            assert d < TOL, (rid, d)


@pytest.mark.parametrize("rid", cc.NARROWED + cc.TINY_BATCH)
def test_first_image_alone_gives_the_same_bits(k, rid):
    """launch_n: the narrowed N tile reads the same packed operand in the same summation order (B = 129 keeps the 128 | 64 wide tile, the
    same image alone takes the 32 wide one); conv_tiny2d_kernel: the result of an image does not depend on the batch"""
    r = cc.by_id(rid)
    p = _problem(r)
    y = Call(k, r, p).run(rid)
    y1 = Call(k, r, _image0(p)).run(rid + " B=1")
    assert_bits(y[:1], y1, rid + ": image 0 of the batch against the image alone")


@pytest.mark.parametrize("rid", [r["id"] for r in cc.OK_ROWS if r["entry"] == "s2_dgrad" and r["form"] == 0])
def test_generic_s2_dgrad_is_upconv_fwd_on_the_mode2_operand(k, rid):
    """df_conv_s2_dgrad without a live-tap form (channel counts, or a gy that is not 16-byte aligned) == df_upconv_fwd(gy, wp(mode 2), NULL, gx,
    ..., Cin := Cout, Cout := Cin, kz, 0, 0) as the header states it, bit for bit"""
    r = cc.by_id(rid)
    p = _problem(r)
    a = Call(k, r, p)
    y = a.run(rid)
    h, s = k
    a.reset()
    rc = h.df_upconv_fwd(a.X.ptr, a.WP.ptr, None, a.Y.ptr, *(a.dims[:4] + (r["cout"], r["cin"], r["kz"], 0, 0.0, s)))
    torch.cuda.synchronize()
    assert rc == 0, h.df_last_error().decode()
    assert_bits(a.Y.get(rid + " df_upconv_fwd"), y, rid)


ERR_IDS = [r["id"] for r in cc.ERR_ROWS]


@pytest.mark.parametrize("rid", ERR_IDS)
def test_error_row_returns_its_code_and_writes_nothing(k, rid):
    r = cc.by_id(rid)
    safe = dict(r, shape=tuple(max(v, 1) for v in r["shape"]), cin=r["cin"] if r["cin"] > 0 else 32, cout=r["cout"] if r["cout"] > 0 else 32, kz=3)
    xs, ys, (wci, wco) = _geometry(_kind(r["entry"]), safe["shape"], safe["cin"], safe["cout"], 3, 0)
    p = dict(x=np.ones(xs, np.float32), w=np.ones((27, wci, wco), np.float32), bias=np.ones((ys[-1],), np.float32), residual=np.ones(ys, np.float32),
             mask_src=np.ones(ys, np.float32), acc0=None, core=np.empty(ys, np.bool_))
    c = Call(k, r, p, pack=False)
    c.Y = Guarded(ys, offset=r["off"]["y"])      # NaN also where the entry point would accumulate
    c.dims = tuple(r["shape"]) + (r["cin"], r["cout"], r["kz"])
    rc = c.raw()
    msg = c.h.df_last_error().decode()
    assert rc == r["reaches"], (rid, rc, msg)
    assert msg.startswith(NAME[r["entry"]].replace("_bf16x3", "")), msg
    assert c.Y.untouched() and c.WP.untouched(), rid + ": written to after an error"
