"""-m gpu: the Winograd conv entry points -- the seven df_wino_* forms, df_wino43_conv, df_wino2d_conv_fwd / _upconv_fwd / _upconv_dgrad,
df_wino2d43_conv / _conv_bits / _conv_addup_bits and the backward tails df_lrelu_bits_bwd_pool2x / df_lrelu_words2d_bwd_pool2x -- through the
raw C ABI, one row of tests/wino_cases.py per branch of the host code and of the epilogues of csrc/conv_wino.hip, conv_wino43.hip,
conv_wino2d.hip and conv_wino2d43.hip (every kernel instantiation of the release library: tests/test_wino_cases_host.py keeps that complete
and observes, without a GPU, what each row launches).  The tests through _ConvSame3 / _GenBlock / _UpGenBlock run on fresh 256-byte aligned
tensors at six shapes per dimensionality; the C-ABI tests of the fused epilogues compare one kernel with another.  Neither sees an operand at a
4-byte aligned address, a write outside a buffer, the run-time-flags instantiation with DF_CONV_ADDUP, a worker that walks a second tile block
while others do not, or an image smaller than a tile.

Harness: every operand, the packed weights, the sign words and every output is a gpu_util.Guarded buffer at the row's payload offset.  The
packed buffer is exactly as large as the *_packed_elems query says and NaN before the pack call; the sign-word buffer exactly
*_signbits_bytes.  Outputs hold the NaN pattern before the call; the accumulator of the two *_upconv_dgrad entries holds seeded random data.
After the call: return code 0, all guards intact, no NaN left in any output, inputs and packed weights unchanged bit for bit, and a second
call gives the same bits.

Reference: oracle/df_oracle.py in fp64 -- conv_same, conv_same_bwd dx for the mode-1 (dgrad) rows, conv_same on upscale_nn(xc) for the
up-sampling forward, upscale_nn_bwd of that dx plus the initial acc for the pooled adjoint -- then the epilogue in the header's order: bias,
lrelu, residual, mask with the slope mask_src > 0 ? 1 : leak (mask_src carries planted +0.0, -0.0 and denormals of both signs), and for
ADDUP y2 = y + upscale_nn(xc).  Inputs are lrelu-distributed full-mantissa values, weights scaled by 1 / sqrt(taps * Cin).  Bound: relative
L-inf < TOL = 2e-5, the suite's own (tests/test_gpu_layers.py::TOL), for all four families; profiles/wino_edge_tests.md holds the measured
maxima.

Relations, all exact: sign words decode to (y > 0) of the kernel's OWN output; an entry point that does not write y gives the words and the y2
of the twin that does; MASK from mask words gives the bits of MASK from the fp32 activation the words were taken from; a loose-operand row
gives the bits of its aligned twin; image 0 of a multi-pass batch gives the bits of image 0 alone; the backward tails on words give the bits of
df_lrelu_bwd_pool2x on the fp32 activation."""
import numpy as np
import pytest
import torch

import df_oracle as orc
import wino_cases as wc
from gpu_util import Guarded, assert_bits, rel_linf

pytestmark = pytest.mark.gpu
TOL = 2e-5                          # tests/test_gpu_layers.py::TOL
LEAK = 0.2
# per kernel family: the size query and the pack call of its weights
PACK = {"wino3d": ("df_wino_packed_elems", "df_wino_pack_weights"), "wino43": ("df_wino43_packed_elems", "df_wino43_pack_weights"),
        "wino2d": ("df_wino2d_packed_elems", "df_wino2d_pack_weights"), "wino2d43": ("df_wino2d43_packed_elems", "df_wino2d43_pack_weights")}
# per entry point: its pointer arguments in order (slots of wc.SLOTS), whether flags / leak follow the channel counts
SIG = {"wino_fwd": ("x wp bias res msrc y", True, True), "wino_fwd_bits": ("x wp bias mbits y sbits", True, True),
       "wino_fwd_addup": ("x wp bias res y y2", False, True), "wino_fwd_addup_bits": ("x wp bias res y2 sbits", False, True),
       "wino_upconv_fwd": ("x wp bias y", True, True), "wino_upconv_fwd_bits": ("x wp bias y sbits", False, True),
       "wino_upconv_dgrad": ("x wp y", False, False), "wino43": ("x wp bias res msrc mbits y y2 sbits", True, True),
       "w2_fwd": ("x wp bias res msrc y", True, True), "w2_up_fwd": ("x wp bias y", True, True), "w2_up_dgrad": ("x wp y", False, False),
       "w2_43": ("x wp bias res msrc y", True, True), "w2_43_bits": ("x wp bias mbits y sbits", True, True),
       "w2_43_addup_bits": ("x wp bias res y2 sbits", False, True)}
# the epilogue of the entry points that take no flags argument
FIXED_FLAGS = {"wino_fwd_addup": 25, "wino_fwd_addup_bits": 25, "w2_43_addup_bits": 25, "wino_upconv_fwd_bits": 9, "wino_upconv_dgrad": 0, "w2_up_dgrad": 0}
# the forward conv that writes the sign words of a family (the 2-D F(2,3)^2 family has none)
WORDS_FWD = {"wino3d": "wino_fwd_bits", "wino43": "wino43", "wino2d43": "w2_43_bits"}


@pytest.fixture(scope="module")
def k():
    """(library handle, stream)"""
    from deep_fluids_amd import _lib
    from deep_fluids_amd.ops import _stream
    return _lib.lib(), _stream()


def _flags(r):
    return FIXED_FLAGS.get(r["entry"], r["flags"])


def _geometry(entry, shape, cin, cout, mode):
    """(x shape, y shape, coarse shape of the add-up operand, the layer's (cin, cout), pack mode) of a call"""
    form = wc.ENTRIES[entry]["form"]
    B, dims = shape[0], tuple(shape[1:])
    fine, half = tuple(2 * v for v in dims), tuple(max(v // 2, 1) for v in dims)
    if form == "up_fwd":
        return (B,) + dims + (cin,), (B,) + fine + (cout,), None, (cin, cout), 0
    if form == "up_dgrad":
        return (B,) + fine + (cout,), (B,) + dims + (cin,), None, (cin, cout), 1
    return (B,) + dims + (cin,), (B,) + dims + (cout,), (B,) + half + (cout,), ((cin, cout) if mode == 0 else (cout, cin)), mode


_CACHE = {}


def _problem(r):
    """inputs (fp32) and the fp64 result before the epilogue of one problem, computed once and shared by every row and relation that uses it;
    read-only.  Keys: x, w [taps, cin, cout], bias, res (fine), xc (coarse), msrc, acc0 (the accumulator of an *_upconv_dgrad before the call), core"""
    e = wc.ENTRIES[r["entry"]]
    form = "conv" if e["form"] == "addup" else e["form"]
    key = (form, r["shape"], r["cin"], r["cout"], r["mode"])
    if key in _CACHE:
        return _CACHE[key]
    xs, ys, cs, (wci, wco), _ = _geometry(r["entry"], r["shape"], r["cin"], r["cout"], r["mode"])
    nd = e["nd"]
    rng = np.random.RandomState((sum(r["shape"]) * 131 + r["cin"] * 7 + r["cout"] * 3 + nd + 17 * len(form) + r["mode"]) % (2 ** 31))
    x = rng.uniform(-1, 1, xs).astype(np.float32)
    x = np.where(x > 0, x, 0.2 * x).astype(np.float32)      # lrelu-distributed input, full-mantissa values
    taps = 3 ** nd
    w = (rng.uniform(-1, 1, (taps, wci, wco)) / np.sqrt(taps * wci)).astype(np.float32)
    p = dict(x=x, w=w, bias=rng.uniform(-0.3, 0.3, (ys[-1],)).astype(np.float32), res=rng.uniform(-1, 1, ys).astype(np.float32),
             acc0=rng.uniform(-1, 1, ys).astype(np.float32))
    if cs is not None:
        p["xc"] = rng.uniform(-1, 1, cs).astype(np.float32)
    m = rng.uniform(-1, 1, ys).astype(np.float32).reshape(-1)
    plant = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45], np.float32)      # the slope is mask_src > 0 ? 1 : leak, exactly
    idx = rng.choice(m.size, size=min(m.size, 16 * plant.size), replace=False)      # (enough to land in the ragged blocks of an image too)
    m[idx] = np.resize(plant, idx.size)
    p["msrc"] = m.reshape(ys)
    # ---- fp64 reference, before the epilogue ----
    x64, w64 = x.astype(np.float64), w.astype(np.float64).reshape((3,) * nd + (wci, wco))
    if form == "conv" and r["mode"] == 0:
        core = orc.conv_same(x64, w64)
    elif form == "conv":
        core = orc.conv_same_bwd(np.zeros(x64.shape[:-1] + (wci,)), w64, x64, need_dx=True)[0]
    elif form == "up_fwd":
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


def _reference(r, p, msrc):
    """{"y", "y2"}: the epilogue in fp64 in the header's order -- bias, lrelu, residual, mask -- then y2 = y + upscale_nn(xc)"""
    fl, form = _flags(r), wc.ENTRIES[r["entry"]]["form"]
    v = p["core"].astype(np.float64)
    if form == "up_dgrad":
        return {"y": v + p["acc0"]}
    if fl & wc.BIAS:
        v = v + p["bias"].astype(np.float64)
    if fl & wc.LRELU:
        v = np.maximum(v, LEAK * v)
    if fl & wc.RESIDUAL:
        v = v + p["res"]
    if fl & wc.MASK:
        v = np.where(msrc > 0, v, LEAK * v)
    out = {"y": v}
    if fl & wc.ADDUP:
        out["y2"] = v + orc.upscale_nn(p["xc"].astype(np.float64))
    return out


def _signbits_bytes(h, nd, ys):
    return (h.df_wino_signbits_bytes if nd == 3 else h.df_wino2d43_signbits_bytes)(*ys)


def _decode(words, nd, ys):
    """the sign words (an int32 device tensor) -> (activation > 0) as a host bool array of shape ys"""
    from deep_fluids_amd import ops
    if nd == 3:
        return ops.sign_bits_to_mask(words, ys[:4], ys[4]).cpu().numpy()
    return ops.sign_words2d_to_mask(words, (ys[0], 1, ys[1], ys[2]), ys[3]).cpu().numpy()


class Call(object):
    """one entry-point call on Guarded buffers (kept alive until the results have been read); the weights are packed by the family's own pack
    call into a buffer of exactly the queried size.  msrc / mbits: the mask operands where they are not the problem's own"""

    def __init__(self, k, r, p, pack=True, msrc=None, mbits=None):
        self.h, self.s = k
        self.r, self.p = r, p
        e = self.e = wc.ENTRIES[r["entry"]]
        ops, off, B = r["ops"], r["off"], p["x"].shape[0]
        self.shape = (B,) + tuple(r["shape"][1:])
        ys, (wci, wco), mode = tuple(p["core"].shape), p["w"].shape[1:], (1 if e["form"] == "up_dgrad" else r["mode"])
        self.ys, self.nd = ys, e["nd"]
        addup = bool(_flags(r) & wc.ADDUP) or e["form"] == "addup"
        self.inputs = {"x": p["x"], "bias": p["bias"], "res": p["xc"] if addup else p["res"], "msrc": p["msrc"] if msrc is None else msrc}
        self.g = {}
        for slot in ("x", "bias", "res", "msrc"):
            if ops & (1 << wc.SLOTS.index(slot)):
                self.g[slot] = Guarded(self.inputs[slot].shape, self.inputs[slot], offset=off[slot])
        nwords = _signbits_bytes(self.h, self.nd, ys) // 4 if pack else 1 << 16
        if ops & wc.MBITS:
            self.inputs["mbits"] = mbits if mbits is not None else np.zeros((nwords,), np.float32)
            self.g["mbits"] = Guarded((nwords,), self.inputs["mbits"], offset=off["mbits"])
        for slot in ("y", "y2"):
            if ops & (1 << wc.SLOTS.index(slot)):
                self.g[slot] = Guarded(ys, p["acc0"] if e["form"] == "up_dgrad" and pack else None, offset=off[slot])
        if ops & wc.SBITS:
            self.g["sbits"] = Guarded((nwords,), offset=off["sbits"])
        q, pk = PACK[e["fam"]]
        self.W = Guarded(p["w"].shape, p["w"])
        self.g["wp"] = Guarded((getattr(self.h, q)(wci, wco, mode) if pack else 1 << 16,), offset=off["wp"])
        self.wp_bits = None
        if pack:
            rc = getattr(self.h, pk)(self.W.ptr, self.g["wp"].ptr, wci, wco, mode, self.s)
            torch.cuda.synchronize()
            assert rc == 0, "%s: %s returned %d: %s" % (r["id"], pk, rc, self.h.df_last_error().decode())
            self.wp_bits = self.g["wp"].get(r["id"] + " packed weights").copy()      # guards intact, every element written

    def raw(self, dims=None):
        r = self.r
        order, has_flags, has_leak = SIG[r["entry"]]
        args = [self.g[s].ptr if (r["ops"] & (1 << wc.SLOTS.index(s))) and s in self.g else None for s in order.split()]
        args += list(dims if dims is not None else self.shape + (r["cin"], r["cout"]))
        args += ([r["flags"]] if has_flags else []) + ([LEAK] if has_leak else []) + [self.s]
        rc = getattr(self.h, self.e["fn"])(*args)
        torch.cuda.synchronize()
        return rc

    def run(self, what):
        """{"y", "y2": host arrays, "sbits": the words as an int32 device tensor} of the outputs the call has"""
        rc = self.raw()
        assert rc == 0, "%s: %s returned %d: %s" % (what, self.e["fn"], rc, self.h.df_last_error().decode())
        out = {}
        for slot in ("y", "y2"):
            if slot in self.g:
                out[slot] = self.g[slot].get("%s %s" % (what, slot))
        if "sbits" in self.g:
            self.g["sbits"].check_guards(what + " sign words")
            out["sbits"] = self.g["sbits"].bits[self.g["sbits"].lo:self.g["sbits"].lo + self.g["sbits"].n].clone()
        for slot in ("x", "bias", "res", "msrc", "mbits"):
            if slot in self.g:
                self.g[slot].check_guards("%s %s" % (what, slot))
                got = self.g[slot].payload().cpu().numpy().reshape(self.inputs[slot].shape)
                assert_bits(got, self.inputs[slot], "%s: %s changed" % (what, slot))
        assert_bits(self.W.get(what + " w"), self.p["w"], what + ": w changed")
        assert_bits(self.g["wp"].get(what + " packed weights"), self.wp_bits, what + ": the packed weights changed")
        return out

    def reset(self):
        """the outputs back to what they held before the call"""
        for slot in ("y", "y2", "sbits"):
            if slot in self.g:
                self.g[slot].refill()
        if self.e["form"] == "up_dgrad":
            self.g["y"].payload().copy_(torch.from_numpy(np.array(self.p["acc0"])).cuda().reshape(-1))


_ACT = {}


def _activation(k, fam, shape, cout):
    """(activation fp32, its sign words as a float32-typed host array) of a forward conv 32 -> cout of this family on `shape`: the mask of a
    dgrad on words, the activation behind a backward tail.  Computed once per (family, shape, cout)."""
    key = (fam, tuple(shape), cout)
    if key not in _ACT:
        entry = WORDS_FWD[fam]
        r = dict(id="activation-%s-%s-%d" % key, entry=entry, shape=tuple(shape), cin=32, cout=cout, flags=9, mode=0, ops=wc.ops_of(entry, 9, "s"),
                 off=dict((s, 0) for s in wc.SLOTS))
        c = Call(k, r, _problem(r))
        out = c.run(r["id"])
        assert np.array_equal(_decode(out["sbits"], c.nd, c.ys), out["y"] > 0), r["id"]
        _ACT[key] = (out["y"], out["sbits"].view(torch.float32).cpu().numpy())
    return _ACT[key]


def _masks(k, r, p):
    """the mask operands of a row on mask words: (fp32 activation, its words)"""
    if not (r["ops"] & wc.MBITS):
        return None, None
    B = p["x"].shape[0]
    return _activation(k, wc.ENTRIES[r["entry"]]["fam"], (B,) + tuple(r["shape"][1:]), r["cout"])


def _run_row(k, r, p, what):
    act, words = _masks(k, r, p)
    c = Call(k, r, p, msrc=act, mbits=words)
    return c, c.run(what), act


def _same_outputs(a, b, what):
    for slot in ("y", "y2"):
        if slot in a and slot in b:
            assert_bits(a[slot], b[slot], "%s: %s" % (what, slot))
    if "sbits" in a and "sbits" in b:
        assert bool((a["sbits"] == b["sbits"]).all()), what + ": sign words"


CONV_IDS = [r["id"] for r in wc.OK_ROWS if wc.ENTRIES[r["entry"]]["form"] != "tail"]


@pytest.mark.parametrize("rid", CONV_IDS)
def test_row_against_oracle(k, rid):
    """the row's call against the fp64 oracle, twice; its sign words against its own output; rows with a twin against the twin's call on the
    same data: the same bits"""
    r = wc.by_id(rid)
    p = _problem(r)
    c, out, act = _run_row(k, r, p, rid)
    ref = _reference(r, p, act if act is not None else p["msrc"])
    for slot in ("y", "y2"):
        if slot in out:
            err = rel_linf(out[slot], ref[slot])
            print("WINO_EDGE %s %s %s %s %.3e" % (rid, c.e["fn"], "/".join(str(v) for v in r["reaches"]), slot, err))
            assert err < TOL, (rid, slot, err)
    if "sbits" in out and "y" in out:
        assert np.array_equal(_decode(out["sbits"], c.nd, c.ys), out["y"] > 0), rid + ": the sign words are not (y > 0) of the kernel's own y"
    c.reset()
    _same_outputs(c.run(rid + " (second call)"), out, rid + ": second call")
    if r["twin"]:
        t = wc.by_id(r["twin"])
        ct = Call(k, t, p, msrc=act)
        tout = ct.run("%s (twin %s)" % (rid, t["id"]))
        common = [s for s in ("y", "y2") if s in out and s in tout]
        assert common, rid
        for slot in common:
            assert_bits(out[slot], tout[slot], "%s against %s: %s" % (rid, t["id"], slot))
        if "sbits" in out and "y" not in out and "y" in tout:      # an entry point that does not write y: the words of the twin's y
            assert np.array_equal(_decode(out["sbits"], c.nd, c.ys), tout["y"] > 0), "%s: sign words against y of %s" % (rid, t["id"])
        if "sbits" in out and "sbits" in tout:
            assert bool((out["sbits"] == tout["sbits"]).all()), "%s against %s: sign words" % (rid, t["id"])


def test_2d_addup_on_words_is_the_conv_on_words_plus_the_coarse_tensor(k):
    """df_wino2d43_conv_addup_bits writes no y and has no twin that writes both: its words are those of df_wino2d43_conv_bits on the same data,
    its y2 that y plus nearest_up2x(xc) (one fp32 addition per element), as the header promises"""
    for rid in [r["id"] for r in wc.OK_ROWS if r["entry"] == "w2_43_addup_bits" and not r["mis"]]:
        r = wc.by_id(rid)
        p = _problem(r)
        out = Call(k, r, p).run(rid)
        t = dict(r, entry="w2_43_bits", flags=9, ops=wc.ops_of("w2_43_bits", 9, "s"))
        tout = Call(k, t, p).run(rid + " (df_wino2d43_conv_bits)")
        assert bool((out["sbits"] == tout["sbits"]).all()), rid + ": sign words"
        assert_bits(out["y2"], tout["y"] + orc.upscale_nn(p["xc"]), rid + ": y2")


@pytest.mark.parametrize("rid", wc.MULTIPASS)
def test_first_image_alone_gives_the_same_bits(k, rid):
    """a worker's second tile block (the double-buffer parity carried over, the prefetched halo, the last decode) computes what a first one does:
    image 0 of the batch -- more than one pass of the grid -- against the same image alone, one pass"""
    r = wc.by_id(rid)
    p = _problem(r)
    y = Call(k, r, p).run(rid)["y"]
    y1 = Call(k, r, _image0(p)).run(rid + " B=1")["y"]
    assert_bits(y[:1], y1, rid + ": image 0 of the batch against the image alone")


TAIL_IDS = [r["id"] for r in wc.OK_ROWS if wc.ENTRIES[r["entry"]]["form"] == "tail"]


@pytest.mark.parametrize("rid", TAIL_IDS)
def test_backward_tail_on_words(k, rid):
    """gx = gy * (bit ? 1 : leak) and gpool = the 2 x 2 (x 2) sum-pool of gy from the sign words of a forward conv: against fp64 computed from the
    DECODED words (gx: one fp32 rounding, gpool: a 4- or 8-term sum) and, bit for bit, against df_lrelu_bwd_pool2x on the fp32 activation"""
    h, s = k
    r = wc.by_id(rid)
    e, C, nd = wc.ENTRIES[r["entry"]], r["cin"], wc.ENTRIES[r["entry"]]["nd"]
    B, cd = r["shape"][0], tuple(r["shape"][1:])
    fine = (B,) + tuple(2 * v for v in cd)
    act, words = _activation(k, ("wino43" if C == 96 else "wino3d") if nd == 3 else "wino2d43", fine, C)
    rng = np.random.RandomState(sum(r["shape"]) * 31 + C)
    gy = rng.uniform(-1, 1, fine + (C,)).astype(np.float32)
    GY, WORDS = Guarded(gy.shape, gy), Guarded(words.shape, words)
    GX, GP = Guarded(gy.shape), Guarded((B,) + cd + (C,))
    rc = getattr(h, e["fn"])(GY.ptr, WORDS.ptr, GX.ptr, GP.ptr, LEAK, *(r["shape"] + (C, s)))
    torch.cuda.synchronize()
    assert rc == 0, h.df_last_error().decode()
    gx, gp = GX.get(rid + " gx"), GP.get(rid + " gpool")
    assert_bits(GY.get(rid + " gy"), gy, rid + ": gy changed")
    mask = _decode(WORDS.bits[WORDS.lo:WORDS.lo + WORDS.n].clone(), nd, fine + (C,))
    assert np.array_equal(mask, act > 0), rid
    egx = rel_linf(gx, np.where(mask, gy.astype(np.float64), LEAK * gy.astype(np.float64)))
    egp = rel_linf(gp, orc.upscale_nn_bwd(gy.astype(np.float64)))
    print("WINO_EDGE %s %s %s gx %.3e\nWINO_EDGE %s %s %s gpool %.3e" % (rid, e["fn"], e["fam"], egx, rid, e["fn"], e["fam"], egp))
    assert egx < TOL and egp < TOL, (rid, egx, egp)
    ACT, GX2, GP2 = Guarded(act.shape, act), Guarded(gy.shape), Guarded((B,) + cd + (C,))
    rc = h.df_lrelu_bwd_pool2x(GY.ptr, ACT.ptr, GX2.ptr, GP2.ptr, LEAK, B, cd[0] if nd == 3 else 1, cd[-2], cd[-1], C, int(nd == 3), s)
    torch.cuda.synchronize()
    assert rc == 0, h.df_last_error().decode()
    assert_bits(gx, GX2.get(rid + " gx of df_lrelu_bwd_pool2x"), rid + ": gx against the fp32-mask twin")
    assert_bits(gp, GP2.get(rid + " gpool of df_lrelu_bwd_pool2x"), rid + ": gpool against the fp32-mask twin")


ERR_IDS = [r["id"] for r in wc.ERR_ROWS]


@pytest.mark.parametrize("rid", ERR_IDS)
def test_error_row_returns_its_code_and_writes_nothing(k, rid):
    h, s = k
    r = wc.by_id(rid)
    e = wc.ENTRIES[r["entry"]]
    safe = tuple(min(max(v, 1), 16) for v in r["shape"])
    cin, cout = (r["cin"] if r["cin"] > 0 else 32), (r["cout"] if r["cout"] > 0 else 32)
    if e["form"] == "tail":
        fine = (safe[0],) + tuple(2 * v for v in safe[1:]) + (cin,)
        g = dict((n, Guarded(sh, offset=r["off"][n])) for n, sh in (("x", fine), ("mbits", (1 << 16,)), ("y", fine), ("y2", safe + (cin,))))
        args = [g[n].ptr if r["ops"] & (1 << wc.SLOTS.index(n)) else None for n in ("x", "mbits", "y", "y2")]
        rc = getattr(h, e["fn"])(*(args + [LEAK] + list(r["shape"]) + [r["cin"], s]))
        torch.cuda.synchronize()
        outs = [g["y"], g["y2"]]
    else:
        xs, ys, cs, (wci, wco), _ = _geometry(r["entry"], safe, cin, cout, 0)
        p = dict(x=np.ones(xs, np.float32), w=np.ones((1, 1, 1), np.float32), bias=np.ones((ys[-1],), np.float32), res=np.ones(ys, np.float32),
                 xc=np.ones(cs or ys, np.float32), msrc=np.ones(ys, np.float32), acc0=None, core=np.empty(ys, np.bool_))
        c = Call(k, r, p, pack=False)
        rc = c.raw(dims=tuple(r["shape"]) + (r["cin"], r["cout"]))
        outs = [c.g[n] for n in ("y", "y2", "sbits", "wp") if n in c.g]
    msg = h.df_last_error().decode()
    assert rc == r["reaches"], (rid, rc, msg)
    assert msg.startswith(e["fn"]), msg
    assert all(o.untouched() for o in outs), rid + ": written to after an error"
