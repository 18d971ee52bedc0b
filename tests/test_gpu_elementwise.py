"""-m gpu: the small train-step kernels of csrc/elementwise.hip, each called directly at its edges -- one element, one below / at / above a
tile, the wrap of the 2048-workgroup grid-stride loops, the switch between two kernel families -- and compared with the NumPy restatements
of tests/elementwise_ref.py.  Three kinds of comparison:
  1. bit-exact against the fp32 twin (data movement, fixed-order sums of <= 8 terms, the gradient-descent step);
  2. bit-exact on integers in [-4, 4] (reductions whose order is the kernel's own business: every partial sum is exact, see the host gate);
  3. |kernel - fp64| <= 3 * e32 + one ulp of the largest reference magnitude, e32 = the twin's own largest error on the same inputs
     (linear / colsum on random data: L * 2^-24 * sum|terms|, L = the kernel's longest sequential fp32 chain).  Nothing is calibrated on
     the kernel; each case prints e32, the kernel's error, the bound and whether the kernel matched the twin bit for bit.
Every output is allocated pre-filled with NaN and one guard row (or element) longer than needed; the guard must stay NaN."""
import numpy as np
import pytest
import torch

import elementwise_ref as ref
from gpu_util import Out, assert_bits, host      # (the guarded output buffer and the bit comparison are shared with the stencil tests)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.array(a, dtype=F32)).cuda()       # (a copy: the shared inputs are read-only arrays)


@pytest.fixture(scope="module")
def k():
    """(call, query, _ptr, stream)"""
    from deep_fluids_amd._lib import call, query
    from deep_fluids_amd.ops import _ptr, _stream
    return call, query, _ptr, _stream()


def rule(name, got, r64, twin):
    r = ref.bounded(got, r64, twin)
    print(ref.fmt(name, r))
    return r


def chain_rule(name, got, r64, L, nterms, abs_terms):
    got = np.asarray(got)
    assert np.isfinite(got).all(), name
    err = np.abs(got.astype(F64) - r64)
    bound = ref.chain_bound(L, nterms, abs_terms)
    i = np.unravel_index(int(np.argmax(err - bound)), err.shape) if err.ndim else ()
    print("%-44s L %-5d kernel %.3e  bound %.3e  ratio %.3f" % (name, L, float(err[i]), float(bound[i]), float(err[i] / bound[i]) if bound[i] > 0 else 0.0))
    assert (err <= bound).all(), "%s: error %.3e above the chain bound %.3e at %s" % (name, float(err[i]), float(bound[i]), i)


# ---- optimisers -----------------------------------------------------------------------------------------------------------------------
def _adam_both(k, inputs, lr_t, gs):
    """host-scalar and device-scalar entry points on the same inputs -> [(p, m, v)] * 2"""
    call, _, _ptr, s = k
    h = ref.ADAM_HYPER
    p, g, m, v = inputs
    res = []
    for devscal in (False, True):
        P, M, V = Out(p.shape, p), Out(m.shape, m), Out(v.shape, v)
        G = dev(g)
        if devscal:
            sc = torch.full((5,), NAN, device="cuda")
            call("df_store_scalars", _ptr(sc), 2, lr_t, gs, 0.0, 0.0, s)
            call("df_adam_tf1_step_dev", P.ptr, _ptr(G), M.ptr, V.ptr, p.size, _ptr(sc), h["b1"], h["b2"], h["eps"], s)
        else:
            call("df_adam_tf1_step", P.ptr, _ptr(G), M.ptr, V.ptr, p.size, lr_t, h["b1"], h["b2"], h["eps"], gs, s)
        res.append((P.get(), M.get(), V.get()))
        assert torch.equal(G, dev(g))
    for a, b in zip(*res):
        assert_bits(b, a, "device-scalar Adam vs host-scalar Adam")
    return res[0]


@pytest.mark.parametrize("n", ref.ADAM_SIZES)
def test_adam_sizes_host_and_device_scalars(k, n):
    h = ref.ADAM_HYPER
    for first, t, gs in ((False, 7, 0.5), (True, 1, 1.0)):
        if first and n not in (257, ref.WRAP + 1):
            continue
        inputs = ref.adam_inputs(n, first)
        lr_t = ref.adam_lr_t(t)
        got = _adam_both(k, inputs, lr_t, gs)
        r64 = ref.adam(*inputs, lr_t, h["b1"], h["b2"], h["eps"], gs, F64)
        r32 = ref.adam(*inputs, lr_t, h["b1"], h["b2"], h["eps"], gs, F32)
        for key, a, b, c in zip("pmv", got, r64, r32):
            rule("adam n=%d t=%d gs=%g %s" % (n, t, gs, key), a, b, c)


@pytest.mark.parametrize("first", [False, True])
def test_adam_extreme_gradients_and_eps_only_denominator(k, first):
    """g = +-1e-20 (g * g is subnormal), +-1e18 (v ~ 1e33), g = v = 0 with m = 0.1 (a step of lr_t * b1 * m / eps): never NaN, the same
    infinity where fp64 overflows fp32; the rule holds on all cells and once more on the plain cells alone."""
    h = ref.ADAM_HYPER
    p, g, m, v, plain = ref.adam_extreme_inputs(first)
    for gs in (1.0, 0.5):
        lr_t = ref.adam_lr_t(1 if first else 7)
        got = _adam_both(k, (p, g, m, v), lr_t, gs)
        r64 = ref.adam(p, g, m, v, lr_t, h["b1"], h["b2"], h["eps"], gs, F64)
        r32 = ref.adam(p, g, m, v, lr_t, h["b1"], h["b2"], h["eps"], gs, F32)
        for key, a, b, c in zip("pmv", got, r64, r32):
            assert np.isfinite(a).all()
            rule("adam extremes first=%d gs=%g %s" % (first, gs, key), a, b, c)
            rule("adam extremes first=%d gs=%g %s (plain cells)" % (first, gs, key), a[plain], b[plain], c[plain])


@pytest.mark.parametrize("n", ref.ADAM_SIZES)
def test_gd_step_host_and_device_scalars_bit_exact(k, n):
    call, _, _ptr, s = k
    p, g, _, _ = ref.adam_inputs(n)
    for lr, gs in ((float(F32(1e-4)), 1.0), (float(F32(3e-3)), 0.5), (float(F32(0.3)), float(F32(1.0 / 3.0)))):
        want = ref.gd(p, g, lr, gs, F32)
        G = dev(g)
        P = Out(p.shape, p)
        call("df_gd_step", P.ptr, _ptr(G), n, lr, gs, s)
        assert_bits(P.get(), want, "gd_step n=%d" % n)
        sc = torch.full((5,), NAN, device="cuda")
        call("df_store_scalars", _ptr(sc), 2, lr, gs, 0.0, 0.0, s)
        P2 = Out(p.shape, p)
        call("df_gd_step_dev", P2.ptr, _ptr(G), n, _ptr(sc), s)
        assert_bits(P2.get(), want, "gd_step_dev n=%d" % n)


def test_store_scalars_writes_exactly_the_first_n(k):
    call, _, _ptr, s = k
    vals = (1.5, -2.25, 3e-7, 4e9)
    for n in (1, 2, 3, 4):
        buf = torch.full((5,), NAN, device="cuda")
        call("df_store_scalars", _ptr(buf), n, *vals, s)
        got = host(buf)
        assert_bits(got[:n], np.asarray(vals, F32)[:n], "store_scalars n=%d" % n)
        assert np.isnan(got[n:]).all(), (n, got)


# ---- fully connected ------------------------------------------------------------------------------------------------------------------
def _linear_raw(k, x, w, b, gy, want):
    """-> dict of the outputs of one forward and one backward call; ``want`` names the backward outputs requested"""
    call, query, _ptr, s = k
    B, K = x.shape
    N = w.shape[1]
    X, W, Gy = dev(x), dev(w), dev(gy)
    Bi = dev(b) if b is not None else None
    nb = query("df_linear_workspace_bytes", B, K, N)
    ws = torch.full((nb // 4 + 1,), NAN, device="cuda")
    Y = Out((B, N))
    call("df_linear_fwd", _ptr(X), _ptr(W), _ptr(Bi), Y.ptr, B, K, N, _ptr(ws), nb, s)
    assert bool(torch.isnan(ws[nb // 4:]).all())
    outs = {"gx": Out((B, K)), "gw": Out((K, N)), "gb": Out((N,))}
    call("df_linear_bwd", _ptr(X), _ptr(W), _ptr(Gy), *[outs[key].ptr if key in want else None for key in ("gx", "gw", "gb")], B, K, N, s)
    res = {"y": Y.get()}
    for key, o in outs.items():
        got = o.get()
        if key in want:
            res[key] = got
        else:
            assert np.isnan(got).all(), "%s was not requested but written" % key
    return res


LINEAR_WANTS = (("gx", "gw", "gb"), ("gw", "gb"), ("gw",), ("gb",), ("gx",))


@pytest.mark.parametrize("B,K,N", ref.LINEAR_TINYK + ref.LINEAR_SPLITK)
def test_linear_integer_data_bit_exact(k, B, K, N):
    """both kernel families, all four outputs, with and without gx / gw / gb, with and without a bias: exact on integer data"""
    x, w, b, gy = ref.linear_inputs(B, K, N, True)
    y64 = ref.linear(x, w, b, F64)
    r64 = dict(zip(("gx", "gw", "gb"), ref.linear_bwd(x, w, gy, F64)), y=y64)
    for want in LINEAR_WANTS:
        got = _linear_raw(k, x, w, b, gy, want)
        for key, a in got.items():
            assert_bits(a, r64[key].astype(F32), "linear %s (%d, %d, %d) %s of %s" % (ref.linear_family(B, K, N), B, K, N, key, want))
    got = _linear_raw(k, x, w, None, gy, ("gb",))
    assert_bits(got["y"], ref.linear(x, w, None, F64).astype(F32), "linear without bias")


@pytest.mark.parametrize("B,K,N", ref.LINEAR_TINYK + ref.LINEAR_SPLITK)
def test_linear_random_data_chain_bound(k, B, K, N):
    """random data: L * 2^-24 * sum|terms| per output; through the raw entry points and through the autograd wrapper (gx requested and not)"""
    from deep_fluids_amd.ops import _Linear
    x, w, b, gy = ref.linear_inputs(B, K, N, False)
    L = ref.linear_chain(B, K, N)
    terms = ref.linear_abs_terms(x, w, b, gy)
    nterms = {"y": K + 1, "gx": N, "gw": B, "gb": B}
    r64 = dict(zip(("gx", "gw", "gb"), ref.linear_bwd(x, w, gy, F64)), y=ref.linear(x, w, b, F64))
    tag = "linear %s (%d,%d,%d) " % (ref.linear_family(B, K, N), B, K, N)
    full = _linear_raw(k, x, w, b, gy, ("gx", "gw", "gb"))
    for key in ("y", "gx", "gw", "gb"):
        chain_rule(tag + key, full[key], r64[key], L[key], nterms[key], terms[key])
    part = _linear_raw(k, x, w, b, gy, ("gw", "gb"))
    for key, a in part.items():
        assert_bits(a, full[key], tag + key + " without gx")
    for need_gx in (True, False):
        xt, wt, bt = dev(x).requires_grad_(need_gx), dev(w).requires_grad_(True), dev(b).requires_grad_(True)
        y = _Linear.apply(xt, wt, bt)
        y.backward(dev(gy))
        assert_bits(host(y), full["y"], tag + "wrapper y")
        assert_bits(host(wt.grad), full["gw"], tag + "wrapper gw")
        assert_bits(host(bt.grad), full["gb"], tag + "wrapper gb")
        if need_gx:
            assert_bits(host(xt.grad), full["gx"], tag + "wrapper gx")
        else:
            assert xt.grad is None


# ---- column sums ----------------------------------------------------------------------------------------------------------------------
def _colsum(k, g):
    call, query, _ptr, s = k
    rows, C = g.shape
    nb = query("df_colsum_workspace_bytes", rows, C)
    ws = torch.full((nb // 4 + 1,), NAN, device="cuda")
    out = Out((C,))
    G = dev(g)
    call("df_colsum", _ptr(G), out.ptr, rows, C, _ptr(ws), nb, s)
    assert bool(torch.isnan(ws[nb // 4:]).all()) and not bool(torch.isnan(ws[:nb // 4]).any())
    return out.get()


@pytest.mark.parametrize("rows,C", ref.COLSUM_SHAPES)
def test_colsum_integer_data_bit_exact(k, rows, C):
    g = ref.colsum_input(rows, C, True)
    assert_bits(_colsum(k, g), ref.colsum(g, F64).astype(F32), "colsum %d x %d" % (rows, C))


def test_colsum_random_data_chain_bound(k):
    rows, C = ref.COLSUM_RANDOM
    g = ref.colsum_input(rows, C, False)
    got = _colsum(k, g)
    chain_rule("colsum %dx%d" % (rows, C), got, ref.colsum(g, F64), ref.COLSUM_CHAIN, rows, np.abs(g).astype(F64).sum(axis=0))
    print("colsum %dx%d bitwise equal to the twin: %s" % (rows, C, "yes" if np.array_equal(got, ref.colsum(g, F32)) else "no"))


# ---- Bernoulli KL ---------------------------------------------------------------------------------------------------------------------
def _kl_case(tag, z, n, rho):
    from deep_fluids_amd import ops
    zt = dev(z).requires_grad_(True)
    loss = ops.kl_bernoulli(zt, n, rho)
    (loss * ref.KL_GOUT).backward()
    got, gz = host(loss), host(zt.grad)
    rule("kl fwd " + tag, got, np.asarray(ref.kl_bernoulli(z, n, rho, F64)), np.asarray(ref.kl_bernoulli(z, n, rho, F32)))
    rule("kl bwd " + tag, gz, ref.kl_bernoulli_bwd(z, n, rho, ref.KL_GOUT, 1.0, F64), ref.kl_bernoulli_bwd(z, n, rho, ref.KL_GOUT, 1.0, F32))
    assert_bits(gz[:, n:], np.zeros((z.shape[0], z.shape[1] - n), F32), "kl bwd tail columns " + tag)
    if n == 0:
        assert_bits(got, np.zeros((), F32), "kl fwd n = 0")
    return zt


@pytest.mark.parametrize("rho", ref.KL_RHOS)
@pytest.mark.parametrize("B,ncol,n", ref.KL_CASES)
def test_kl_bernoulli_fwd_bwd(k, B, ncol, n, rho):
    call, _, _ptr, s = k
    z = ref.kl_input(B, ncol)
    zt = _kl_case("B=%d ncol=%d n=%d rho=%.2f" % (B, ncol, n, rho), z, n, rho)
    # the raw entry points once more into guarded NaN buffers, with a scale other than 1: every element of gz is written, nothing behind it
    out, gz = Out(()), Out((B, ncol))
    gout = dev(np.asarray([ref.KL_GOUT], F32))
    call("df_kl_bernoulli_fwd", _ptr(zt), B, ncol, n, rho, out.ptr, s)
    call("df_kl_bernoulli_bwd", _ptr(zt), _ptr(gout), -0.5, gz.ptr, B, ncol, n, rho, s)
    rule("kl fwd raw", out.get(), np.asarray(ref.kl_bernoulli(z, n, rho, F64)), np.asarray(ref.kl_bernoulli(z, n, rho, F32)))
    rule("kl bwd raw scale=-0.5", gz.get(), ref.kl_bernoulli_bwd(z, n, rho, ref.KL_GOUT, -0.5, F64), ref.kl_bernoulli_bwd(z, n, rho, ref.KL_GOUT, -0.5, F32))
    assert_bits(gz.get()[:, n:], np.zeros((B, ncol - n), F32), "kl bwd raw tail columns")


@pytest.mark.parametrize("rho", ref.KL_RHOS)
def test_kl_bernoulli_means_next_to_0_and_1(k, rho):
    _kl_case("means 1e-6 | 1-1e-6 rho=%.2f" % rho, ref.kl_extreme_input(), 16, rho)


# ---- sigmoid --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.SIGMOID_SIZES)
def test_sigmoid_fwd_bwd_with_saturation(k, n):
    from deep_fluids_amd import ops
    call, _, _ptr, s = k
    x, gy = ref.sigmoid_inputs(n)
    X, Gy = dev(x), dev(gy)
    Y = Out((n,))
    call("df_sigmoid_fwd", _ptr(X), Y.ptr, n, s)
    y = Y.get()
    assert not np.isnan(y).any() and y.min() >= 0 and y.max() <= 1
    rule("sigmoid fwd n=%d" % n, y, ref.sigmoid(x, F64), ref.sigmoid(x, F32))
    if n >= 257:
        sat = np.abs(x) >= 89
        assert sat.sum() >= 6 and set(np.unique(y[sat])) == {0.0, 1.0}
    # backward on the output the kernel saved
    Gx = Out((n,))
    Ysaved = dev(y)
    call("df_sigmoid_bwd", _ptr(Gy), _ptr(Ysaved), Gx.ptr, n, s)
    gx = Gx.get()
    assert np.isfinite(gx).all() and (gx[(y == 0) | (y == 1)] == 0).all()
    rule("sigmoid bwd n=%d" % n, gx, ref.sigmoid_bwd(gy, y, F64), ref.sigmoid_bwd(gy, y, F32))
    # the autograd wrapper runs the same two kernels
    xt = dev(x).requires_grad_(True)
    yt = ops.sigmoid(xt)
    yt.backward(Gy)
    assert_bits(host(yt), y, "ops.sigmoid"); assert_bits(host(xt.grad), gx, "ops.sigmoid backward")


# ---- L1 and mean squared error ----------------------------------------------------------------------------------------------------------
def _mean_fwd(k, name, a, b):
    call, query, _ptr, s = k
    nb = query("df_l1_mean_workspace_bytes", a.size)
    ws = torch.full((nb // 8 + 1,), NAN, dtype=torch.float64, device="cuda")
    out = Out(())
    A, B = dev(a), dev(b)
    call(name, _ptr(A), _ptr(B), a.size, out.ptr, _ptr(ws), nb, s)
    assert bool(torch.isnan(ws[nb // 8:]).all())
    return out.get()


def _mean_bwd(k, name, a, b, gout, scale):
    call, _, _ptr, s = k
    ga = Out(a.shape)
    G = dev(np.asarray([gout], F32)) if gout is not None else None
    A, B = dev(a), dev(b)
    call(name, _ptr(A), _ptr(B), _ptr(G), scale, ga.ptr, a.size, s)
    return ga.get()


@pytest.mark.parametrize("n", ref.MEAN_SIZES)
def test_l1_and_mse_means(k, n):
    from deep_fluids_amd import ops
    a, b = ref.mean_inputs(n, True)
    d = a.astype(F64) - b
    assert_bits(_mean_fwd(k, "df_l1_mean_fwd", a, b), np.asarray(F32(np.abs(d).sum() / n)), "l1_mean_fwd n=%d" % n)
    assert_bits(_mean_fwd(k, "df_mse_mean_fwd", a, b), np.asarray(F32((d * d).sum() / n)), "mse_mean_fwd n=%d" % n)
    for integer in (True, False):
        a, b = ref.mean_inputs(n, integer)
        for gout, scale in ((None, 1.0), (3.0, 1.0), (0.7, -1.0)):
            g = 1.0 if gout is None else gout
            got = _mean_bwd(k, "df_l1_mean_bwd", a, b, gout, scale)
            assert_bits(got, ref.l1_mean_bwd(a, b, g, scale, F32), "l1_mean_bwd n=%d gout=%s scale=%g" % (n, gout, scale))
            assert (got[a == b] == 0).all() and (a == b).any()
            if gout is None:
                assert_bits(got, np.sign(a - b) * F32(scale / n), "l1_mean_bwd == sign(a - b) * float32(scale / n)")
            got = _mean_bwd(k, "df_mse_mean_bwd", a, b, gout, scale)
            rule("mse bwd n=%d int=%d gout=%s scale=%g" % (n, integer, gout, scale), got, ref.mse_mean_bwd(a, b, g, scale, F64), ref.mse_mean_bwd(a, b, g, scale, F32))
    # the autograd wrappers with a non-unit upstream gradient, both operands
    a, b = ref.mean_inputs(n, False)
    for fn, bwd, name in ((ops.l1_mean, ref.l1_mean_bwd, "df_l1_mean_fwd"), (ops.mse_mean, ref.mse_mean_bwd, "df_mse_mean_fwd")):
        at, bt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        loss = fn(at, bt)
        (loss * 3.0).backward()
        assert_bits(host(loss), _mean_fwd(k, name, a, b), "wrapper forward")
        if bwd is ref.l1_mean_bwd:
            assert_bits(host(at.grad), bwd(a, b, 3.0, 1.0, F32), "ops.l1_mean grad a"); assert_bits(host(bt.grad), bwd(a, b, 3.0, -1.0, F32), "ops.l1_mean grad b")
        else:
            rule("ops.mse_mean grad a n=%d" % n, host(at.grad), bwd(a, b, 3.0, 1.0, F64), bwd(a, b, 3.0, 1.0, F32))
            rule("ops.mse_mean grad b n=%d" % n, host(bt.grad), bwd(a, b, 3.0, -1.0, F64), bwd(a, b, 3.0, -1.0, F32))


def test_mse_mean_fwd_random_data(k):
    """one rounding case of the forward as well: squares in fp32, the sum in double"""
    for n in (257, 4 * ref.WRAP + 3):
        a, b = ref.mean_inputs(n, False)
        rule("mse fwd n=%d" % n, _mean_fwd(k, "df_mse_mean_fwd", a, b), np.asarray(ref.mse_mean(a, b, F64)), np.asarray(ref.mse_mean(a, b, F32)))
        rule("l1 fwd n=%d" % n, _mean_fwd(k, "df_l1_mean_fwd", a, b), np.asarray(ref.l1_mean(a, b, F64)), np.asarray(ref.l1_mean(a, b, F32)))


# ---- lrelu / add ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leak", ref.EW_LEAKS)
def test_lrelu_and_add_tiles(k, leak):
    call, _, _ptr, s = k
    rng = np.random.RandomState(11)
    for n in ref.EW_SIZES:
        a, c = ref.uni(rng, n), ref.uni(rng, n)
        a[:min(n, 3):2] = 0.0                                      # x == 0 and y == 0 take the leak branch (y > 0 is false)
        A, C = dev(a), dev(c)
        y = Out((n,)); call("df_lrelu_fwd", _ptr(A), y.ptr, leak, n, s)
        assert_bits(y.get(), ref.lrelu(a, leak, F32), "lrelu_fwd n=%d" % n)
        gx = Out((n,)); call("df_lrelu_bwd", _ptr(C), _ptr(A), gx.ptr, leak, n, s)
        assert_bits(gx.get(), ref.lrelu_bwd(c, a, leak, F32), "lrelu_bwd n=%d" % n)
        if leak == ref.EW_LEAKS[0]:
            o = Out((n,)); call("df_add", _ptr(A), _ptr(C), o.ptr, n, s)
            assert_bits(o.get(), ref.add(a, c, F32), "add n=%d" % n)


# ---- up-sampling family -----------------------------------------------------------------------------------------------------------------
def _up_shapes(is3d, wrap):
    return (ref.UP_SHAPES_3D if is3d else ref.UP_SHAPES_2D) + ((wrap[is3d],) if wrap else ())


def _up_rng(shape, is3d):
    return np.random.RandomState(sum(shape) * 2 + int(is3d))


@pytest.mark.parametrize("is3d", [True, False])
def test_upsample2x_fwd_bwd_bit_exact(k, is3d):
    from deep_fluids_amd.ops import _Upsample2x
    call, _, _ptr, s = k
    for shape in _up_shapes(is3d, ref.UP_WRAP_SRC):
        rng = _up_rng(shape, is3d)
        fine = ref.fine_shape(shape, is3d)
        x, g = ref.uni(rng, shape), ref.uni(rng, fine)
        x.reshape(-1)[0] = -0.0; g.reshape(-1)[:2] = -0.0
        X, G = dev(x), dev(g)
        y = Out(fine); call("df_upsample2x_fwd", _ptr(X), y.ptr, *shape, int(is3d), s)
        assert_bits(y.get(), ref.upsample2x(x, is3d), "upsample2x_fwd %s" % (shape,))
        gx = Out(shape); call("df_upsample2x_bwd", _ptr(G), gx.ptr, *shape, int(is3d), s)
        want = ref.upsample2x_bwd(g, is3d, F32)
        assert_bits(gx.get(), want, "upsample2x_bwd %s" % (shape,))
        if np.prod(shape) < 1 << 16:                               # the autograd wrapper (4-D tensors in 2-D)
            sq = (lambda t: t) if is3d else (lambda t: t[:, 0])
            xt = dev(sq(x)).requires_grad_(True)
            up = _Upsample2x.apply(xt)
            up.backward(dev(sq(g)))
            assert_bits(host(up), sq(ref.upsample2x(x, is3d)), "wrapper forward"); assert_bits(host(xt.grad), sq(want), "wrapper backward")


@pytest.mark.parametrize("is3d", [True, False])
def test_add_up2x_and_dilate2_odd_bit_exact(k, is3d):
    call, _, _ptr, s = k
    for shape in _up_shapes(is3d, ref.UP_WRAP_DST):
        rng = _up_rng(shape, is3d)
        fine = ref.fine_shape(shape, is3d)
        a, bc = ref.uni(rng, fine), ref.uni(rng, shape)
        A, Bc = dev(a), dev(bc)
        y = Out(fine); call("df_add_up2x", _ptr(A), _ptr(Bc), y.ptr, *shape, int(is3d), s)
        assert_bits(y.get(), ref.add_up2x(a, bc, is3d, F32), "add_up2x %s" % (shape,))
        bc.reshape(-1)[0] = -0.0                                   # a value is copied with its sign; the inserted zeros are +0.0
        Bc = dev(bc)
        o = Out(fine); call("df_dilate2_odd", _ptr(Bc), o.ptr, *shape, int(is3d), s)
        assert_bits(o.get(), ref.dilate2_odd(bc, is3d), "dilate2_odd %s" % (shape,))


@pytest.mark.parametrize("is3d", [True, False])
def test_lrelu_bwd_pool2x_against_the_restatement(k, is3d):
    call, _, _ptr, s = k
    for shape in _up_shapes(is3d, None):
        rng = _up_rng(shape, is3d)
        fine = ref.fine_shape(shape, is3d)
        dy, y = ref.uni(rng, fine), ref.uni(rng, fine)
        y.reshape(-1)[:2] = 0.0
        Dy, Y = dev(dy), dev(y)
        for leak in ref.EW_LEAKS:
            gx, gp = Out(fine), Out(shape)
            call("df_lrelu_bwd_pool2x", _ptr(Dy), _ptr(Y), gx.ptr, gp.ptr, leak, *shape, int(is3d), s)
            wx, wp = ref.lrelu_bwd_pool2x(dy, y, leak, is3d, F32)
            assert_bits(gx.get(), wx, "lrelu_bwd_pool2x gx %s" % (shape,)); assert_bits(gp.get(), wp, "lrelu_bwd_pool2x gpool %s" % (shape,))


# ---- concat ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Ca,Cb", ref.CONCAT_CASES)
def test_concat2_fwd_bwd_bit_exact(k, rows, Ca, Cb):
    from deep_fluids_amd import ops
    call, _, _ptr, s = k
    rng = np.random.RandomState(rows % 1000 + Ca * 10 + Cb)
    a, b, gy = ref.uni(rng, (rows, Ca)), ref.uni(rng, (rows, Cb)), ref.uni(rng, (rows, Ca + Cb))
    A, B, Gy = dev(a), dev(b), dev(gy)
    y = Out((rows, Ca + Cb)); call("df_concat2_fwd", _ptr(A), _ptr(B), y.ptr, rows, Ca, Cb, s)
    assert_bits(y.get(), ref.concat2(a, b), "concat2_fwd")
    ga, gb = Out((rows, Ca)), Out((rows, Cb))
    call("df_concat2_bwd", _ptr(Gy), ga.ptr, gb.ptr, rows, Ca, Cb, s)
    wa, wb = ref.concat2_bwd(gy, Ca)
    assert_bits(ga.get(), wa, "concat2_bwd ga"); assert_bits(gb.get(), wb, "concat2_bwd gb")
    if rows < 1000:
        at, bt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        yt = ops.concat([at, bt])
        yt.backward(dev(gy))
        assert_bits(host(yt), ref.concat2(a, b), "ops.concat"); assert_bits(host(at.grad), wa, "ops.concat ga"); assert_bits(host(bt.grad), wb, "ops.concat gb")


def test_concat2_unaligned_operand_takes_the_scalar_path(k):
    """float4-eligible extents, but b (forward) / gb (backward) starts one float into its buffer: not 16-byte aligned, so the entry point
    must fall back to the scalar kernel and stay exact; nothing before or behind the offset view may be written."""
    call, _, _ptr, s = k
    rows, Ca, Cb = ref.CONCAT_UNALIGNED
    rng = np.random.RandomState(5)
    a, b, gy = ref.uni(rng, (rows, Ca)), ref.uni(rng, (rows, Cb)), ref.uni(rng, (rows, Ca + Cb))
    bbuf = torch.full((rows * Cb + 2,), NAN, device="cuda")
    bbuf[1:1 + rows * Cb] = dev(b).reshape(-1)
    assert _ptr(bbuf) % 16 == 0 and (_ptr(bbuf) + 4) % 16 == 4
    A, Gy = dev(a), dev(gy)
    y = Out((rows, Ca + Cb)); call("df_concat2_fwd", _ptr(A), _ptr(bbuf) + 4, y.ptr, rows, Ca, Cb, s)
    assert_bits(y.get(), ref.concat2(a, b), "concat2_fwd, b one float in")
    ga = Out((rows, Ca))
    gbuf = torch.full((rows * Cb + 2,), NAN, device="cuda")
    call("df_concat2_bwd", _ptr(Gy), ga.ptr, _ptr(gbuf) + 4, rows, Ca, Cb, s)
    wa, wb = ref.concat2_bwd(gy, Ca)
    got = host(gbuf)
    assert np.isnan(got[0]) and np.isnan(got[-1]), "written outside the offset view"
    assert_bits(ga.get(), wa, "concat2_bwd ga, gb one float in"); assert_bits(got[1:-1].reshape(rows, Cb), wb, "concat2_bwd gb one float in")
