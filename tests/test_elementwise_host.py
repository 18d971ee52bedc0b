"""Host gate of the element-wise kernel tests (no GPU): the fp64 restatements of tests/elementwise_ref.py equal the oracle where it has
the operation; the integer-data cases of the GPU tests are exact in fp32 whatever the summation order; the fp32 twins' own distance from
fp64 (printed: the GPU tests' bound is three times that figure plus one ulp) is that of fp32 arithmetic; and the argument checks of the
entry points of csrc/elementwise.hip return their documented codes before any launch."""
import ctypes

import numpy as np
import pytest

import df_oracle as orc
import elementwise_ref as ref
from deep_fluids_amd import _lib

F32, F64 = np.float32, np.float64


# ---- (a) the fp64 restatements against the oracle --------------------------------------------------------------------------------------
def test_fp64_restatements_equal_the_oracle():
    rng = np.random.RandomState(0)
    # adam_tf1 (the oracle forms lr_t itself; grad_scale multiplies the gradient)
    p, g, m, v = (a.astype(F64) for a in ref.adam_inputs(257))
    for t, lr, gs in ((1, 1e-4, 1.0), (7, 2e-5, 0.5)):
        lr_t = lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.5 ** t)
        got = ref.adam(p, g, m, v, lr_t, 0.5, 0.999, 1e-8, gs, F64)
        want = orc.adam_tf1(p, gs * g, m, v, t, lr)
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=1e-14, atol=0)
    # Bernoulli KL, forward and backward, n < ncol included
    for (B, ncol, n) in ref.KL_CASES:
        z = ref.kl_input(B, ncol).astype(F64)
        for rho in ref.KL_RHOS:
            np.testing.assert_allclose(ref.kl_bernoulli(z, n, rho, F64), orc.kl_bernoulli(z, n, rho), rtol=1e-13, atol=0)
            np.testing.assert_allclose(ref.kl_bernoulli_bwd(z, n, rho, 1.75, 1.0, F64), orc.kl_bernoulli_bwd(z, n, rho, 1.75), rtol=1e-13, atol=0)
    # nearest up-sampling and its adjoint, 3-D and 2-D (the oracle's 2-D tensors are [B, H, W, C])
    for shape in ref.UP_SHAPES_3D:
        x = rng.uniform(-1, 1, shape)
        np.testing.assert_array_equal(ref.upsample2x(x, True), orc.upscale_nn(x))
        gy = rng.uniform(-1, 1, ref.fine_shape(shape, True))
        np.testing.assert_allclose(ref.upsample2x_bwd(gy, True, F64), orc.upscale_nn_bwd(gy), rtol=1e-15, atol=1e-16)
    for shape in ref.UP_SHAPES_2D:
        x = rng.uniform(-1, 1, shape)
        np.testing.assert_array_equal(ref.upsample2x(x, False)[:, 0], orc.upscale_nn(x[:, 0]))
        gy = rng.uniform(-1, 1, ref.fine_shape(shape, False))
        np.testing.assert_allclose(ref.upsample2x_bwd(gy, False, F64)[:, 0], orc.upscale_nn_bwd(gy[:, 0]), rtol=1e-15, atol=1e-16)
    # linear, lrelu
    for (B, K, N) in ((5, 3, 1000), (3, 1024, 16)):
        x, w, b, _ = (a.astype(F64) for a in ref.linear_inputs(B, K, N, False))
        np.testing.assert_allclose(ref.linear(x, w, b, F64), orc.linear(x, w, b), rtol=1e-14, atol=1e-14)
    x = rng.uniform(-1, 1, 1003)
    for leak in ref.EW_LEAKS:
        np.testing.assert_array_equal(ref.lrelu(x, leak, F64), orc.lrelu(x, leak))


def test_restatements_of_the_data_movement_are_adjoint_pairs():
    """<up(x), g> == <x, up_bwd(g)>, the same for concat; dilate2_odd puts g at the odd positions and +0.0 elsewhere."""
    rng = np.random.RandomState(1)
    for is3d, shapes in ((True, ref.UP_SHAPES_3D), (False, ref.UP_SHAPES_2D)):
        for shape in shapes:
            x = rng.randint(-4, 5, shape).astype(F64)
            g = rng.randint(-4, 5, ref.fine_shape(shape, is3d)).astype(F64)
            assert (ref.upsample2x(x, is3d) * g).sum() == (x * ref.upsample2x_bwd(g, is3d, F64)).sum()
            d = ref.dilate2_odd(x.astype(F32), is3d)
            assert d.shape == ref.fine_shape(shape, is3d) and d.sum() == x.sum() and not np.signbit(d[d == 0]).any()
            assert np.count_nonzero(d) == np.count_nonzero(x)
            gx, gp = ref.lrelu_bwd_pool2x(g, -g, 0.2, is3d, F64)
            np.testing.assert_array_equal(gp, ref.upsample2x_bwd(g, is3d, F64))
            np.testing.assert_array_equal(gx, np.where(-g > 0, g, 0.2 * g))
    for (rows, Ca, Cb) in ref.CONCAT_CASES[:5]:
        a, b = ref.ints(rng, (rows, Ca)), ref.ints(rng, (rows, Cb))
        y = ref.concat2(a, b)
        ga, gb = ref.concat2_bwd(y, Ca)
        np.testing.assert_array_equal(ga, a); np.testing.assert_array_equal(gb, b)


# ---- (b) the integer-data cases are exact in fp32 in any order -------------------------------------------------------------------------
def test_integer_cases_keep_every_partial_sum_below_2_pow_24():
    """sum(|terms|) < 2^24 per output: every partial sum in every order is an integer of smaller magnitude, hence exact.  The fp32 twin
    must then equal the rounded fp64 result bit for bit -- which also shows the twins' index arithmetic (chunks, lanes, ragged blocks)."""
    for (B, K, N) in ref.LINEAR_TINYK + ref.LINEAR_SPLITK:
        x, w, b, gy = ref.linear_inputs(B, K, N, True)
        for a in (x, w, b, gy):
            assert np.abs(a).max() <= 4 and np.array_equal(a, np.round(a))
        terms = ref.linear_abs_terms(x, w, b, gy)
        for key, t in terms.items():
            assert np.max(t) < ref.EXACT, ((B, K, N), key, float(np.max(t)))
        np.testing.assert_array_equal(ref.linear(x, w, b, F32), ref.linear(x, w, b, F64).astype(F32))
        for got, want in zip(ref.linear_bwd(x, w, gy, F32), ref.linear_bwd(x, w, gy, F64)):
            np.testing.assert_array_equal(got, want.astype(F32))
    for (rows, C) in ref.COLSUM_SHAPES:
        g = ref.colsum_input(rows, C, True)
        assert np.abs(g).astype(F64).sum(axis=0).max() < ref.EXACT
        np.testing.assert_array_equal(ref.colsum(g, F32), ref.colsum(g, F64).astype(F32))
    for n in ref.MEAN_SIZES:
        a, b = ref.mean_inputs(n, True)
        assert np.abs(a).max() <= 4 and np.abs(b).max() <= 4
        d = a.astype(F64) - b
        assert np.abs(d).sum() < ref.EXACT and (d * d).sum() < ref.EXACT, n
        # the kernel multiplies by the double 1/n: after the rounding to fp32 that is float32(exact_sum / n) on every case
        assert ref.l1_mean(a, b, F32) == F32(np.abs(d).sum() / n), n
        assert ref.mse_mean(a, b, F32) == F32((d * d).sum() / n), n
        assert float(F32(n)) == n                                     # the backward divides by float(n)
        body = 4 * (n // 4)
        assert (body == 0 or (d[:body] == 0).any()) and (n % 4 == 0 or d[n - 1] == 0)      # ties in the body and in the tail


# ---- (c) the twins' distance from fp64 on the rounding cases ---------------------------------------------------------------------------
def _report(name, twin, r64, rel_cap):
    """print e32 and what the GPU rule would ask (3 * e32 + one ulp of the largest magnitude); e32 must be fp32-sized"""
    twin = np.asarray(twin); r64 = np.asarray(r64, F64)
    with np.errstate(over="ignore"):
        fin = ~np.isinf(r64.astype(F32))
    assert np.isfinite(twin[fin]).all(), name
    assert np.array_equal(twin[~fin], r64.astype(F32)[~fin]) if (~fin).any() else True
    e32 = float(np.abs(twin[fin].astype(F64) - r64[fin]).max()) if fin.any() else 0.0
    scale = float(np.abs(r64[fin]).max()) if fin.any() else 0.0
    floor = float(np.spacing(F32(scale)))
    print("%-44s e32 %.3e  bound %.3e  largest |ref| %.3e" % (name, e32, 3 * e32 + floor, scale))
    assert e32 <= rel_cap * max(scale, 1e-30), (name, e32, scale)
    return e32


def test_twin_errors_of_the_optimisers_sigmoid_kl_and_mse():
    h = ref.ADAM_HYPER
    for n in ref.ADAM_SIZES:
        for first, t, gs in ((False, 7, 0.5), (True, 1, 1.0)):
            if first and n not in (257, ref.WRAP + 1):
                continue
            p, g, m, v = ref.adam_inputs(n, first)
            lr_t = ref.adam_lr_t(t)
            r64 = ref.adam(p, g, m, v, lr_t, h["b1"], h["b2"], h["eps"], gs, F64)
            r32 = ref.adam(p, g, m, v, lr_t, h["b1"], h["b2"], h["eps"], gs, F32)
            for key, a, b in zip("pmv", r32, r64):
                _report("adam n=%d t=%d gs=%g %s" % (n, t, gs, key), a, b, 4 * ref.U)
    for first in (False, True):
        p, g, m, v, plain = ref.adam_extreme_inputs(first)
        lr_t = ref.adam_lr_t(1 if first else 7)
        r64 = ref.adam(p, g, m, v, lr_t, h["b1"], h["b2"], h["eps"], 1.0, F64)
        r32 = ref.adam(p, g, m, v, lr_t, h["b1"], h["b2"], h["eps"], 1.0, F32)
        for key, a, b in zip("pmv", r32, r64):
            _report("adam extremes first=%d %s" % (first, key), a, b, 4 * ref.U)
            _report("adam extremes first=%d %s (plain cells)" % (first, key), a[plain], b[plain], 4 * ref.U)
    for n in ref.SIGMOID_SIZES:
        x, gy = ref.sigmoid_inputs(n)
        y32, y64 = ref.sigmoid(x, F32), ref.sigmoid(x, F64)
        assert not np.isnan(y32).any() and y32.min() >= 0 and y32.max() <= 1
        _report("sigmoid fwd n=%d" % n, y32, y64, 4 * ref.U)
        g32 = ref.sigmoid_bwd(gy, y32, F32)
        assert np.isfinite(g32).all() and (g32[(y32 == 0) | (y32 == 1)] == 0).all()
        _report("sigmoid bwd n=%d" % n, g32, ref.sigmoid_bwd(gy, y32, F64), 4 * ref.U)
    for (B, ncol, n) in ref.KL_CASES:
        z = ref.kl_input(B, ncol)
        for rho in ref.KL_RHOS:
            _report("kl fwd B=%d ncol=%d n=%d rho=%.2f" % (B, ncol, n, rho), ref.kl_bernoulli(z, n, rho, F32), ref.kl_bernoulli(z, n, rho, F64), 4 * ref.U)
            g32 = ref.kl_bernoulli_bwd(z, n, rho, ref.KL_GOUT, 1.0, F32)
            assert (g32[:, n:] == 0).all() and not np.signbit(g32[:, n:]).any()
            _report("kl bwd B=%d ncol=%d n=%d rho=%.2f" % (B, ncol, n, rho), g32, ref.kl_bernoulli_bwd(z, n, rho, ref.KL_GOUT, 1.0, F64), 4 * ref.U)
    z = ref.kl_extreme_input()
    assert (z.astype(F64).mean(axis=0) == z[0]).all()
    for rho in ref.KL_RHOS:
        _report("kl fwd means 1e-6 | 1-1e-6 rho=%.2f" % rho, ref.kl_bernoulli(z, 16, rho, F32), ref.kl_bernoulli(z, 16, rho, F64), 4 * ref.U)
        _report("kl bwd means 1e-6 | 1-1e-6 rho=%.2f" % rho, ref.kl_bernoulli_bwd(z, 16, rho, ref.KL_GOUT, 1.0, F32),
                ref.kl_bernoulli_bwd(z, 16, rho, ref.KL_GOUT, 1.0, F64), 4 * ref.U)
    for n in ref.MEAN_SIZES:
        a, b = ref.mean_inputs(n, False)
        for gout in (1.0, 3.0):
            _report("mse bwd n=%d gout=%g" % (n, gout), ref.mse_mean_bwd(a, b, gout, 1.0, F32), ref.mse_mean_bwd(a, b, gout, 1.0, F64), 4 * ref.U)


def test_twin_errors_of_linear_and_colsum_stay_inside_the_chain_bound():
    """The random-data cases of linear and colsum are held to L * 2^-24 * sum|terms| (L: the kernel's longest sequential fp32 chain); the
    twins, which run those chains, must satisfy it themselves."""
    for (B, K, N) in ref.LINEAR_TINYK + ref.LINEAR_SPLITK:
        x, w, b, gy = ref.linear_inputs(B, K, N, False)
        L = ref.linear_chain(B, K, N)
        terms = ref.linear_abs_terms(x, w, b, gy)
        nterms = {"y": K + 1, "gx": N, "gw": B, "gb": B}
        r64 = dict(zip(("gx", "gw", "gb"), ref.linear_bwd(x, w, gy, F64))); r64["y"] = ref.linear(x, w, b, F64)
        r32 = dict(zip(("gx", "gw", "gb"), ref.linear_bwd(x, w, gy, F32))); r32["y"] = ref.linear(x, w, b, F32)
        for key in ("y", "gx", "gw", "gb"):
            err = np.abs(r32[key].astype(F64) - r64[key])
            bound = ref.chain_bound(L[key], nterms[key], terms[key])
            print("linear %-8s B=%d K=%d N=%d %-2s L=%-5d twin %.3e  bound %.3e" % (ref.linear_family(B, K, N), B, K, N, key, L[key], err.max(), bound[err.argmax() if err.ndim == 0 else np.unravel_index(err.argmax(), err.shape)]))
            assert (err <= bound).all(), ((B, K, N), key)
    rows, C = ref.COLSUM_RANDOM
    g = ref.colsum_input(rows, C, False)
    err = np.abs(ref.colsum(g, F32).astype(F64) - ref.colsum(g, F64))
    bound = ref.chain_bound(ref.COLSUM_CHAIN, rows, np.abs(g).astype(F64).sum(axis=0))
    print("colsum %dx%d L=%d twin %.3e  bound %.3e" % (rows, C, ref.COLSUM_CHAIN, err.max(), bound[err.argmax()]))
    assert (err <= bound).all()


def test_the_bounded_rule_itself():
    """ref.bounded: passes the twin, refuses NaN where the reference is finite, a wrong infinity, and an error above the bound."""
    r64 = np.array([1.0, 2.0, 1e40, -1e40])
    twin = np.array([1.0, 2.0000002, np.inf, -np.inf], F32)
    res = ref.bounded(twin, r64, twin)
    assert res["bitwise"] and res["err"] == res["e32"] and res["bound"] >= 3 * res["e32"]
    for bad in ([np.nan, 2.0, np.inf, -np.inf], [1.0, 2.0, -np.inf, -np.inf], [1.0, 2.0, 3e38, -np.inf], [1.0, 2.00001, np.inf, -np.inf]):
        with pytest.raises(AssertionError):
            ref.bounded(np.array(bad, F32), r64, twin)


# ---- (d) argument errors come back before any launch -----------------------------------------------------------------------------------
def test_elementwise_entry_points_reject_bad_arguments_before_the_device():
    """Every call below fails a DF_REQUIRE that precedes the launch in csrc/elementwise.hip: DF_EINVAL -1 (null pointer, non-positive
    extent, rho outside (0, 1)), DF_ESHAPE -2 (C % 4, D != 1 in 2-D, KL extents), DF_EALIGN -3, DF_EWORKSPACE -4."""
    h = _lib.lib()
    buf = ctypes.create_string_buffer(8192)
    a = (ctypes.addressof(buf) + 15) & ~15
    b, c, o = a + 1024, a + 2048, a + 4096
    big = 1 << 20
    # df_l1_mean_fwd / df_mse_mean_fwd (a, b, n, out, workspace, workspace_bytes, stream)
    for fn in (h.df_l1_mean_fwd, h.df_mse_mean_fwd):
        assert fn(None, b, 16, o, c, big, None) == -1
        assert fn(a, None, 16, o, c, big, None) == -1
        assert fn(a, b, 16, None, c, big, None) == -1
        assert fn(a, b, 16, o, None, big, None) == -1
        assert fn(a, b, 0, o, c, big, None) == -1
        assert fn(a, b, 16, o, c, h.df_l1_mean_workspace_bytes(16) - 1, None) == -4
        assert b"workspace too small" in h.df_last_error()
    assert h.df_l1_mean_fwd(a + 4, b, 16, o, c, big, None) == -3
    assert h.df_l1_mean_fwd(a, b + 8, 16, o, c, big, None) == -3
    # df_l1_mean_bwd / df_mse_mean_bwd (a, b, gout, scale, ga, n, stream)
    for fn in (h.df_l1_mean_bwd, h.df_mse_mean_bwd):
        assert fn(None, b, c, 1.0, o, 16, None) == -1
        assert fn(a, None, c, 1.0, o, 16, None) == -1
        assert fn(a, b, c, 1.0, None, 16, None) == -1
        assert fn(a, b, c, 1.0, o, 0, None) == -1
        assert fn(a, b, c, 1.0, o, -3, None) == -1
    assert h.df_l1_mean_bwd(a, b, c, 1.0, o + 4, 16, None) == -3
    assert b"alignment" in h.df_last_error()
    # df_lrelu_fwd (x, y, leak, n, stream); df_lrelu_bwd (gy, y, gx, leak, n, stream); df_add (a, b, y, n, stream)
    assert h.df_lrelu_fwd(None, o, 0.2, 16, None) == -1
    assert h.df_lrelu_fwd(a, None, 0.2, 16, None) == -1
    assert h.df_lrelu_fwd(a, o, 0.2, 0, None) == -1
    assert h.df_lrelu_fwd(a, o + 4, 0.2, 16, None) == -3
    assert h.df_lrelu_bwd(None, b, o, 0.2, 16, None) == -1
    assert h.df_lrelu_bwd(a, None, o, 0.2, 16, None) == -1
    assert h.df_lrelu_bwd(a, b, None, 0.2, 16, None) == -1
    assert h.df_lrelu_bwd(a, b, o, 0.2, 0, None) == -1
    assert h.df_lrelu_bwd(a, b + 4, o, 0.2, 16, None) == -3
    assert h.df_add(None, b, o, 16, None) == -1
    assert h.df_add(a, b, None, 16, None) == -1
    assert h.df_add(a, b, o, 0, None) == -1
    assert h.df_add(a + 12, b, o, 16, None) == -3
    # the up-sampling family: (.., B, D, H, W, C, is_3d, stream)
    two = {"df_upsample2x_fwd": h.df_upsample2x_fwd, "df_upsample2x_bwd": h.df_upsample2x_bwd, "df_dilate2_odd": h.df_dilate2_odd}
    for name, fn in two.items():
        assert fn(None, o, 1, 1, 2, 2, 4, 1, None) == -1, name
        assert fn(a, None, 1, 1, 2, 2, 4, 1, None) == -1, name
        for dims in ((0, 1, 2, 2, 4), (1, 0, 2, 2, 4), (1, 1, 0, 2, 4), (1, 1, 2, -1, 4), (1, 1, 2, 2, 0)):
            assert fn(a, o, *dims, 1, None) == -1, (name, dims)
        assert fn(a, o, 1, 1, 2, 2, 6, 1, None) == -2, name
        assert b"multiple of 4" in h.df_last_error()
        assert fn(a, o, 1, 2, 2, 2, 4, 0, None) == -2, name
        assert b"D must be 1" in h.df_last_error()
        assert fn(a + 4, o, 1, 1, 2, 2, 4, 1, None) == -3, name
        assert fn(a, o + 8, 1, 1, 2, 2, 4, 0, None) == -3, name
    # df_add_up2x (a, bc, y, B, D, H, W, C, is_3d, stream)
    assert h.df_add_up2x(None, b, o, 1, 1, 2, 2, 4, 1, None) == -1
    assert h.df_add_up2x(a, None, o, 1, 1, 2, 2, 4, 1, None) == -1
    assert h.df_add_up2x(a, b, None, 1, 1, 2, 2, 4, 1, None) == -1
    assert h.df_add_up2x(a, b, o, 1, 1, 0, 2, 4, 1, None) == -1
    assert h.df_add_up2x(a, b, o, 1, 1, 2, 2, 5, 1, None) == -2
    assert h.df_add_up2x(a, b, o, 1, 3, 2, 2, 4, 0, None) == -2
    assert h.df_add_up2x(a, b + 4, o, 1, 1, 2, 2, 4, 1, None) == -3
    # df_lrelu_bwd_pool2x (gy, y, gx, gpool, leak, B, D, H, W, C, is_3d, stream)
    assert h.df_lrelu_bwd_pool2x(None, b, c, o, 0.2, 1, 1, 2, 2, 4, 1, None) == -1
    assert h.df_lrelu_bwd_pool2x(a, b, c, None, 0.2, 1, 1, 2, 2, 4, 1, None) == -1
    assert h.df_lrelu_bwd_pool2x(a, b, c, o, 0.2, 1, 1, 2, 0, 4, 1, None) == -1
    assert h.df_lrelu_bwd_pool2x(a, b, c, o, 0.2, 1, 1, 2, 2, 2, 1, None) == -2
    assert h.df_lrelu_bwd_pool2x(a, b, c, o, 0.2, 1, 2, 2, 2, 4, 0, None) == -2
    assert h.df_lrelu_bwd_pool2x(a, b, c + 4, o, 0.2, 1, 1, 2, 2, 4, 1, None) == -3
    # df_linear_fwd (x, w, bias, y, B, K, N, workspace, workspace_bytes, stream)
    assert h.df_linear_fwd(None, b, None, o, 1, 3, 8, None, 0, None) == -1
    assert h.df_linear_fwd(a, None, None, o, 1, 3, 8, None, 0, None) == -1
    assert h.df_linear_fwd(a, b, None, None, 1, 3, 8, None, 0, None) == -1
    for dims in ((0, 3, 8), (1, 0, 8), (1, 3, 0), (65536, 3, 8)):
        assert h.df_linear_fwd(a, b, None, o, *dims, None, 0, None) == -1, dims
    for (B, K, N) in ((3, 1024, 16), (2, 2049, 17), (1, 4096, 32)):       # the split-K path needs its workspace
        need = h.df_linear_workspace_bytes(B, K, N)
        assert need == -(-K // 2048) * B * N * 4
        assert h.df_linear_fwd(a, b, None, o, B, K, N, None, need, None) == -4
        assert b"split-K" in h.df_last_error()
        assert h.df_linear_fwd(a, b, None, o, B, K, N, c, need - 1, None) == -4
    assert h.df_linear_workspace_bytes(2, 1023, 16) == 0 and h.df_linear_workspace_bytes(2, 2048, 33) == 0
    # df_linear_bwd (x, w, gy, gx, gw, gb, B, K, N, stream)
    assert h.df_linear_bwd(None, b, c, None, o, None, 1, 3, 8, None) == -1
    assert h.df_linear_bwd(a, None, c, None, o, None, 1, 3, 8, None) == -1
    assert h.df_linear_bwd(a, b, None, None, o, None, 1, 3, 8, None) == -1
    for dims in ((0, 3, 8), (1, 0, 8), (1, 3, 0), (65536, 3, 8), (1, (1 << 31) - 1, 8)):
        assert h.df_linear_bwd(a, b, c, None, o, None, *dims, None) == -1, dims
    # df_colsum (g, gb, rows, C, workspace, workspace_bytes, stream)
    assert h.df_colsum(None, o, 8, 4, c, big, None) == -1
    assert h.df_colsum(a, None, 8, 4, c, big, None) == -1
    assert h.df_colsum(a, o, 8, 4, None, big, None) == -1
    for dims in ((0, 4), (8, 0), (8, 1 << 20)):
        assert h.df_colsum(a, o, *dims, c, 1 << 40, None) == -1, dims
    assert h.df_colsum_workspace_bytes(513, 3) == 2 * 3 * 4
    assert h.df_colsum(a, o, 513, 3, c, 2 * 3 * 4 - 1, None) == -4
    # the optimisers
    assert h.df_adam_tf1_step(None, b, c, o, 8, 1e-4, 0.5, 0.999, 1e-8, 1.0, None) == -1
    assert h.df_adam_tf1_step(a, None, c, o, 8, 1e-4, 0.5, 0.999, 1e-8, 1.0, None) == -1
    assert h.df_adam_tf1_step(a, b, None, o, 8, 1e-4, 0.5, 0.999, 1e-8, 1.0, None) == -1
    assert h.df_adam_tf1_step(a, b, c, None, 8, 1e-4, 0.5, 0.999, 1e-8, 1.0, None) == -1
    assert h.df_adam_tf1_step(a, b, c, o, 0, 1e-4, 0.5, 0.999, 1e-8, 1.0, None) == -1
    assert b"positive" in h.df_last_error()
    assert h.df_adam_tf1_step_dev(None, b, c, o, 8, a, 0.5, 0.999, 1e-8, None) == -1
    assert h.df_adam_tf1_step_dev(a, b, c, o, 8, None, 0.5, 0.999, 1e-8, None) == -1
    assert h.df_adam_tf1_step_dev(a, b, c, o, 0, a, 0.5, 0.999, 1e-8, None) == -1
    assert h.df_gd_step(None, b, 8, 1e-4, 1.0, None) == -1
    assert h.df_gd_step(a, None, 8, 1e-4, 1.0, None) == -1
    assert h.df_gd_step(a, b, 0, 1e-4, 1.0, None) == -1
    assert h.df_gd_step_dev(None, b, 8, c, None) == -1
    assert h.df_gd_step_dev(a, None, 8, c, None) == -1
    assert h.df_gd_step_dev(a, b, 8, None, None) == -1
    assert h.df_gd_step_dev(a, b, 0, c, None) == -1
    assert h.df_store_scalars(None, 2, 1.0, 2.0, 3.0, 4.0, None) == -1
    for n in (0, 5, -1):
        assert h.df_store_scalars(a, n, 1.0, 2.0, 3.0, 4.0, None) == -1, n
        assert b"1..4" in h.df_last_error()
    # df_concat2_fwd (a, b, y, rows, Ca, Cb, stream) / df_concat2_bwd (gy, ga, gb, rows, Ca, Cb, stream)
    for fn in (h.df_concat2_fwd, h.df_concat2_bwd):
        assert fn(None, b, o, 2, 4, 4, None) == -1
        assert fn(a, None, o, 2, 4, 4, None) == -1
        assert fn(a, b, None, 2, 4, 4, None) == -1
        for dims in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (2, -4, 4)):
            assert fn(a, b, o, *dims, None) == -1, dims
    # df_kl_bernoulli_fwd (z, B, ncol, n, rho, out, stream) / _bwd (z, gout, scale, gz, B, ncol, n, rho, stream)
    assert h.df_kl_bernoulli_fwd(None, 2, 16, 16, 0.05, o, None) == -1
    assert h.df_kl_bernoulli_fwd(a, 2, 16, 16, 0.05, None, None) == -1
    for dims in ((0, 16, 16), (2, 0, 0), (2, 16, 17), (2, 16, -1), (1 << 24, 16, 16), (2, 1 << 24, 16)):
        assert h.df_kl_bernoulli_fwd(a, *dims, 0.05, o, None) == -2, dims
        assert h.df_kl_bernoulli_bwd(a, b, 1.0, o, *dims, 0.05, None) == -2, dims
    for rho in (0.0, 1.0, -0.5, 1.5):
        assert h.df_kl_bernoulli_fwd(a, 2, 16, 16, rho, o, None) == -1, rho
        assert b"rho" in h.df_last_error()
        assert h.df_kl_bernoulli_bwd(a, b, 1.0, o, 2, 16, 16, rho, None) == -1, rho
    assert h.df_kl_bernoulli_bwd(None, b, 1.0, o, 2, 16, 16, 0.05, None) == -1
    assert h.df_kl_bernoulli_bwd(a, None, 1.0, o, 2, 16, 16, 0.05, None) == -1
    assert h.df_kl_bernoulli_bwd(a, b, 1.0, None, 2, 16, 16, 0.05, None) == -1
    # df_sigmoid_fwd (x, y, n, stream) / df_sigmoid_bwd (gy, y, gx, n, stream)
    assert h.df_sigmoid_fwd(None, o, 8, None) == -1
    assert h.df_sigmoid_fwd(a, None, 8, None) == -1
    assert h.df_sigmoid_fwd(a, o, 0, None) == -1
    assert h.df_sigmoid_bwd(None, b, o, 8, None) == -1
    assert h.df_sigmoid_bwd(a, None, o, 8, None) == -1
    assert h.df_sigmoid_bwd(a, b, None, 8, None) == -1
    assert h.df_sigmoid_bwd(a, b, o, 0, None) == -1
