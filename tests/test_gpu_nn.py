"""arch='nn' on the MI355X: every kernel of libdeepfluids_hip_nn.so against the NumPy twin (tests/nn_ref.py), the train step, the
evaluation losses, the one-launch rollout, determinism, checkpoint resume, the argument refusals and the chain from a synthetic data set
to velocity fields.

The mask, the column sums (so mean / rstd / the moving averages), the whole backward block given its inputs, the window step and the
MSE must match the fp32 twin BIT FOR BIT.  Everything downstream of ELU is compared to fp64 within ``nn_ref.tolerance``: 4 x the twin's
own deviation from fp64, measured here (ELU is the header's own fp32 series, which the twin repeats; the twin's fused multiply-adds of
the linear layers are formed in fp64 and can differ from the device's on exact ties)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nn_ref as R
from gpu_util import Guarded, assert_bits, dev, host

pytestmark = pytest.mark.gpu

Z, P = 3, 2
O32, O64 = R.Ops32(), R.Ops64()


def _call(name, *args):
    from deep_fluids_amd import ops
    ops.call(name, *(tuple(float(a) if isinstance(a, np.floating) else a for a in args) + (ops._stream(),)))


def _close(got, ref64, twin32, what):
    tol = R.tolerance(ref64, twin32)
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    print("%s: |gpu - fp64| %.3e  tolerance %.3e" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


# ---- the block between the linear layers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5, 67])
@pytest.mark.parametrize("filters", [8, 40])
def test_bn_elu_dropout_forward_backward_inference(filters, B):
    rng = np.random.RandomState(100 * filters + B)
    for layer, N in enumerate((2 * filters, filters)):          # 16 / 8 and 80 / 40 columns: each leaves a partial block of 32
        keep, seed, step, window = (0.1, 0.5)[layer], 7, 3, 2
        x = _f32(rng.normal(0.3, 1.5, (B, N)))
        x[0, 0] = 0.0
        gamma, beta = _f32(rng.uniform(0.5, 1.5, N)), _f32(rng.uniform(-0.5, 0.5, N))
        mm, mv = _f32(rng.uniform(-0.2, 0.2, N)), _f32(rng.uniform(0.5, 1.5, N))
        kept = R.mask(R.mask_key(seed, step, window, layer), B, N, keep)
        t_out, t_act, t_mean, t_rstd, t_mm, t_mv = O32.bn_fwd(x, gamma, beta, mm, mv, kept, keep)
        r_out, r_act, _, _, r_mm, r_mv = O64.bn_fwd(*[a.astype(np.float64) for a in (x, gamma, beta, mm, mv)], kept, keep)
        gx_, g_gamma, g_beta, g_mm, g_mv = Guarded((B, N), x), Guarded((N,), gamma), Guarded((N,), beta), Guarded((N,), mm), Guarded((N,), mv)
        act, out, mean, rstd = Guarded((B, N)), Guarded((B, N)), Guarded((N,)), Guarded((N,))
        _call("df_nn_bn_elu_dropout_fwd", gx_.ptr, g_gamma.ptr, g_beta.ptr, g_mm.ptr, g_mv.ptr, act.ptr, out.ptr, mean.ptr, rstd.ptr, B, N,
              R.EPS, R.DECAY, keep, seed, step, window, layer)
        what = "fwd B%d N%d" % (B, N)
        assert_bits(mean.get(what), t_mean, what + " mean"); assert_bits(rstd.get(what), t_rstd, what + " rstd")
        assert_bits(g_mm.get(what), t_mm, what + " moving_mean"); assert_bits(g_mv.get(what), t_mv, what + " moving_variance")
        g_act, g_out = act.get(what), out.get(what)
        assert_bits(g_out[~kept], np.zeros(int((~kept).sum()), np.float32), what + " dropped")
        assert_bits(g_out[kept], g_act[kept] * (np.float32(1) / np.float32(keep)), what + " kept = act * inv")
        _close(g_act, r_act, t_act, what + " act")
        _close(g_out, r_out, t_out, what + " out")
        for g in (gx_, g_gamma, g_beta):
            g.check_guards(what)

        # backward, on the twin's own activations: bit for bit
        gout = _f32(rng.normal(0, 1, (B, N)))
        if B > 2:
            t_act[1, 0] = 0.0          # an exact zero takes g
        t_gx, t_gg, t_gb = O32.bn_bwd(x, t_act, gout, gamma, t_mean, t_rstd, kept, keep)
        a_in, go_in, m_in, r_in = Guarded((B, N), t_act), Guarded((B, N), gout), Guarded((N,), t_mean), Guarded((N,), t_rstd)
        gx, gg, gb = Guarded((B, N)), Guarded((N,)), Guarded((N,))
        _call("df_nn_bn_elu_dropout_bwd", gx_.ptr, a_in.ptr, go_in.ptr, g_gamma.ptr, m_in.ptr, r_in.ptr, gx.ptr, gg.ptr, gb.ptr, B, N, keep, seed,
              step, window, layer)
        what = "bwd B%d N%d" % (B, N)
        assert_bits(gb.get(what), t_gb, what + " gbeta"); assert_bits(gg.get(what), t_gg, what + " ggamma")
        assert_bits(gx.get(what), t_gx, what + " gx")

        # inference mode
        t_inf = O32.bn_infer(x, gamma, beta, mm, mv)
        r_inf = O64.bn_infer(*[a.astype(np.float64) for a in (x, gamma, beta, mm, mv)])
        inf, i_mm, i_mv = Guarded((B, N)), Guarded((N,), mm), Guarded((N,), mv)
        _call("df_nn_bn_elu_infer", gx_.ptr, g_gamma.ptr, g_beta.ptr, i_mm.ptr, i_mv.ptr, inf.ptr, B, N, R.EPS)
        _close(inf.get("infer"), r_inf, t_inf, "infer B%d N%d" % (B, N))


def test_two_identical_calls_give_identical_bits_and_columns_do_not_interact():
    from deep_fluids_amd import ops
    rng = np.random.RandomState(4)
    B, N = 67, 80
    x, gamma, beta = dev(rng.normal(0, 1, (B, N))), dev(rng.uniform(0.5, 1.5, N)), dev(rng.uniform(-0.5, 0.5, N))
    runs = []
    for _ in range(2):
        mm, mv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
        out = ops.nn_bn_elu_dropout(x, gamma, beta, mm, mv, train=True, keep_prob=0.5, seed=1, step=2, window=0, layer=1)
        runs.append([host(t) for t in (out, mm, mv)])
    for a, b in zip(*runs):
        assert_bits(a, b, "second call")
    # columns 37..43 on their own (one workgroup, other neighbours): the same statistics, the same activations before the mask
    full = [Guarded((B, N)) for _ in range(2)] + [Guarded((N,)) for _ in range(2)]
    mm, mv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    _call("df_nn_bn_elu_dropout_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mm.data_ptr(), mv.data_ptr(),
          *([g.ptr for g in full] + [B, N, R.EPS, R.DECAY, 0.5, 1, 2, 0, 1]))
    c0, c1 = 37, 44
    xs, gs, bs = x[:, c0:c1].contiguous(), gamma[c0:c1].contiguous(), beta[c0:c1].contiguous()
    part = [Guarded((B, c1 - c0)) for _ in range(2)] + [Guarded((c1 - c0,)) for _ in range(2)]
    _call("df_nn_bn_elu_dropout_fwd", xs.data_ptr(), gs.data_ptr(), bs.data_ptr(), mm.data_ptr(), mv.data_ptr(),
          *([g.ptr for g in part] + [B, c1 - c0, R.EPS, R.DECAY, 0.5, 1, 2, 0, 1]))
    assert_bits(part[0].get(), full[0].get()[:, c0:c1], "act of a column block"); assert_bits(part[2].get(), full[2].get()[c0:c1], "mean")
    assert_bits(part[3].get(), full[3].get()[c0:c1], "rstd")


# ---- window step, stack, MSE --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5, 67])
@pytest.mark.parametrize("W", [1, 3])
def test_window_advance_stack_and_mse_bit_for_bit(B, W):
    from deep_fluids_amd import ops
    rng = np.random.RandomState(10 * B + W)
    K0, ratio = Z + P, np.float32(0.37)
    xw, yw = _f32(rng.normal(0, 1, (B, W, K0))), _f32(rng.normal(0, 1, (B, W, Z)))
    x, y = _f32(rng.normal(0, 1, (B, K0))), _f32(rng.normal(0, 1, (B, Z)))
    if W > 1:
        g_x, g_y, g_xw = Guarded((B, K0), x), Guarded((B, Z), y), Guarded((B, W, K0), xw)
        for i in range(W - 1):
            xn = Guarded((B, K0))
            _call("df_nn_window_advance_fwd", g_x.ptr, g_y.ptr, g_xw.ptr, xn.ptr, B, W, Z, P, i, ratio)
            assert_bits(xn.get(), O32.advance(x, y, xw, i, ratio, Z), "advance %d" % i)
        g = _f32(rng.normal(0, 1, (B, K0)))
        g_in, gx, gy = Guarded((B, K0), g), Guarded((B, K0)), Guarded((B, Z))
        _call("df_nn_window_advance_bwd", g_in.ptr, gx.ptr, gy.ptr, B, Z, P, ratio)
        want = g.copy(); want[:, Z:] = 0
        assert_bits(gx.get(), want, "advance gx"); assert_bits(gy.get(), g[:, :Z] * ratio, "advance gy")
        # through autograd: only the code part of x and y carry a gradient
        xt, yt = dev(x).requires_grad_(True), dev(y).requires_grad_(True)
        ops.nn_window_advance(xt, yt, dev(xw), 0, float(ratio)).backward(dev(g))
        assert_bits(host(xt.grad), want, "autograd gx"); assert_bits(host(yt.grad), g[:, :Z] * ratio, "autograd gy")
    ys = [dev(yw[:, i]).requires_grad_(True) for i in range(W)]
    stacked = ops.nn_window_stack(ys)
    assert_bits(host(stacked), yw, "stack")
    target = _f32(rng.normal(0, 1, (B, W, Z)))
    loss = ops.nn_mse(stacked, dev(target))
    assert_bits(host(loss).reshape(1), np.array([O32.mse(yw, target)]), "mse")
    loss.backward()
    gref = O32.mse_bwd(yw, target)
    for i in range(W):
        assert_bits(host(ys[i].grad), gref[:, i], "mse gradient of window entry %d" % i)


def test_mse_past_one_workgroup_and_past_256_partials():
    from deep_fluids_amd import ops
    rng = np.random.RandomState(3)
    for n in (1025, 300001):          # 2 workgroups with a partial one; 293 partial sums, more than the 256 threads of the second launch
        a, b = _f32(rng.normal(0, 1, n)), _f32(rng.normal(0, 1, n))
        got = host(ops.nn_mse(dev(a), dev(b))).reshape(1)
        assert_bits(got, np.array([O32.mse(a, b)]), "mse n=%d" % n)
        assert abs(float(got[0]) - float(O64.mse(a.astype(np.float64), b.astype(np.float64)))) < 1e-6


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def _trainer(filters, B, W, keep, params=None, lr=1e-3, **over):
    from deep_fluids_amd import ops
    from deep_fluids_amd.trainer import NNTrainer, default_config
    ops.reset_variables()
    bm = SimpleNamespace(code_std=np.float32(1.7), out_std=np.float32(0.4), p_num=P, epochs_per_step=0.01)
    cfg = default_config(arch="nn", z_num=Z, filters=filters, w_size=W, batch_size=B, lr_max=lr, lr_min=lr / 10, max_epoch=1, random_seed=17, **over)
    tr = NNTrainer(cfg, bm, keep_prob=keep)
    if params is not None:
        tr.load_variables({"NN/" + k: v for k, v in params.items()})
    return tr, bm


def _batches(rng, n, B, W):
    return [(_f32(rng.normal(0, 1, (B, W, Z + P))), _f32(rng.normal(0, 1, (B, W, Z)))) for _ in range(n)]


@pytest.mark.parametrize("filters,B,W,keep", [(8, 67, 3, 0.5), (40, 5, 3, 0.1), (8, 2, 1, 0.5), (40, 1, 1, 0.5)])
def test_train_step_matches_the_twin_for_three_steps(filters, B, W, keep):
    """Loss of every step, every gradient of the first, parameters and moving statistics after the third.  B = 2 and B = 1 are the
    ill-conditioned ends (a column whose two rows nearly agree has rstd near 1 / sqrt(eps) = 316, and Adam turns a gradient of 1e-6 into a
    full-size update): the twin follows the device op for op there too -- the linear layers, ELU and the optimizer included -- so its
    deviation from fp64 is the deviation this arithmetic has."""
    rng = np.random.RandomState(filters + B + W)
    p0 = R.init_params(rng, Z + P, filters, Z)
    batches = _batches(rng, 3, B, W)
    tr, bm = _trainer(filters, B, W, keep, p0)
    assert sorted(tr.var_names) == sorted("NN/" + k for k in R.NAMES)
    lrs, losses, grads = [], [], []
    for xw, yw in batches:
        lrs.append(tr.g_lr)
        m = tr.train_step(dev(xw), dev(yw))
        losses.append(float(m.loss)); grads.append(tr.grads_numpy())
    got = tr.variables_numpy()
    ratio = float(np.float32(bm.out_std) / np.float32(bm.code_std))
    p64, o64 = R.train_steps(O64, p0, batches, ratio, keep, 17, lambda s: lrs[s])
    p32, o32 = R.train_steps(O32, p0, batches, ratio, keep, 17, lambda s: lrs[s])
    for s in range(3):
        _close(losses[s], np.float64(o64[s]["loss"]), o32[s]["loss"], "step %d loss" % s)
        if s == 0:          # (later steps start from parameters that already differ by the optimizer's rounding: see the parameters below)
            for k in R.TRAINABLE:
                _close(grads[s]["NN/" + k], o64[s]["grads"][k], o32[s]["grads"][k], "step 0 gradient " + k)
            for k in R.NAMES:
                if "moving" in k:
                    assert not grads[s]["NN/" + k].any()
    for k in R.NAMES:
        _close(got["NN/" + k], p64[k], p32[k], "after 3 steps " + k)
    assert tr.step == 3 and tr._adam_t == 3


@pytest.mark.parametrize("filters,B,W", [(8, 67, 3), (40, 5, 1)])
def test_evaluation_losses_match_the_twin(filters, B, W):
    from deep_fluids_amd import ops
    rng = np.random.RandomState(filters)
    p0 = R.init_params(rng, Z + P, filters, Z)
    (xw, yw), = _batches(rng, 1, B, W)
    tr, bm = _trainer(filters, B, W, 0.1, p0)
    before = tr.variables_numpy()
    ratio = float(np.float32(bm.out_std) / np.float32(bm.code_std))
    with torch.no_grad():
        yw_, loss = tr._window(dev(xw), dev(yw), False)
    r64 = R.window_step(O64, p0, xw, yw, ratio, 0.1, 17, 0, train=False)
    r32 = R.window_step(O32, R.cast_params(O32, p0), xw, yw, ratio, 0.1, 17, 0, train=False)
    _close(host(yw_), r64["yw_"], r32["yw_"], "l_test_w predictions")
    _close(float(loss), np.float64(r64["loss"]), r32["loss"], "l_test_w")
    y1 = tr.predict(dev(xw[:, 0]))
    e64, e32 = R.forward_eval(O64, p0, xw[:, 0]), R.forward_eval(O32, R.cast_params(O32, p0), xw[:, 0])
    _close(host(y1), e64, e32, "l_test predictions")
    _close(float(ops.nn_mse(y1, dev(yw[:, 0]))), np.float64(O64.mse(e64, yw[:, 0].astype(np.float64))), O32.mse(e32, yw[:, 0]), "l_test")
    after = tr.variables_numpy()
    for k in before:          # evaluation mode moves nothing
        assert_bits(after[k], before[k], k)


@pytest.mark.parametrize("filters", [8, 40])
def test_rollout_one_launch_matches_the_twin_and_the_host_loop(filters):
    rng = np.random.RandomState(20 + filters)
    S, F = 2, 6
    p0 = R.init_params(rng, Z + P, filters, Z, scale=0.5)
    x_test, y_test = _f32(rng.normal(0, 1, (S * (F - 1), Z + P))), _f32(rng.normal(0, 1, (S * (F - 1), Z)))
    tr, bm = _trainer(filters, 4, 3, 0.1, p0)
    bm.x_test, bm.y_test, bm.num_test_scenes, bm.num_frames = x_test, y_test, S, F
    cs, os_ = bm.code_std, bm.out_std
    r64 = R.rollout(O64, p0, x_test, y_test, S, F, Z, cs, os_)
    r32 = R.rollout(O32, R.cast_params(O32, p0), x_test, y_test, S, F, Z, cs, os_)
    tol = R.tolerance(r64, r32)
    assert tol < 1e-4 * np.abs(r64).max(), "the twin's fp32 and fp64 rollouts drifted apart: the weights are too large for this check"
    z1, z2 = host(tr.rollout(bm)), host(tr.rollout(bm))
    assert_bits(z1, z2, "second rollout")
    _close(z1, r64, r32, "rollout kernel")
    # the same rollout as a host loop over the inference ops, one step per frame (what the reference does with sess.run)
    loop = np.zeros((S, F, Z), np.float32)
    for s in range(S):
        xin = x_test[s * (F - 1)].copy()
        loop[s, 0] = xin[:Z] * cs
        for t in range(F - 1):
            r = s * (F - 1) + t
            pred = host(tr.predict(dev(xin[None])))[0] * os_ + xin[:Z] * cs
            pred[Z - P:] = (y_test[r] * os_ + x_test[r, :Z] * cs)[Z - P:]
            loop[s, t + 1] = pred
            xin = np.concatenate([pred / cs, x_test[r + 1, Z:] if t < F - 2 else xin[Z:]])
    _close(loop, r64, r32, "host loop")
    assert np.abs(z1 - loop).max() <= tol
    np.testing.assert_array_equal(z1[:, :, Z - P:], R.z_gt(x_test, y_test, S, F, Z, cs, os_)[:, :, Z - P:])


def test_checkpoint_resume_is_bit_identical(tmp_path):
    rng = np.random.RandomState(8)
    batches = _batches(rng, 4, 5, 3)
    tr, _ = _trainer(8, 5, 3, 0.5)
    start = tr.variables_numpy()
    for xw, yw in batches:
        tr.train_step(dev(xw), dev(yw))
    want = [host(t).copy() for t in (tr.flat_p, tr.flat_m, tr.flat_v)] + [tr.step, tr.g_lr, tr._adam_t]
    tr, _ = _trainer(8, 5, 3, 0.5)
    tr.load_variables(start)
    for xw, yw in batches[:2]:
        tr.train_step(dev(xw), dev(yw))
    ckpt = str(tmp_path / "model.ckpt-2.npz")
    tr.save(ckpt)
    with np.load(ckpt) as d:
        assert "NN/BatchNorm/moving_mean" in d.files and "NN/BatchNorm_1/moving_variance" in d.files
        assert np.abs(d["NN/BatchNorm/moving_mean"]).max() > 0
    tr, _ = _trainer(8, 5, 3, 0.5)
    tr.load(ckpt)
    for xw, yw in batches[2:]:
        tr.train_step(dev(xw), dev(yw))
    for a, b, what in zip([host(t) for t in (tr.flat_p, tr.flat_m, tr.flat_v)], want[:3], ("parameters and moving statistics", "Adam m", "Adam v")):
        assert_bits(a, b, what)
    assert [tr.step, tr.g_lr, tr._adam_t] == want[3:]


def test_what_is_left_out_says_so():
    from deep_fluids_amd import ops
    from deep_fluids_amd.trainer import NNTrainer, default_config
    tr, bm = _trainer(8, 4, 3, 0.1)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        tr.enable_data_parallel()
    ops.reset_variables()
    with pytest.raises(NotImplementedError, match="graph=True"):
        NNTrainer(default_config(z_num=Z, filters=8, graph=True), bm)
    with pytest.raises(Exception, match="other than Adam"):
        NNTrainer(default_config(z_num=Z, filters=8, optimizer="gd"), bm)
    ops.reset_variables()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    from deep_fluids_amd import _lib
    E = _lib.DeepFluidsHipError
    B, N = 4, 8
    t = [torch.zeros(B * N + 8, device="cuda") for _ in range(9)]
    p = [a.data_ptr() for a in t]
    fwd = lambda *a: _call("df_nn_bn_elu_dropout_fwd", *a)
    good = p + [B, N, R.EPS, R.DECAY, 0.1, 1, 2, 3, 0]
    fwd(*good)
    fwd(*(p + [1, N, R.EPS, R.DECAY, 0.1, 1, 2, 3, 0]))                      # B = 1 is legal
    for i in range(9):
        with pytest.raises(E, match=r"\(%d\).*null" % _lib.DF_EINVAL):
            fwd(*(good[:i] + [None] + good[i + 1:]))
        with pytest.raises(E, match=r"\(%d\).*aligned" % _lib.DF_EALIGN):
            fwd(*(good[:i] + [p[i] + 2] + good[i + 1:]))
    for bad, code in (((0, N), _lib.DF_EINVAL), ((B, -1), _lib.DF_EINVAL), ((1 << 20, 1 << 12), _lib.DF_ESHAPE)):
        with pytest.raises(E, match=r"\(%d\)" % code):
            fwd(*(p + list(bad) + good[11:]))
    for keep in (0.0, 1.5, float("nan")):
        with pytest.raises(E, match="keep_prob"):
            fwd(*(p + [B, N, R.EPS, R.DECAY, keep, 1, 2, 3, 0]))
    with pytest.raises(E, match="eps"):
        fwd(*(p + [B, N, 0.0, R.DECAY, 0.1, 1, 2, 3, 0]))
    with pytest.raises(E, match="decay"):
        fwd(*(p + [B, N, R.EPS, 1.5, 0.1, 1, 2, 3, 0]))
    bwd = p + [B, N, 0.1, 1, 2, 3, 0]
    _call("df_nn_bn_elu_dropout_bwd", *bwd)
    with pytest.raises(E, match="null"):
        _call("df_nn_bn_elu_dropout_bwd", *([None] + bwd[1:]))
    with pytest.raises(E, match="keep_prob"):
        _call("df_nn_bn_elu_dropout_bwd", *(p + [B, N, 0.0, 1, 2, 3, 0]))
    with pytest.raises(E, match=r"\(%d\)" % _lib.DF_EINVAL):
        _call("df_nn_bn_elu_infer", *(p[:6] + [B, 0, R.EPS]))
    with pytest.raises(E, match="aligned"):
        _call("df_nn_bn_elu_infer", *([p[0] + 1] + p[1:6] + [B, N, R.EPS]))
    adv = lambda W, z, pn, i: _call("df_nn_window_advance_fwd", p[0], p[1], p[2], p[3], 2, W, z, pn, i, 0.5)
    adv(2, 2, 1, 0)
    for args, code in (((2, 2, 1, 1), _lib.DF_EINVAL), ((2, 2, 1, -1), _lib.DF_EINVAL), ((1, 2, 1, 0), _lib.DF_EINVAL), ((2, 1, 2, 0), _lib.DF_ESHAPE),
                       ((2, 0, 1, 0), _lib.DF_EINVAL)):
        with pytest.raises(E, match=r"\(%d\)" % code):
            adv(*args)
    with pytest.raises(E, match="null"):
        _call("df_nn_window_advance_bwd", None, p[1], p[2], 2, 2, 1, 0.5)
    _call("df_nn_window_advance_bwd", p[0], None, None, 2, 2, 1, 0.5)         # both outputs optional
    with pytest.raises(E, match="stride"):
        _call("df_nn_rows_copy", p[0], 2, p[1], 3, 2, 3)
    assert _lib.query("df_nn_mse_workspace_bytes", 0) == -1 and _lib.query("df_nn_mse_workspace_bytes", 1025) == 16
    ws = torch.zeros(4, dtype=torch.float64, device="cuda")
    _call("df_nn_mse_fwd", p[0], p[1], B * N, p[2], ws.data_ptr(), 32)
    with pytest.raises(E, match=r"\(%d\)" % _lib.DF_EWORKSPACE):
        _call("df_nn_mse_fwd", p[0], p[1], B * N, p[2], ws.data_ptr(), 0)
    with pytest.raises(E, match="8-byte"):
        _call("df_nn_mse_fwd", p[0], p[1], B * N, p[2], ws.data_ptr() + 4, 32)
    with pytest.raises(E, match=r"\(%d\)" % _lib.DF_EINVAL):
        _call("df_nn_mse_bwd", p[0], p[1], p[2], p[3], 0)
    buf = torch.zeros(64, device="cuda")
    big = [buf.data_ptr()] * 17
    roll = lambda S, F, z, pn, n1, n2, cs=1.0: _call("df_nn_rollout", *(big + [S, F, z, pn, n1, n2, R.EPS, cs, 1.0]))
    for args, code in (((1, 1, 2, 1, 4, 4), _lib.DF_ESHAPE), ((1, 3, 1, 2, 4, 4), _lib.DF_ESHAPE), ((0, 3, 2, 1, 4, 4), _lib.DF_EINVAL),
                       ((1, 3, 2, 1, 8192, 4), _lib.DF_ESHAPE), ((1, 3, 2, 1, 4, 4, 0.0), _lib.DF_EINVAL)):
        with pytest.raises(E, match=r"\(%d\)" % code):
            roll(*args)
    with pytest.raises(E, match="null"):
        _call("df_nn_rollout", *([None] + big[1:] + [1, 3, 2, 1, 4, 4, R.EPS, 1.0, 1.0]))
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_from_a_synthetic_data_set_to_velocity_fields(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, NNBatchManager, write_synthetic_ae_dataset
    from deep_fluids_amd.trainer import AETrainer, NNTrainer, default_config
    ops.reset_variables()
    root, spatial, scenes, frames, z_num, filters = str(tmp_path / "data"), (8, 16, 8), 3, 6, 4, 8
    n = write_synthetic_ae_dataset(root, spatial, num_scenes=scenes, num_frames=frames, seed=3)
    dcfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=True, arch="ae", data_type="velocity", batch_size=2, res_x=8, res_y=16, res_z=8,
                           num_worker=1)
    bm = BatchManager(dcfg, device="cuda")
    ae_dir, nn_dir = str(tmp_path / "ae"), str(tmp_path / "nn")
    ae = AETrainer(default_config(is_3d=True, res_x=8, res_y=16, res_z=8, filters=filters, batch_size=2, num_samples=n, z_num=z_num, p_num=2,
                                  model_dir=ae_dir, test_batch_size=6))
    code = ae.test_ae(bm)
    assert code == os.path.join(ae_dir, "code%d.npz" % z_num)
    cfg = default_config(arch="nn", is_3d=True, z_num=z_num, filters=filters, w_size=3, batch_size=4, max_epoch=2, model_dir=nn_dir, log_step=2,
                         data_path=root, code_path=ae_dir, test_batch_size=4)
    nbm = NNBatchManager(cfg)
    assert nbm.num_test_scenes == 1 and nbm.p_num == 2 and nbm.x_train_w.shape == (6, 3, z_num + 2)
    x, y = nbm.batch(is_window=True)
    assert x.is_cuda and x.shape[0] in (4, 2) and tuple(x.shape[1:]) == (3, z_num + 2) and tuple(y.shape) == (x.shape[0], 3, z_num)
    tr = NNTrainer(cfg, nbm)
    assert tr.max_step == 4                                  # 2 epochs of 2 windowed batches (4 + the remainder of 2)
    records = tr.train(nbm)
    assert [r["step"] for r in records] == [0, 2, 3] and all(np.isfinite([r["loss/total_loss"], r["loss/loss_test"], r["loss/loss_test_w"]]).all() for r in records)
    assert os.path.exists(os.path.join(nn_dir, "model.ckpt-4.npz"))
    out = tr.test_nn(nbm)
    assert out == os.path.join(nn_dir, "code_out.npz")
    with np.load(out) as d:
        assert d["z_out"].shape == d["z_gt"].shape == (1, frames, z_num) and np.isfinite(d["z_out"]).all()
        np.testing.assert_array_equal(d["z_out"][:, :, -2:], d["z_gt"][:, :, -2:])
    paths = ae.test_ae(bm, code_path=nn_dir)
    assert paths == [os.path.join(ae_dir, "v0.npz")]
    with np.load(paths[0]) as d:
        assert d["v"].shape == d["v_gt"].shape == (frames, 8, 16, 8, 3) and np.isfinite(d["v"]).all()
    ops.reset_variables()
