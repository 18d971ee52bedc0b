"""arch='nn' without a GPU: the fp64 restatement's own gradient, the hash mask, NNBatchManager against data_nn.py's arithmetic, and the
code_out.npz hand-over to AETrainer.test_ae(code_path=)."""
import os
from types import SimpleNamespace

import numpy as np

import nn_ref as R
from deep_fluids_amd.data import NNBatchManager

Z, P = 3, 2


def _windows(rng, B, W):
    return rng.uniform(-1, 1, (B, W, Z + P)), rng.uniform(-1, 1, (B, W, Z))


def test_fp64_gradient_of_the_windowed_loss_matches_central_differences():
    """every trainable entry: through the three applications, their batch statistics, their masks and the window step"""
    rng = np.random.RandomState(0)
    ops, W, ratio, keep, seed, step = R.Ops64(), 3, 0.7, 0.5, 11, 4
    p = R.init_params(rng, Z + P, 4, Z)
    xw, yw = _windows(rng, 5, W)
    g = R.window_step(ops, p, xw, yw, ratio, keep, seed, step)["grads"]
    h = 1e-6
    for k in R.TRAINABLE:
        num = np.zeros_like(p[k])
        for idx in np.ndindex(p[k].shape):
            lo, hi = dict(p), dict(p)
            lo[k] = p[k].copy(); hi[k] = p[k].copy()
            lo[k][idx] -= h; hi[k][idx] += h
            num[idx] = (R.window_step(ops, hi, xw, yw, ratio, keep, seed, step, want_grad=False)["loss"]
                        - R.window_step(ops, lo, xw, yw, ratio, keep, seed, step, want_grad=False)["loss"]) / (2 * h)
        # central differences of a smooth fp64 function: truncation h^2 and cancellation 1e-16 / h, both far below 1e-7 of the largest entry
        assert np.abs(num - g[k]).max() <= 1e-7 * max(np.abs(num).max(), 1.0) + 1e-9, k


def test_fp32_twin_follows_fp64():
    rng = np.random.RandomState(1)
    p = R.init_params(rng, Z + P, 8, Z)
    xw, yw = _windows(rng, 67, 3)
    a = R.window_step(R.Ops64(), p, xw, yw, 0.7, 0.5, 3, 0)
    b = R.window_step(R.Ops32(), R.cast_params(R.Ops32(), p), xw, yw, 0.7, 0.5, 3, 0)
    assert abs(float(b["loss"]) - a["loss"]) < 1e-5 * a["loss"]
    for k in R.TRAINABLE:
        assert np.abs(b["grads"][k] - a["grads"][k]).max() < 1e-4 * max(np.abs(a["grads"][k]).max(), 1e-3), k
    e = R.window_step(R.Ops64(), p, xw, yw, 0.7, 0.5, 3, 0, train=False)
    assert e["loss"] != a["loss"] and all(np.array_equal(e["moving"][k], p[k]) for k in e["moving"])


def test_mask_keep_rate_and_independence_of_the_batch():
    key = R.mask_key(123, 7, 2, 1)
    for keep in (0.1, 0.5):
        m = R.mask(key, 512, 512, keep)
        sigma = np.sqrt(keep * (1 - keep) / m.size)
        assert abs(m.mean() - keep) < 5 * sigma
    assert R.mask(key, 64, 64, 1.0).all()
    big = R.mask(key, 67, 80, 0.1)
    np.testing.assert_array_equal(R.mask(key, 5, 16, 0.1), big[:5, :16])                    # a shorter batch, fewer columns: same elements
    np.testing.assert_array_equal(R.mask(key, 7, 9, 0.1, row0=60, col0=71), big[60:, 71:])
    others = [R.mask_key(124, 7, 2, 1), R.mask_key(123, 8, 2, 1), R.mask_key(123, 7, 1, 1), R.mask_key(123, 7, 2, 0)]
    for k in others:                                                                        # seed, step, window, layer each move it
        assert (R.mask(k, 67, 80, 0.5) != R.mask(key, 67, 80, 0.5)).mean() > 0.4


def _write_code(tmp_path, scenes=3, frames=7, seed=5):
    rng = np.random.RandomState(seed)
    root = str(tmp_path / "data"); code_dir = str(tmp_path / "ae")
    os.makedirs(root); os.makedirs(code_dir)
    with open(os.path.join(root, "args.txt"), "w") as f:
        f.write("num_param: 2\nnum_frames: %d\nnum_dof: %d\n" % (frames, P))
    c = rng.normal(0, 2.0, (scenes, frames, Z)).astype(np.float32)
    code = dict(x=c[:, :-1].reshape(-1, Z), y=c[:, 1:].reshape(-1, Z), p=rng.uniform(-0.1, 0.1, (scenes * (frames - 1), P)).astype(np.float32),
                s=scenes, f=frames)
    np.savez_compressed(os.path.join(code_dir, "code%d.npz" % Z), **code)
    cfg = SimpleNamespace(data_path=root, code_path=code_dir, is_3d=True, w_size=3, z_num=Z, batch_size=4, random_seed=123)
    return cfg, code


def test_batch_manager_matches_data_nn_arithmetic(tmp_path):
    cfg, code = _write_code(tmp_path)
    bm = NNBatchManager(cfg, device="cpu")
    want = R.nn_arrays(code, cfg.w_size)
    for k in ("code_std", "out_std", "p_std", "x_train", "y_train", "x_test", "y_test", "x_train_w", "y_train_w", "x_test_w", "y_test_w"):
        np.testing.assert_array_equal(np.asarray(getattr(bm, k)), want[k], err_msg=k)
    assert bm.num_test_scenes == 1 and bm.num_frames == 7 and bm.p_num == P
    assert bm.x_train.shape == (12, Z + P) and bm.x_test.shape == (6, Z + P) and bm.x_train_w.shape == (8, 3, Z + P) and bm.x_test_w.shape == (4, 3, Z + P)
    # data_nn.py:121-126
    assert (bm.train_steps, bm.test_steps, bm.train_w_steps, bm.test_w_steps) == (3, 2, 2, 1) and bm.epochs_per_step == 0.5
    # consecutive slices, the remainder kept; an epoch visits every batch once, in a seeded order that seek() reproduces
    seen = [bm.batch(is_window=True) for _ in range(4)]
    assert sorted(int(x.shape[0]) for x, _ in seen[:2]) == [4, 4] and all(x.dtype.is_floating_point and y.shape[1:] == (3, Z) for x, y in seen)
    order = [bm.batch_index(i, True) for i in range(4)]
    assert sorted(order[:2]) == [0, 1] and sorted(order[2:]) == [0, 1]
    for (x, y), b in zip(seen, order):
        np.testing.assert_array_equal(x.numpy(), want["x_train_w"][4 * b:4 * b + 4]); np.testing.assert_array_equal(y.numpy(), want["y_train_w"][4 * b:4 * b + 4])
    bm.seek(1, is_window=True)
    np.testing.assert_array_equal(bm.batch(is_window=True)[0].numpy(), seen[1][0].numpy())
    sizes = [int(bm.batch()[0].shape[0]) for _ in range(3)]
    assert sorted(sizes) == [4, 4, 4]
    bm.init_test_it()
    a, b2, c = bm.test_batch(), bm.test_batch(), bm.test_batch()
    assert a[0].shape[0] == 4 and b2[0].shape[0] == 2 and np.array_equal(c[0].numpy(), a[0].numpy())      # the short remainder, then over again


def test_code_out_round_trip_has_the_shapes_test_ae_reads(tmp_path):
    cfg, code = _write_code(tmp_path, scenes=3, frames=7)
    bm = NNBatchManager(cfg, device="cpu")
    S, F = bm.num_test_scenes, bm.num_frames
    ops = R.Ops32()
    p = R.cast_params(ops, R.init_params(np.random.RandomState(2), Z + P, 8, Z, scale=0.3))
    z_out = R.rollout(ops, p, bm.x_test, bm.y_test, S, F, Z, bm.code_std, bm.out_std)
    z_gt = R.z_gt(bm.x_test, bm.y_test, S, F, Z, bm.code_std, bm.out_std)
    path = str(tmp_path / "code_out.npz")
    np.savez_compressed(path, z_out=z_out, z_gt=z_gt)
    with np.load(path) as d:                                  # what AETrainer.test_ae(code_path=) does with it (trainer.py:524-533)
        z_, z_gt_ = d["z_out"], d["z_gt"]
    num_sims, num_frames = z_.shape[0], z_[0].shape[0]
    assert (num_sims, num_frames) == (1, 7) and z_.shape == z_gt_.shape == (1, 7, Z) and z_.dtype == np.float32
    np.testing.assert_array_equal(z_[:, 0], z_gt_[:, 0])                           # both start from the scene's first code
    np.testing.assert_array_equal(z_[:, :, -P:], z_gt_[:, :, -P:])                 # the supervised parameters are the ground truth's
    assert np.abs(z_[:, 1:, :Z - P] - z_gt_[:, 1:, :Z - P]).max() > 0
    # de-normalising undoes data_nn.py:71-78: z_gt is the auto-encoder's own codes of the test scene
    truth = np.concatenate([code["x"][12:13], code["y"][12:]])[None]
    assert np.abs(z_gt_ - truth).max() < 1e-5 * np.abs(truth).max()
