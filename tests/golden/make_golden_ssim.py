#!/usr/bin/env python3
"""Capture the fixtures of SSIM / MS-SSIM by EXECUTING the reference's own ``ops.py`` functions ``fspecial_gauss``, ``ssim`` and
``ms_ssim``: ``tests/golden/ssim.npz``.

Runs only where a checkout of the reference is at hand (``DF_REFERENCE``, default: where make_golden.py looks); it never travels with
the tests.  As in make_golden.py a NumPy-backed ``tensorflow`` stub stands in for TF 1.15; this script adds exactly the names the three
functions touch -- ``constant, exp, reduce_sum, reduce_mean, reduce_prod, stack, nn.conv2d`` ('VALID'), ``nn.avg_pool`` ('SAME') and
``get_shape()`` with ``.value`` dimensions -- with their published semantics, computing in float64 from float32 inputs.

Only numbers are written: what the reference's functions returned for the seeded inputs of tests/ssim_ref.py (a checksum of each input
stands for it; the small ones are stored whole), one plane per map (the reference's C channels are asserted equal here).  For the largest
shape the maps are stored for C = 2 only, the per-image means for every C: the file stays a few hundred KB.

Usage:  python tests/golden/make_golden_ssim.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402  (the stub of the stencil / model fixtures; reused, not changed)
import ssim_ref as ref  # noqa: E402

REF = os.environ.get("DF_REFERENCE", mg.REF)
F64 = np.float64


class _Dim(object):
    def __init__(self, v):
        self.value = int(v)


class T(np.ndarray):
    """ndarray that answers ``get_shape()`` the way ``ssim`` reads it: indexable, ``.value`` per dimension"""

    def get_shape(self):
        return [_Dim(s) for s in self.shape]


def _t(a):
    return np.asarray(a, F64).view(T)


def _conv2d_valid(x, w, strides, padding):
    assert list(strides) == [1, 1, 1, 1] and padding == "VALID"
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    kh, kw = w.shape[:2]
    oh, ow = x.shape[1] - kh + 1, x.shape[2] - kw + 1
    out = np.zeros((x.shape[0], oh, ow, w.shape[3]))
    for i in range(kh):
        for j in range(kw):
            out += x[:, i:i + oh, j:j + ow, :] @ w[i, j]
    return _t(out)


def _avg_pool_same(x, ksize, strides, padding):
    assert list(ksize) == [1, 2, 2, 1] and list(strides) == [1, 2, 2, 1] and padding == "SAME"
    x = np.asarray(x, F64)
    N, H, W, C = x.shape
    ph, pw = (H + 1) // 2, (W + 1) // 2
    pad = np.zeros((N, 2 * ph, 2 * pw, C))
    cnt = np.zeros((1, 2 * ph, 2 * pw, 1))
    pad[:, :H, :W] = x
    cnt[:, :H, :W] = 1
    s = lambda v: v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]      # noqa: E731
    return _t(s(pad) / s(cnt))                                       # 'SAME' averages the elements that exist


def install_stub():
    mg.install_stub()
    tf = sys.modules["tensorflow"]
    tf.constant = lambda x, dtype=None: _t(x)                         # float64 throughout: the coordinates are exact in either
    tf.exp = lambda x: _t(np.exp(np.asarray(x, F64)))
    tf.reduce_sum = lambda x: F64(np.sum(np.asarray(x, F64)))
    tf.reduce_mean = lambda x: F64(np.mean(np.asarray(x, F64)))
    tf.reduce_prod = lambda x: F64(np.prod(np.asarray(x, F64)))
    tf.stack = lambda xs, axis=0: _t(np.stack([np.asarray(x, F64) for x in xs], axis=axis))
    tf.nn.conv2d = _conv2d_valid
    tf.nn.avg_pool = _avg_pool_same


def _plane(m):
    m = np.asarray(m, F64)
    assert all(np.array_equal(m[..., 0], m[..., c]) or np.allclose(m[..., 0], m[..., c], rtol=1e-14, atol=0) for c in range(m.shape[-1]))
    return m[..., 0].copy()


def capture(ops):
    out = {}
    for size, sigma in ref.WINDOWS:
        for c in (1, 3):
            out["g_s%d_c%d" % (size, c)] = np.asarray(ops.fspecial_gauss(size, sigma, c), F64)
    for (H, W), _ in ref.SSIM_SHAPES:
        for c in ref.SSIM_CHANNELS:
            x, g = ref.inputs((H, W), c)
            key = "ssim_%dx%d_c%d" % (H, W, c)
            out[key + "_check"] = ref.checksum(g, x)
            if H * W <= 204:
                out[key + "_in_g"], out[key + "_in_x"] = g, x
            r = ops.ssim(_t(g), _t(x), mean_metric=False)
            sm, cm = _plane(r["ssim_map"]), _plane(r["cs_map"])
            size = min(11, H, W)
            assert np.asarray(r["g"]).shape == (size, size, c, c) and sm.shape == (ref.SSIM_N, H - size + 1, W - size + 1)
            out[key + "_mean"], out[key + "_mean_cs"] = sm.mean(axis=(1, 2)), cm.mean(axis=(1, 2))
            out[key + "_batch_mean"] = np.asarray(ops.ssim(_t(g), _t(x)), F64)
            if (H, W) != (64, 70) or c == 2:
                out[key + "_ssim_map"], out[key + "_cs_map"] = sm, cm
    for (H, W), c in ref.MS_CASES:
        for noise in ref.MS_NOISE:
            x, g = ref.inputs((H, W), c, noise, ref.MS_N)
            key = "ms_%dx%d_c%d_s%d" % (H, W, c, int(round(noise * 1000)))
            out[key + "_check"] = ref.checksum(g, x)
            a, b = _t(g), _t(x)
            mssim, mcs = [], []
            for k in range(len(ref.WEIGHTS)):                        # the levels as ms_ssim walks them, with the reference's own calls
                r = ops.ssim(a, b, mean_metric=False)
                mssim.append(np.mean(np.asarray(r["ssim_map"]))); mcs.append(np.mean(np.asarray(r["cs_map"])))
                if ((H, W), c) == ref.POOL_CASE and noise == ref.MS_NOISE[0] and k > 0:
                    out[key + "_pool%d_g" % k], out[key + "_pool%d_x" % k] = np.asarray(a, F64), np.asarray(b, F64)
                a = sys.modules["tensorflow"].nn.avg_pool(a, [1, 2, 2, 1], [1, 2, 2, 1], padding="SAME")
                b = sys.modules["tensorflow"].nn.avg_pool(b, [1, 2, 2, 1], [1, 2, 2, 1], padding="SAME")
            # the condition on the MS-SSIM inputs: no fractional power of a non-positive number on either side
            assert min(mcs[:-1]) > 0 and mssim[-1] > 0, (key, mcs, mssim)
            value = F64(ops.ms_ssim(_t(g), _t(x)))
            w = np.asarray(ref.WEIGHTS)
            assert np.isclose(value, np.prod(np.asarray(mcs[:-1]) ** w[:-1]) * mssim[-1] ** w[-1], rtol=1e-13, atol=0)
            out[key + "_mssim"], out[key + "_mcs"], out[key + "_value"] = np.asarray(mssim), np.asarray(mcs), value
            print("%s: level means cs %s ssim[4] %.4f -> %.6f" % (key, " ".join("%.4f" % v for v in mcs), mssim[-1], value))
    # one case with the second image negated: a level mean goes negative and the reference returns NaN
    (H, W), c = ref.MS_CASES[0]
    x, g = ref.inputs((H, W), c, ref.MS_NOISE[0], ref.MS_N)
    with np.errstate(invalid="ignore"):
        value = F64(ops.ms_ssim(_t(g), _t(-x)))
    assert np.isnan(value)
    out["ms_negated_value"] = value
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    print("ssim.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


def main():
    install_stub()
    sys.path.insert(0, REF)
    import ops       # the reference's own module
    capture(ops)


if __name__ == "__main__":
    main()
