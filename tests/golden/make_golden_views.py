#!/usr/bin/env python3
"""Capture the fixtures of the sample-sheet path by EXECUTING the reference's own ``ops.py`` / ``util.py`` / ``data.py`` /
``trainer.py`` functions: ``tests/golden/views.npz`` and the colour table ``deep_fluids_amd/rdbu_256.txt``.

Runs only where a checkout of the reference is at hand (``DF_REFERENCE``, default: where make_golden.py looks); it never travels with the tests.  As in
make_golden.py a NumPy-backed ``tensorflow`` stub stands in for TF 1.15; this script adds the calls the image functions make
(``reduce_mean, slice, squeeze, clip_by_value, cast, zeros, split``) and an empty ``imageio`` so that the reference's ``util.py``
imports.  The stubbed ``plane_view`` is pinned against the reference's own NumPy twin ``plane_view_np`` before anything is written.

Only numbers are written: seeded inputs and what the reference's functions returned for them.

Usage:  python tests/golden/make_golden_views.py
"""
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402  (the stub of the stencil / model fixtures; reused, not changed)

_t = mg._t
REF = os.environ.get("DF_REFERENCE", mg.REF)

# 3-D cases: tag -> (shape [B,Z,Y,X], channel counts, sigma).  Ragged extents, odd Z and X (Z//2, X//2), X*C both a multiple of 4 and
# not, one Z above 16 (more than one chunk of the kernel's z walk), and one sigma = 1 input that reaches both clip ends.
CASES3 = {
    "r567": ((2, 5, 6, 7), (1, 2, 3, 4), 0.5),
    "r13": ((1, 13, 10, 7), (3, 4), 0.5),
    "m16": ((1, 16, 24, 16), (3,), 0.5),
    "z19": ((1, 19, 4, 6), (3,), 0.5),
    "s1": ((1, 7, 9, 12), (3,), 1.0),
}


def install_stub():
    mg.install_stub()
    tf = sys.modules["tensorflow"]
    tf.uint8 = np.uint8
    tf.reduce_mean = lambda x, axis: _t(np.mean(np.asarray(x), axis=axis))

    def _slice(x, begin, size):
        x = np.asarray(x)
        idx = tuple(slice(b, None if s == -1 else b + s) for b, s in zip(begin, size))
        return _t(x[idx])
    tf.slice = _slice
    tf.squeeze = lambda x, axis: _t(np.squeeze(np.asarray(x), axis=tuple(axis)))
    tf.clip_by_value = lambda x, lo, hi: _t(np.clip(np.asarray(x), lo, hi))
    tf.cast = lambda x, dtype: _t(np.asarray(x).astype(dtype))          # float -> uint8 truncates, like tf.cast
    tf.zeros = lambda shape, dtype=np.float32: _t(np.zeros(shape, dtype))

    def _split(x, sizes, axis):
        x = np.asarray(x)
        cuts = np.cumsum([s for s in sizes[:-1]])
        return [_t(p) for p in np.split(x, cuts, axis=axis)]
    tf.split = _split
    sys.modules["imageio"] = types.ModuleType("imageio")


def capture(ops, util, data, trainer):
    rng = np.random.RandomState(123)
    out = {}
    for tag, (shape, chans, sigma) in CASES3.items():
        for c in chans:
            x = (rng.randn(*(shape + (c,))) * sigma).astype(np.float32)
            key = "v3_%s_c%d" % (tag, c)
            out[key + "_in"] = x
            imgs = ops.denorm_img3(_t(x))
            for k in ("xy", "zy", "xym", "zym"):
                got = np.asarray(imgs[k])
                assert got.dtype == np.uint8
                one = np.asarray(ops.plane_view(_t(x), xy_plane=k[0] == "x", project=not k.endswith("m")))
                assert np.array_equal(one, got)
                # pin the stub: the reference's own NumPy twin, run as it is, must agree once cast
                twin = np.stack([ops.plane_view_np(x[b], xy_plane=k[0] == "x", project=not k.endswith("m")) for b in range(shape[0])])
                assert np.array_equal(twin.astype(np.uint8), got), (key, k)
                out[key + "_" + k] = got
                if c == 3:
                    out[key + "_np_" + k] = twin
            if sigma >= 1.0:
                allv = np.concatenate([np.asarray(imgs[k]).ravel() for k in ("xym", "zym")])
                assert allv.min() == 0 and allv.max() == 255          # both clip ends are hit
    for c in (1, 2, 3, 4):
        x = (rng.randn(2, 6, 5, c) * 0.7).astype(np.float32)
        out["d2_c%d_in" % c] = x
        out["d2_c%d_nhwc" % c] = np.asarray(ops.denorm_img(_t(x), data_format="NHWC"))
        xc = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
        out["d2_c%d_nchw" % c] = np.asarray(ops.denorm_img(_t(xc), data_format="NCHW"))
        assert np.array_equal(out["d2_c%d_nhwc" % c], out["d2_c%d_nchw" % c])
    # sheets
    for tag, (n, h, w, ch, nrow, pad, flip) in {"a": (5, 4, 6, 3, 3, 2, True), "b": (4, 4, 6, 3, 4, 1, True),
                                                "c": (3, 5, 3, 1, 8, 2, False), "d": (7, 3, 4, 3, 2, 1, True)}.items():
        t = rng.randint(0, 256, size=(n, h, w, ch)).astype(np.uint8)
        out["grid_%s_in" % tag] = t
        out["grid_%s_args" % tag] = np.array([nrow, pad, int(flip)])
        out["grid_%s_out" % tag] = util.make_grid(t, nrow=nrow, padding=pad, flip=flip)
    # get_vort_image on a de-quantised uint8 picture, as generate() calls it (trainer.py:760,767)
    img = rng.randint(0, 256, size=(3, 6, 5, 3)).astype(np.uint8)
    out["vort_in"] = img
    for arch in ("de", "ae"):
        got = trainer.Trainer.get_vort_image(types.SimpleNamespace(arch=arch), img / 127.5 - 1)
        assert got.dtype == np.uint8 and got.shape == (3, 6, 5, 3)
        out["vort_%s" % arch] = got
    flat = np.zeros((1, 4, 4, 3), np.uint8) + 100                       # zero vorticity: 0/0 under normalisation
    out["vort_flat_in"] = flat
    with np.errstate(all="ignore"):
        out["vort_flat_de"] = trainer.Trainer.get_vort_image(types.SimpleNamespace(arch="de"), flat / 127.5 - 1)
    # one random_list3d sample on the synthetic dataset the tests can write again (seeded)
    from deep_fluids_amd.data import write_synthetic_dataset
    with tempfile.TemporaryDirectory() as tmp:
        write_synthetic_dataset(tmp, (6, 8, 5), num_p=(3, 2), num_frames=4, seed=7)
        args = {}
        for line in open(os.path.join(tmp, "args.txt")):
            k, v = line.rstrip("\n").split(": ")
            args[k] = v
        r = np.loadtxt(os.path.join(tmp, "v_range.txt"))
        bm = types.SimpleNamespace(rng=np.random.RandomState(11), root=tmp, data_type="velocity", args=args, y_num=[3, 2, 4],
                                   x_range=max(abs(r[0]), abs(r[1])), y_range=[[0.2, 0.8], [0.04, 0.12], [0.0, 3.0]])
        bm.list_from_p = lambda pl: data.BatchManager.list_from_p(bm, pl)
        s = data.BatchManager.random_list3d(bm, 2)
        out["rl3_p"] = np.array(s["p"]); out["rl3_z"] = np.array(s["z"])
        for k in ("x", "y", "xy", "zy", "xym", "zym", "xy_c", "zy_c", "xym_c", "zym_c"):
            out["rl3_" + k] = np.asarray(s[k])
    np.savez_compressed(os.path.join(HERE, "views.npz"), **out)
    print("views.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "views.npz"))))


def write_rdbu():
    """uint8(RdBu(i) * 255) for i = 0..255: an integer argument indexes the colour map's 256-entry lookup table directly."""
    import matplotlib.pyplot as plt
    t = np.uint8(plt.cm.RdBu(np.arange(256)) * 255)[:, :3]
    assert t.shape == (256, 3)
    np.savetxt(os.path.join(ROOT, "deep_fluids_amd", "rdbu_256.txt"), t, fmt="%d",
               header="RdBu colour map, 256 entries: uint8(RdBu(i) * 255) as 'R G B' per line (tests/golden/make_golden_views.py)")
    print("rdbu_256.txt written")


def main():
    install_stub()
    sys.path.insert(0, REF)
    import ops       # the reference's own modules
    import util
    import data
    import trainer
    write_rdbu()
    capture(ops, util, data, trainer)


if __name__ == "__main__":
    main()
