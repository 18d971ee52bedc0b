"""Host side of the sample sheets (no GPU): plane_view_np, make_grid, save_image, vort_image and BatchManager.random_list against
fixtures captured from the reference (tests/golden/make_golden_views.py), and the argument checks of the three view entry points."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

from deep_fluids_amd import _lib, ops, util
from deep_fluids_amd.data import BatchManager, write_synthetic_dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views.npz")
KEYS = ("xy", "zy", "xym", "zym")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def _kw(k):
    return dict(xy_plane=k[0] == "x", project=not k.endswith("m"))


def test_plane_view_np_equals_the_reference(g):
    tags = sorted(k[:-3] for k in g if k.startswith("v3_") and k.endswith("_c3_in"))
    assert len(tags) >= 4
    for tag in tags:
        x = g[tag + "_in"]
        for k in KEYS:
            want = g["%s_np_%s" % (tag, k)]
            got = np.stack([ops.plane_view_np(x[b], **_kw(k)) for b in range(x.shape[0])])
            assert got.dtype == want.dtype and got.shape == want.shape
            np.testing.assert_array_equal(got, want)
            # float result, no uint8 cast; the cast of it is the tensor-side view
            np.testing.assert_array_equal(got.astype(np.uint8), g["%s_%s" % (tag, k)])


def test_make_grid_equals_the_reference(g):
    for tag in "abcd":
        nrow, pad, flip = (int(v) for v in g["grid_%s_args" % tag])
        got = util.make_grid(g["grid_%s_in" % tag], nrow=nrow, padding=pad, flip=bool(flip))
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, g["grid_%s_out" % tag])
    # the reference's sheet geometry, written out: cells of (h + p) x (w + p), origin 1 + p // 2
    t = np.full((5, 4, 6, 3), 9, np.uint8)
    assert util.make_grid(t, nrow=3, padding=2).shape == (2 * 6 + 2, 3 * 8 + 2, 3)
    assert util.make_grid(t, nrow=5, padding=1).shape == (5 + 1, 5 * 7 + 1, 3)


def test_vort_image_equals_the_reference(g):
    x = g["vort_in"] / 127.5 - 1
    np.testing.assert_array_equal(util.vort_image(x, normalize=True), g["vort_de"])
    np.testing.assert_array_equal(util.vort_image(x, normalize=False), g["vort_ae"])
    np.testing.assert_array_equal(util.vort_image(g["vort_flat_in"] / 127.5 - 1, normalize=True), g["vort_flat_de"])
    t = util.rdbu_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert t[0, 0] > t[0, 2] and t[255, 2] > t[255, 0]          # red end, blue end


def test_save_image_roundtrip(tmp_path, g):
    from PIL import Image
    t = g["grid_a_in"]
    path = str(tmp_path / "sheet.png")
    util.save_image(t, path, nrow=3, padding=2)
    np.testing.assert_array_equal(np.asarray(Image.open(path)), g["grid_a_out"])
    util.save_image(t[0], path, single=True)
    np.testing.assert_array_equal(np.asarray(Image.open(path)), t[0, ::-1])
    util.save_image(t[0], path, single=True, flip=False)
    np.testing.assert_array_equal(np.asarray(Image.open(path)), t[0])


def _manager(root, is_3d, seed=11, b=2, spatial=(6, 8, 5)):
    cfg = SimpleNamespace(random_seed=seed, data_path=root, is_3d=is_3d, data_type="velocity", arch="de", batch_size=b,
                          res_x=spatial[-1], res_y=spatial[-2], res_z=spatial[0] if is_3d else 1)
    return BatchManager(cfg, device=None)


def test_random_list_3d(tmp_path, g):
    write_synthetic_dataset(str(tmp_path), (6, 8, 5), num_p=(3, 2), num_frames=4, seed=7)
    bm = _manager(str(tmp_path), True)
    s = bm.random_list(2)
    assert sorted(s) == sorted(["x", "y", "xy", "zy", "xym", "zym", "xy_c", "zy_c", "xym_c", "zym_c", "p", "z"])
    assert s["x"].shape == (2, 6, 8, 5, 3) and s["y"].shape == (2, 3)
    for k in ("xy", "xym", "xy_c", "xym_c"):
        assert s[k].shape == (2, 8, 5, 3)
    for k in ("zy", "zym", "zy_c", "zym_c"):
        assert s[k].shape == (2, 8, 6, 3)
    for p, z in zip(s["p"], s["z"]):
        assert z == [pi / float(n - 1) * 2 - 1 for pi, n in zip(p, bm.y_num)]
    for i in range(2):
        for k in KEYS:
            np.testing.assert_array_equal(s[k][i], ops.plane_view_np(s["x"][i], **_kw(k)))
    # the reference's own random_list3d on the same dataset and seed
    for k in ("x", "y", "p", "z") + KEYS + tuple(k + "_c" for k in KEYS):
        np.testing.assert_array_equal(np.asarray(s[k]), g["rl3_" + k])
    assert bm.list_from_p([[2, 1, 3]]) == [os.path.join(str(tmp_path), "v", "2_1_3.npz")]


def test_random_list_2d(tmp_path):
    write_synthetic_dataset(str(tmp_path), (8, 6), num_p=(3, 2), num_frames=4, seed=3)
    bm = _manager(str(tmp_path), False, b=3, spatial=(8, 6))
    xs, pis, zis = bm.random_list(3)
    assert xs.shape == (3, 8, 6, 3) and len(pis) == len(zis) == 3
    assert xs.min() >= 0 and xs.max() <= 255
    np.testing.assert_array_equal(xs[..., 2], 127.5)              # the zero third channel of velocity data
    for p, z in zip(pis, zis):
        assert z == [pi / float(n - 1) * 2 - 1 for pi, n in zip(p, bm.y_num)]
        with np.load(bm.list_from_p([p])[0]) as d:
            x = (d["x"].astype(np.float32) / bm.x_range).astype(np.float32)
        np.testing.assert_array_equal(xs[pis.index(p)][..., :2], np.clip((x.astype(np.float64) + 1) * 127.5, 0, 255))
    # level-set data: thresholded at 0.5 before the mapping
    os.makedirs(str(tmp_path / "l"))
    rng = np.random.RandomState(0)
    for i in range(3):
        for j in range(2):
            for t in range(4):
                np.savez_compressed(str(tmp_path / "l" / ("%d_%d_%d.npz" % (i, j, t))), x=rng.uniform(-1, 2, (8, 6, 1)).astype(np.float32),
                                    y=np.array([0.5, 0.08, t], np.float32))
    with open(str(tmp_path / "l_range.txt"), "w") as f:
        f.write("-1\n1\n")
    cfg = SimpleNamespace(random_seed=5, data_path=str(tmp_path), is_3d=False, data_type="levelset", arch="de", batch_size=2, res_x=6,
                          res_y=8, res_z=1)
    xs, _, _ = BatchManager(cfg, device=None).random_list(4)
    assert xs.shape == (4, 8, 6, 1) and set(np.unique(xs)) <= {0.0, 255.0} and len(np.unique(xs)) == 2


def test_view_entry_points_reject_bad_arguments_before_the_device():
    h = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15
    o = a + 2048
    # df_plane_views3d(x, xy, zy, xym, zym, B, Z, Y, X, C, stream)
    assert h.df_plane_views3d(None, o, o, o, o, 1, 4, 4, 4, 3, None) == -1
    assert b"null input" in h.df_last_error()
    assert h.df_plane_views3d(a, None, None, None, None, 1, 4, 4, 4, 3, None) == -1
    assert b"output" in h.df_last_error()
    assert h.df_plane_views3d(a, o, o, o, o, 1, 0, 4, 4, 3, None) == -1
    for c in (0, 5):
        assert h.df_plane_views3d(a, o, o, o, o, 1, 4, 4, 4, c, None) == -2
        assert b"1..4" in h.df_last_error()
    assert h.df_plane_views3d(a + 2, o, o, o, o, 1, 4, 4, 4, 3, None) == -3
    assert b"aligned" in h.df_last_error()
    assert h.df_plane_views3d(a, o, o, o, o, 1, 4, 4, 1 << 20, 4, None) == -2          # a row-plane beyond the LDS
    assert b"LDS" in h.df_last_error()
    # df_velocity_views3d(u, xy, zy, xym, zym, cxy, czy, cxym, czym, B, Z, Y, X, stream)
    assert h.df_velocity_views3d(None, o, o, o, o, o, o, o, o, 1, 4, 4, 4, None) == -1
    assert b"null input" in h.df_last_error()
    assert h.df_velocity_views3d(a, None, None, None, None, None, None, None, None, 1, 4, 4, 4, None) == -1
    for ext in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        assert h.df_velocity_views3d(a, o, o, o, o, o, o, o, o, 1, ext[0], ext[1], ext[2], None) == -2      # a difference needs >= 2
        assert b">= 2" in h.df_last_error()
    assert h.df_velocity_views3d(a + 1, o, o, o, o, o, o, o, o, 1, 4, 4, 4, None) == -3
    assert b"aligned" in h.df_last_error()
    # df_denorm_img2d(x, out, B, H, W, C, nchw, stream)
    assert h.df_denorm_img2d(None, o, 1, 4, 4, 3, 0, None) == -1
    assert b"null input" in h.df_last_error()
    assert h.df_denorm_img2d(a, None, 1, 4, 4, 3, 0, None) == -1
    assert b"null output" in h.df_last_error()
    assert h.df_denorm_img2d(a, o, 1, 4, 0, 3, 0, None) == -1
    assert h.df_denorm_img2d(a, o, 1, 4, 4, 0, 1, None) == -2
    assert b"channel" in h.df_last_error()
    assert h.df_denorm_img2d(a + 2, o, 1, 4, 4, 3, 0, None) == -3
    assert b"aligned" in h.df_last_error()


def test_python_surface_of_the_views_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        return          # with a GPU the same calls are exercised by tests/test_gpu_views.py
    for fn, x in ((ops.denorm_img3, torch.zeros((1, 4, 4, 4, 3))), (ops.velocity_views3, torch.zeros((1, 4, 4, 4, 3))),
                  (ops.denorm_img, torch.zeros((1, 4, 4, 2))), (ops.plane_view, torch.zeros((1, 4, 4, 4, 1)))):
        with pytest.raises(_lib.DeepFluidsHipError):
            fn(x)
