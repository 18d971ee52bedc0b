"""GPU side of the sample sheets: the fused plane-view kernels (views.hip) against fixtures captured from the reference
(tests/golden/make_golden_views.py) and against the composition of existing ops, and the trainers' PNG sheets."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "views.npz")
KEYS = ("xy", "zy", "xym", "zym")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def _cases3(g):
    return sorted(k[:-3] for k in g if k.startswith("v3_") and k.endswith("_in"))


def _check_projection(got, want, tag):
    """Projected views: the fp32 mean may be summed in another order than the reference's, so a value that sits on an integer step may
    land on the neighbouring grey level -- never further, and in at most 0.1 % of a view's pixels."""
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    n = int((diff != 0).sum())
    print("projection %-22s %6d pixels, %d differ, max step %d" % (tag, diff.size, n, int(diff.max())))
    assert diff.max() <= 1, tag
    assert n <= 0.001 * diff.size, (tag, n, diff.size)
    return n


def test_plane_views_equal_the_reference(g):
    from deep_fluids_amd import ops
    cases = _cases3(g)
    assert len(cases) >= 9
    for tag in cases:
        x = dev(g[tag + "_in"])
        views = ops.denorm_img3(x)
        assert sorted(views) == sorted(KEYS)
        for k in KEYS:
            got = views[k]
            assert got.dtype == torch.uint8 and got.is_cuda
            one = ops.plane_view(x, xy_plane=k[0] == "x", project=not k.endswith("m"))      # the other outputs null
            assert torch.equal(one, got)
            want = g["%s_%s" % (tag, k)]
            assert tuple(got.shape) == want.shape
            if k.endswith("m"):
                np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=tag + k)     # no reduction: exact
            else:
                _check_projection(got.cpu().numpy(), want, tag + "_" + k)


def test_velocity_views_mid_slices_equal_the_reference_and_the_composition(g):
    from deep_fluids_amd import ops
    cases = [t for t in _cases3(g) if t.endswith("_c3")]
    assert len(cases) >= 5
    big = torch.randn((2, 64, 96, 64, 3), generator=torch.Generator().manual_seed(5)) * 0.5
    inputs = [(t, dev(g[t + "_in"])) for t in cases] + [("64x96x64x2", big.cuda())]
    for tag, u in inputs:
        vu, vc = ops.velocity_views3(u)
        want_u = ops.denorm_img3(u)
        want_c = ops.denorm_img3(ops.curl3(u))
        for k in KEYS:
            assert vu[k].dtype == torch.uint8 and vc[k].dtype == torch.uint8
            assert torch.equal(vu[k], want_u[k]), (tag, k)          # bit for bit
            assert torch.equal(vc[k], want_c[k]), (tag, k)
        if tag in cases:
            for k in ("xym", "zym"):
                np.testing.assert_array_equal(vu[k].cpu().numpy(), g["%s_%s" % (tag, k)])
            for k in ("xy", "zy"):
                _check_projection(vu[k].cpu().numpy(), g["%s_%s" % (tag, k)], "velocity " + tag + "_" + k)
        # two launches on the same input: bitwise equal
        vu2, vc2 = ops.velocity_views3(u)
        again = ops.denorm_img3(u)
        for k in KEYS:
            assert torch.equal(vu[k], vu2[k]) and torch.equal(vc[k], vc2[k]) and torch.equal(want_u[k], again[k])


def test_projections_at_the_flagship_grid_against_fp64():
    """64x96x64 (not a fixture: 4.7 MB per sample): the z / x means against a float64 mean of the same fp32 data."""
    from deep_fluids_amd import ops
    x = (torch.randn((2, 64, 96, 64, 3), generator=torch.Generator().manual_seed(6)) * 0.5)
    views = ops.denorm_img3(x.cuda())
    x64 = x.numpy().astype(np.float64)
    want = {"xy": x64.mean(axis=1), "zy": x64.mean(axis=3).transpose(0, 2, 1, 3)}
    for k, w in want.items():
        w8 = np.clip((w.astype(np.float32) + np.float32(1)) * np.float32(127.5), 0, 255).astype(np.uint8)
        _check_projection(views[k].cpu().numpy(), w8, "64x96x64 " + k)
    np.testing.assert_array_equal(views["xym"].cpu().numpy(), np.clip((x.numpy()[:, 32] + 1) * 127.5, 0, 255).astype(np.uint8))
    np.testing.assert_array_equal(views["zym"].cpu().numpy(),
                                  np.clip((x.numpy()[:, :, :, 32].transpose(0, 2, 1, 3) + 1) * 127.5, 0, 255).astype(np.uint8))


def test_denorm_img2d_equals_the_reference(g):
    from deep_fluids_amd import ops
    for c in (1, 2, 3, 4):
        x = g["d2_c%d_in" % c]
        got = ops.denorm_img(dev(x))
        assert got.dtype == torch.uint8
        np.testing.assert_array_equal(got.cpu().numpy(), g["d2_c%d_nhwc" % c])
        got = ops.denorm_img(dev(x.transpose(0, 3, 1, 2)), data_format="NCHW")
        np.testing.assert_array_equal(got.cpu().numpy(), g["d2_c%d_nchw" % c])
    x = dev(g["d2_c2_in"])
    assert torch.equal(ops.denorm_img(ops.add_channels(x)), ops.denorm_img(x))
    x4 = dev(g["d2_c4_in"])
    assert torch.equal(ops.denorm_img(ops.remove_channels(x4).contiguous()), ops.denorm_img(x4))
    # odd byte counts (the last 32-bit word is partial) and a larger picture
    for shape in ((1, 3, 3, 1), (3, 5, 7, 3), (2, 128, 96, 2)):
        t = torch.randn(shape, generator=torch.Generator().manual_seed(1))
        v = t.numpy() if shape[-1] != 2 else np.concatenate([t.numpy(), np.zeros(shape[:-1] + (1,), np.float32)], axis=-1)
        np.testing.assert_array_equal(ops.denorm_img(t.cuda()).cpu().numpy(), np.clip((v + 1) * 127.5, 0, 255).astype(np.uint8))


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _train_setup(tmp_path, is_3d, sample_images, b=2, **over):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset
    from deep_fluids_amd.trainer import Trainer, Trainer3, default_config
    spatial = (8, 16, 8) if is_3d else (16, 8)
    root = str(tmp_path / "data")
    n = write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=4)
    model_dir = str(tmp_path / ("run_%d" % int(sample_images)))
    cfg = default_config(is_3d=is_3d, res_x=8, res_y=16, res_z=8, filters=16, batch_size=b, num_samples=n, model_dir=model_dir,
                         log_step=2, test_step=2, sample_images=sample_images, **over)
    dcfg = SimpleNamespace(random_seed=123, data_path=root, is_3d=is_3d, arch="de", data_type="velocity", batch_size=b,
                           res_x=8, res_y=16, res_z=8 if is_3d else 1, num_worker=1)
    ops.reset_variables()
    tr = (Trainer3 if is_3d else Trainer)(cfg)
    return tr, BatchManager(dcfg), model_dir


TODAY_FILES = ["0_G.npz", "2_G.npz", "model.ckpt-3.npz", "params.json", "scalars.jsonl"]      # what train(max_step=3, test_step=2) writes today


@pytest.mark.parametrize("is_3d", [False, True])
def test_train_without_sample_images_writes_what_it_wrote_before(tmp_path, is_3d):
    tr, bm, model_dir = _train_setup(tmp_path, is_3d, False)
    tr.train(bm, max_step=3)
    assert sorted(os.listdir(model_dir)) == TODAY_FILES
    with np.load(os.path.join(model_dir, "2_G.npz")) as d:
        assert d["G"].shape == ((3, 2, 8, 16, 8, 3) if is_3d else (3, 2, 16, 8, 2)) and d["z"].shape == (3, 2, 3)


@pytest.mark.parametrize("graph", [False, True])
def test_trainer3_sample_images(tmp_path, graph):
    from deep_fluids_amd import ops, util
    tr, bm, model_dir = _train_setup(tmp_path, True, True, graph=graph)
    tr.train(bm, max_step=3)
    b = 2
    sheets = ["%d_%s.png" % (s, t) for s in (0, 2) for t in ("xym", "zym")] + ["x_fixed_%s_%d.png" % (t, s) for s in (0, 2) for t in ("xym", "zym")]
    want = sorted(sheets + ["x_fixed_xym_gt.png", "x_fixed_zym_gt.png", "x_fixed_gt.txt", "model.ckpt-3.npz", "params.json", "scalars.jsonl"])
    assert sorted(os.listdir(model_dir)) == want
    # the reference's sheet sizes: rows of b pictures, cells of (h + 1) x (w + 1), origin 1 (padding = 1)
    assert _png(os.path.join(model_dir, "2_xym.png")).shape == (6 * 17 + 1, b * 9 + 1, 3)        # 3 sweeps + their 3 curls
    assert _png(os.path.join(model_dir, "2_zym.png")).shape == (6 * 17 + 1, b * 9 + 1, 3)
    assert _png(os.path.join(model_dir, "x_fixed_xym_2.png")).shape == (2 * 17 + 1, b * 9 + 1, 3)
    assert _png(os.path.join(model_dir, "x_fixed_xym_gt.png")).shape == (2 * 17 + 1, b * 9 + 1, 3)
    assert _png(os.path.join(model_dir, "x_fixed_zym_gt.png")).shape == (2 * 17 + 1, b * 9 + 1, 3)
    lines = open(os.path.join(model_dir, "x_fixed_gt.txt")).read().split("\n")
    p, z = eval(lines[0]), eval(lines[1])
    assert len(p) == b and all(len(v) == 3 for v in p)
    assert z == [[pi / float(n - 1) * 2 - 1 for pi, n in zip(pp, bm.y_num)] for pp in p]
    # every sheet again, from the trained weights, with the views computed separately (curl3 materialised, one view per launch)
    z_samples = []
    for i in range(3):
        zi = np.zeros((b, 3), np.float32)
        zi[:, i] = np.linspace(-1, 1, num=b)
        z_samples.append(zi)
    z_samples.append(np.asarray(z, np.float32))
    out = str(tmp_path / "again")
    paths = tr.sample_images(z_samples, out, 7)
    assert sorted(os.path.basename(q) for q in paths) == sorted(["7_xym.png", "7_zym.png", "x_fixed_xym_7.png", "x_fixed_zym_7.png"])
    fields = [tr.generate(dev(zz)) for zz in z_samples]
    for tag, xy_plane in (("xym", True), ("zym", False)):
        vel = [ops.plane_view(f, xy_plane=xy_plane, project=False).cpu().numpy() for f in fields]
        vort = [ops.plane_view(ops.curl3(f), xy_plane=xy_plane, project=False).cpu().numpy() for f in fields]
        np.testing.assert_array_equal(_png(os.path.join(out, "7_%s.png" % tag)),
                                      util.make_grid(np.concatenate(vel[:-1] + vort[:-1]), nrow=b, padding=1))
        np.testing.assert_array_equal(_png(os.path.join(out, "x_fixed_%s_7.png" % tag)),
                                      util.make_grid(np.concatenate([vel[-1], vort[-1]]), nrow=b, padding=1))
        # (the last training step changed nothing after the step-2 sheets were written: max_step - 1 == 2)
        np.testing.assert_array_equal(_png(os.path.join(model_dir, "2_%s.png" % tag)), _png(os.path.join(out, "7_%s.png" % tag)))
    ops.reset_variables()


def test_trainer_2d_sample_images(tmp_path):
    from deep_fluids_amd import ops, util
    tr, bm, model_dir = _train_setup(tmp_path, False, True)
    tr.train(bm, max_step=3)
    b = 2
    want = sorted(["%d_%s.png" % (s, t) for s in (0, 2) for t in ("c", "cv")] + ["x_fixed_0.png", "x_fixed_2.png", "x_fixed_gt.png",
                  "x_fixed_gt.txt", "model.ckpt-3.npz", "params.json", "scalars.jsonl"])
    assert sorted(os.listdir(model_dir)) == want
    # rows of b pictures, cells of (h + 2) x (w + 2), origin 2 (padding = 2)
    assert _png(os.path.join(model_dir, "2_c.png")).shape == (3 * 18 + 2, b * 10 + 2, 3)
    assert _png(os.path.join(model_dir, "2_cv.png")).shape == (3 * 18 + 2, b * 10 + 2, 3)
    assert _png(os.path.join(model_dir, "x_fixed_2.png")).shape == (2 * 18 + 2, b * 10 + 2, 3)
    assert _png(os.path.join(model_dir, "x_fixed_gt.png")).shape == (2 * 18 + 2, b * 10 + 2, 3)
    lines = open(os.path.join(model_dir, "x_fixed_gt.txt")).read().split("\n")
    p, z = eval(lines[0]), eval(lines[1])
    assert z == [[pi / float(n - 1) * 2 - 1 for pi, n in zip(pp, bm.y_num)] for pp in p]
    z_samples = []
    for i in range(3):
        zi = np.zeros((b, 3), np.float32)
        zi[:, i] = np.linspace(-1, 1, num=b)
        z_samples.append(zi)
    z_samples.append(np.asarray(z, np.float32))
    out = str(tmp_path / "again")
    tr.sample_images(z_samples, out, 7)
    imgs = []
    for zz in z_samples:
        f = tr.generate(dev(zz)).cpu().numpy()                                     # [b,16,8,2]: the picture by hand
        f = np.concatenate([f, np.zeros(f.shape[:-1] + (1,), np.float32)], axis=-1)
        imgs.append(np.clip((f + 1) * 127.5, 0, 255).astype(np.uint8))
    c = np.concatenate(imgs[:-1])
    np.testing.assert_array_equal(_png(os.path.join(out, "7_c.png")), util.make_grid(c, nrow=b))
    np.testing.assert_array_equal(_png(os.path.join(out, "7_cv.png")), util.make_grid(util.vort_image(c / 127.5 - 1, True), nrow=b))
    np.testing.assert_array_equal(_png(os.path.join(out, "x_fixed_7.png")),
                                  util.make_grid(np.concatenate([imgs[-1], util.vort_image(imgs[-1] / 127.5 - 1, True)]), nrow=b))
    np.testing.assert_array_equal(_png(os.path.join(model_dir, "2_c.png")), _png(os.path.join(out, "7_c.png")))
    ops.reset_variables()


@pytest.mark.parametrize("is_3d,spatial", [(False, (16, 16)), (True, (8, 16, 8))])
def test_ae_trainer_autoencode(tmp_path, is_3d, spatial):
    from deep_fluids_amd import ops, util
    from deep_fluids_amd.data import BatchManager, write_synthetic_ae_dataset
    from deep_fluids_amd.trainer import AETrainer, default_config
    ops.reset_variables()
    root = str(tmp_path / "data")
    n = write_synthetic_ae_dataset(root, spatial, num_scenes=2, num_frames=4, seed=3)
    dcfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=is_3d, arch="ae", data_type="velocity", batch_size=2,
                           res_x=spatial[-1], res_y=spatial[-2], res_z=spatial[0] if is_3d else 1, num_worker=1)
    bm = BatchManager(dcfg, device="cuda")
    cfg = default_config(is_3d=is_3d, res_x=spatial[-1], res_y=spatial[-2], res_z=spatial[0] if is_3d else 1, filters=8, batch_size=2,
                         num_samples=n, z_num=6, p_num=2 if is_3d else 1, arch="ae")
    tr = AETrainer(cfg)
    out = str(tmp_path / "sheets")
    if is_3d:
        s = bm.random_list(2)
        paths = tr.autoencode(s["x"], out, 5)
        assert [os.path.basename(q) for q in paths] == ["xym_5.png", "zym_5.png"]
        rec = tr.reconstruct(dev(s["x"]))
        for tag, q in zip(("xym", "zym"), paths):
            view = ops.plane_view(rec, xy_plane=tag == "xym", project=False).cpu().numpy()
            np.testing.assert_array_equal(_png(q), util.make_grid(view, nrow=2))
        assert _png(paths[0]).shape == (18 + 2, 2 * 10 + 2, 3) and _png(paths[1]).shape == (18 + 2, 2 * 10 + 2, 3)
    else:
        xs, _, _ = bm.random_list(2)
        paths = tr.autoencode(xs, out, 5)
        assert [os.path.basename(q) for q in paths] == ["5.png"]
        rec = ops.denorm_img(tr.reconstruct(dev(xs[..., :-1] / 127.5 - 1))).cpu().numpy()
        want = np.concatenate([rec, util.vort_image(rec / 127.5 - 1, normalize=False)])          # 'ae': the vorticity keeps its scale
        np.testing.assert_array_equal(_png(paths[0]), util.make_grid(want, nrow=2))
        assert _png(paths[0]).shape == (2 * 18 + 2, 2 * 18 + 2, 3)
    ops.reset_variables()
