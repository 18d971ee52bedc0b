"""SSIM / MS-SSIM on the MI355X (csrc/ssim.hip through ``ops.ssim`` / ``ms_ssim`` / ``field_ssim`` and the raw C ABI) against the NumPy
restatement of include/deepfluids_hip_ssim.h (tests/ssim_ref.py): the maps, the per-image rows and the pooled images are the fp32 twin
BIT FOR BIT, and within 4x the twin's own deviation of what the reference's functions returned (tests/golden/ssim.npz); an image does
not depend on its batch; two calls give the same bits; ``evaluate_(ssim=True)`` writes what direct calls return.

The MS-SSIM value is formed from the level means (bitwise the twin's) by fp64 ``pow`` and products on the device; the device's and
NumPy's ``pow`` may differ in the last fp64 place, which can move the fp32 rounding of the result by one place: it is asserted within
one fp32 ulp of the twin (2^-23 relative: values are below 1)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_ref as ref  # noqa: E402
from gpu_util import Guarded, assert_bits, dev, host  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim.npz")
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _raw(g, x, maps=True, pool=True, **kw):
    """one ``df_ssim`` call on guarded buffers: ``(rows int32 [N,8], ssim_map, cs_map, pool_g, pool_x)``"""
    from deep_fluids_amd import _lib, ops
    a = dict(ref.DEFAULTS)
    a.update(kw)
    N, H, W, C = g.shape
    size = min(a["filter_size"], H, W)
    taps = ops._ssim_taps(size, a["filter_sigma"] * size / a["filter_size"])[1]
    need = _lib.query("df_ssim_workspace_bytes", N, H, W, a["filter_size"])
    gi, xi = Guarded(g.shape, g), Guarded(x.shape, x)
    out, ws = Guarded((N, ref.WORDS)), Guarded((need // 4,))
    oshape, pshape = (N, H - size + 1, W - size + 1), (N, (H + 1) // 2, (W + 1) // 2, C)
    sm, cm = (Guarded(oshape), Guarded(oshape)) if maps else (None, None)
    pa, pb = (Guarded(pshape), Guarded(pshape)) if pool else (None, None)
    p = lambda b: None if b is None else b.ptr      # noqa: E731
    _lib.call("df_ssim", gi.ptr, xi.ptr, taps, p(sm), p(cm), p(pa), p(pb), out.ptr, ws.ptr, need, N, H, W, C, a["filter_size"],
              a["k1"], a["k2"], a["min_val"], a["max_val"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for b, what in ((gi, "g"), (xi, "x"), (ws, "workspace"), (out, "out")):
        b.check_guards(what)
    rows = host(out.payload()).view(np.int32).reshape(N, ref.WORDS)      # (half of an fp64 may look like a NaN: no NaN scan here)
    assert not (rows == np.int32(0x7FC5A5A5)).any(), "a word of out was never written"
    return (rows,) + tuple(None if b is None else b.get(what) for b, what in ((sm, "ssim_map"), (cm, "cs_map"), (pa, "pool_a"), (pb, "pool_b")))


@pytest.mark.parametrize("n", [1, ref.SSIM_N])
@pytest.mark.parametrize("channels", ref.SSIM_CHANNELS)
@pytest.mark.parametrize("shape", [s for s, _ in ref.SSIM_SHAPES], ids=lambda s: "%dx%d" % s)
def test_maps_rows_and_pooled_images_are_the_twin_bit_for_bit(golden, shape, channels, n):
    x, g = ref.inputs(shape, channels)
    twin, _ = ref.reference(shape, channels)
    rows, sm, cm, pg, px = _raw(g[:n], x[:n])
    assert_bits(sm, twin["ssim_map"][:n], "ssim_map")                  # image n of the batch of 3 is the image alone
    assert_bits(cm, twin["cs_map"][:n], "cs_map")
    np.testing.assert_array_equal(rows, ref.raw_words(twin)[:n])
    assert_bits(pg, ref.pool(g[:n]), "pool_a")
    assert_bits(px, ref.pool(x[:n]), "pool_b")
    again = _raw(g[:n], x[:n])
    for a, b in zip((rows, sm, cm, pg, px), again):                    # two calls: the same bits
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    lean = _raw(g[:n], x[:n], maps=False, pool=False)                  # the optional outputs change nothing
    np.testing.assert_array_equal(lean[0], rows)
    # ... and within 4x the twin's own deviation of the reference's numbers
    key = "ssim_%dx%d_c%d" % (shape + (channels,))
    means = rows[:, ref.CONST["mean"]].view(F32).astype(F64), rows[:, ref.CONST["mean_cs"]].view(F32).astype(F64)
    for got, tw, want in ((means[0], twin["mean"], golden[key + "_mean"]), (means[1], twin["mean_cs"], golden[key + "_mean_cs"])) + \
            (((sm, twin["ssim_map"], golden[key + "_ssim_map"]), (cm, twin["cs_map"], golden[key + "_cs_map"])) if key + "_ssim_map" in golden else ()):
        yard = np.abs(tw[:n].astype(F64) - want[:n]).max()
        assert np.abs(got.astype(F64) - want[:n]).max() <= 4 * yard, key


def test_an_image_does_not_depend_on_its_batch():
    x, g = ref.inputs((33, 45), 2)
    rows, sm, cm, pg, px = _raw(g, x)
    for i in range(ref.SSIM_N):
        one = _raw(g[i:i + 1], x[i:i + 1])
        for a, b in zip((rows, sm, cm, pg, px), one):
            np.testing.assert_array_equal(a[i:i + 1].view(np.int32), b.view(np.int32))


def test_other_arguments_follow_the_twin():
    x, g = ref.inputs((33, 45), 3)
    kw = dict(filter_size=8, filter_sigma=2.0, k1=0.02, k2=0.05, min_val=-1.5, max_val=2.0)
    twin = ref.ssim(g, x, F32, **kw)
    rows, sm, cm, _, _ = _raw(g, x, **kw)
    assert_bits(sm, twin["ssim_map"], "ssim_map")
    assert_bits(cm, twin["cs_map"], "cs_map")
    np.testing.assert_array_equal(rows, ref.raw_words(twin))


def test_pooled_chain_on_odd_and_even_extents():
    (H, W), c = ref.POOL_CASE
    x, g = ref.inputs((H, W), c, ref.MS_NOISE[0], ref.MS_N)
    for shape in [(19, 25), (10, 13), (5, 7), (3, 4)]:
        _, _, _, pg, px = _raw(g, x, maps=False)
        assert pg.shape == (ref.MS_N,) + shape + (c,)
        assert_bits(pg, ref.pool(g), "pool_a %s" % (shape,))
        assert_bits(px, ref.pool(x), "pool_b %s" % (shape,))
        g, x = pg, px


@pytest.mark.parametrize("noise", ref.MS_NOISE)
@pytest.mark.parametrize("shape,channels", ref.MS_CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "c%d" % v)
def test_ms_ssim(golden, shape, channels, noise):
    from deep_fluids_amd import ops
    x, g = ref.inputs(shape, channels, noise, ref.MS_N)
    twin, _ = ref.ms_reference(shape, channels, noise)
    key = "ms_%dx%d_c%d_s%d" % (shape + (channels, int(round(noise * 1000))))
    assert golden[key + "_mcs"][:-1].min() > 0 and golden[key + "_mssim"][-1] > 0      # the condition on the inputs
    gd, xd = dev(g), dev(x)
    ws = ops.SSIMWorkspace(g.shape, gd.device, 5, 11, 1)
    mean = host(ops._ssim_run("test", gd, xd, ws, 1.5, 0.01, 0.03, -1.0, 1.0))          # [5, 1, 2] fp64: the level means
    np.testing.assert_array_equal(mean[:, 0, 0].view(np.int64), twin["mssim"][:, 0].view(np.int64))
    np.testing.assert_array_equal(mean[:, 0, 1].view(np.int64), twin["mcs"][:, 0].view(np.int64))
    for k in range(1, 5):                                                # each level read the images the level before wrote
        assert_bits(host(ws.level[k - 1]["pool"][0]), twin["images"][k][0], "level %d" % k)
    v = ops.ms_ssim(gd, xd)
    assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    got, tw, want = float(v), float(twin["value"][0]), float(golden[key + "_value"])
    assert abs(got - tw) <= ULP * tw, (got, tw)
    assert abs(got - want) <= 4 * abs(tw - want) + ULP * want, (got, tw, want)
    assert float(ops.ms_ssim(gd, xd, mean_metric=False)) == got
    yard = np.abs(twin["mcs"][:, 0] - golden[key + "_mcs"]).max()
    assert np.abs(mean[:, 0, 1] - golden[key + "_mcs"]).max() <= 4 * yard


def test_ms_ssim_gives_nan_where_the_reference_does(golden):
    from deep_fluids_amd import ops
    (H, W), c = ref.MS_CASES[0]
    x, g = ref.inputs((H, W), c, ref.MS_NOISE[0], ref.MS_N)
    assert np.isnan(golden["ms_negated_value"])
    assert np.isnan(float(ops.ms_ssim(dev(g), dev(-x))))


def test_ssim_returns_the_mean_or_the_references_dict(golden):
    from deep_fluids_amd import ops
    shape, c = (12, 17), 3
    x, g = ref.inputs(shape, c)
    twin, _ = ref.reference(shape, c)
    m = ops.ssim(dev(g), dev(x))
    assert m.dim() == 0 and m.dtype == torch.float32 and m.is_cuda
    want = ref.group_mean(twin["sum"], twin["count"], 1)[0]
    assert float(m) == float(F32(want))
    yard = abs(float(F32(want)) - float(golden["ssim_12x17_c3_batch_mean"]))
    assert abs(float(m) - float(golden["ssim_12x17_c3_batch_mean"])) <= 4 * yard
    r = ops.ssim(dev(g), dev(x), mean_metric=False)
    assert sorted(r) == ["cs_map", "g", "ssim_map"]
    assert tuple(r["ssim_map"].shape) == (3, 2, 7, c) and tuple(r["cs_map"].shape) == (3, 2, 7, c) and tuple(r["g"].shape) == (11, 11, c, c)
    for k in range(c):
        assert_bits(host(r["ssim_map"][..., k]), twin["ssim_map"], "ssim_map")
        assert_bits(host(r["cs_map"][..., k]), twin["cs_map"], "cs_map")
    np.testing.assert_array_equal(host(r["g"]), golden["g_s11_c3"].astype(F32))
    small = ops.ssim(dev(g[:, :7]), dev(x[:, :7]), mean_metric=False)    # the window shrinks with the image
    assert tuple(small["g"].shape) == (7, 7, c, c) and tuple(small["ssim_map"].shape) == (3, 1, 11, c)


def test_field_ssim_is_the_2d_calls_combined():
    from deep_fluids_amd import ops
    x, g = ref.inputs((12, 17), 3, 0.05, 6)
    x5, g5 = x.reshape(2, 3, 12, 17, 3), g.reshape(2, 3, 12, 17, 3)
    twin = ref.ssim(g, x, F32)
    got = ops.field_ssim(dev(g5), dev(x5))
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,)
    np.testing.assert_array_equal(host(got).view(np.int64), ref.group_mean(twin["sum"], twin["count"], 2).view(np.int64))
    for b in range(2):                                                   # an entry: the fp64 totals of its slices' 2-D calls
        rows = _raw(g5[b], x5[b], maps=False, pool=False)[0]
        tot = np.ascontiguousarray(rows[:, ref.CONST["sum"]:ref.CONST["sum"] + 2]).view(F64)[:, 0]
        assert float(got[b]) == float(ref.group_mean(tot, 2 * 7, 1)[0])
    x2, g2 = ref.inputs((12, 17), 2, 0.05, 2)
    e = ops.field_ssim(dev(g2), dev(x2))
    for b in range(2):
        one = ops.ssim(dev(g2[b:b + 1]), dev(x2[b:b + 1]))
        assert float(e[b].float()) == float(one)
    ws = ops.ssim_workspace(dev(g5), multiscale=True)                    # a preallocated workspace gives the same bits, call after call
    m1 = host(ops.field_ssim(dev(g5), dev(x5), multiscale=True, workspace=ws)).copy()
    m2 = host(ops.field_ssim(dev(g5), dev(x5), multiscale=True, workspace=ws))
    m3 = host(ops.field_ssim(dev(g5), dev(x5), multiscale=True))
    np.testing.assert_array_equal(m1.view(np.int64), m2.view(np.int64))
    np.testing.assert_array_equal(m1.view(np.int64), m3.view(np.int64))
    tw = ref.ms_ssim(g, x, F64, groups=2)["value"]
    np.testing.assert_allclose(m1, tw, rtol=1e-5)
    same = ops.field_ssim(dev(x5), dev(x5))
    assert (host(same) == 1.0).all()                                     # a field against itself: exactly 1


def test_evaluate_with_ssim(tmp_path):
    import test_gpu_field_metrics as fm
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset, preprocess
    from deep_fluids_amd.trainer import EVAL_SSIM, Trainer, default_config
    ops.reset_variables()
    spatial = (16, 16)
    root = str(tmp_path / "data")
    write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=4, seed=5)
    bm = BatchManager(fm._data_cfg(root, spatial, "de"), device=None)
    cfg = default_config(is_3d=False, res_x=16, res_y=16, res_z=1, filters=8, batch_size=2, num_samples=24, use_curl=True,
                         model_dir=str(tmp_path / "model"), test_batch_size=2)
    tr = Trainer(cfg)
    plain = tr.evaluate_(bm, pairs=[(2, 1)], model_dir=str(tmp_path / "plain"))
    summary = tr.evaluate_(bm, pairs=[(2, 1)], ssim=True)
    z_c, _, _ = tr._sweep_codes(bm, 2, 1, 4, "test")
    truth = np.stack([preprocess(p, bm.data_type, bm.x_range, bm.y_range)[0] for p in bm.list_from_p([(2, 1, t) for t in range(4)])])
    want = {q: [] for q in EVAL_SSIM}
    for i in (0, 2):
        g, x = tr.generate(dev(z_c[i:i + 2])).contiguous(), dev(truth[i:i + 2])
        want["ssim"].append(host(ops.field_ssim(g, x)))
        want["ms_ssim"].append(host(ops.field_ssim(g, x, multiscale=True)))
        assert (host(ops.field_ssim(x, x)) == 1.0).all()                 # a frame against itself
    with np.load(os.path.join(summary["dir"], "2_1.npz")) as z, np.load(os.path.join(plain["dir"], "2_1.npz")) as z0:
        assert set(z.files) == set(z0.files) | set(EVAL_SSIM)
        for k in z0.files:
            np.testing.assert_array_equal(z[k], z0[k])
        for q in EVAL_SSIM:
            np.testing.assert_array_equal(z[q].view(np.int64), np.concatenate(want[q]).view(np.int64))
            st = summary["groups"]["2_1"]
            assert st[q + "_mean"] == float(np.mean(z[q])) and st[q + "_min"] == float(np.min(z[q])) and st[q + "_max"] == float(np.max(z[q]))
            assert summary["total"][q + "_mean"] == st[q + "_mean"]
        assert (z["ssim"] <= 1).all() and (z["ssim"] > -1).all()
    assert "ssim_mean" not in plain["total"]
    lines = open(os.path.join(summary["dir"], "summary.txt")).read().splitlines()
    assert lines[:3] == open(os.path.join(plain["dir"], "summary.txt")).read().splitlines() and lines[3].startswith("# group ssim_mean")
    ops.reset_variables()


def test_ae_evaluate_with_ssim(tmp_path):
    import test_gpu_field_metrics as fm
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_ae_dataset, preprocess
    from deep_fluids_amd.trainer import AETrainer, default_config
    ops.reset_variables()
    spatial = (8, 16, 8)
    root = str(tmp_path / "data")
    n = write_synthetic_ae_dataset(root, spatial, num_scenes=2, num_frames=3, seed=3)
    bm = BatchManager(fm._data_cfg(root, spatial, "ae"), device=None)
    cfg = default_config(is_3d=True, res_x=8, res_y=16, res_z=8, filters=8, batch_size=2, num_samples=n, z_num=6, p_num=2, arch="ae",
                         model_dir=str(tmp_path / "model"), test_batch_size=4)
    tr = AETrainer(cfg)
    summary = tr.evaluate_(bm, ssim=True)                                # batches of 4 and 2 frames over scenes of 3
    truth = np.stack([preprocess(p, bm.data_type, bm.x_range, bm.y_range)[0] for p in bm.paths])
    by_hand = np.concatenate([host(ops.field_ssim(tr.reconstruct(x).contiguous(), x)) for x in (dev(truth[:4]), dev(truth[4:]))])
    ms = np.concatenate([host(ops.field_ssim(tr.reconstruct(x).contiguous(), x, multiscale=True)) for x in (dev(truth[:4]), dev(truth[4:]))])
    for s in range(2):
        with np.load(os.path.join(summary["dir"], "%d.npz" % s)) as z:
            np.testing.assert_array_equal(z["ssim"].view(np.int64), by_hand[3 * s:3 * s + 3].view(np.int64))
            np.testing.assert_array_equal(z["ms_ssim"].view(np.int64), ms[3 * s:3 * s + 3].view(np.int64))
    assert summary["total"]["ssim_min"] == float(by_hand.min())
    ops.reset_variables()


def test_refusals():
    from deep_fluids_amd import _lib, ops
    a = torch.zeros((2, 12, 17, 3), device="cuda")
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.ssim(torch.zeros((2, 12, 17, 3), device="cuda", requires_grad=True), a)
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.ms_ssim(a, torch.zeros((2, 12, 17, 3), device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="filter_size"):
        ops.ssim(a, a, filter_size=0)
    with pytest.raises(ValueError, match="must be float32"):
        ops.ssim(a, a.double())
    with pytest.raises(ValueError, match="disagree in shape"):
        ops.ssim(a, a[:, :, :16].contiguous())
    with pytest.raises(ValueError, match="must be contiguous"):
        ops.field_ssim(a.transpose(1, 2), a.transpose(1, 2))
    with pytest.raises(_lib.DeepFluidsHipError, match="no CPU path"):
        ops.ssim(a.cpu(), a.cpu())
    with pytest.raises(_lib.DeepFluidsHipError, match="no CPU path"):
        ops.ms_ssim(a, a.cpu())
    with pytest.raises(ValueError, match="another call"):
        ops.field_ssim(a, a, workspace=ops.ssim_workspace(a, multiscale=True))
