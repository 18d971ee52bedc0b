"""-m gpu: the fused field metrics (csrc/metrics.hip, include/deepfluids_hip_metrics.h) against their NumPy restatement
tests/field_metrics_ref.py: counts, arg-max and maxima exact, every sum bit for bit the fp32 twin (the header fixes the order), and
against the fp64 truth within 4 x the twin's own deviation from it, measured in the same test (the convention of
test_gpu_liquid_mesh.py; no constant is written down).  ``ref.SHAPES`` names the boundary of the kernels each shape crosses.  Then the
masks, the independence of an entry from its batch, the agreement with the existing stencil ops, the C ABI's refusals on device
buffers, and ``Trainer.evaluate_`` / ``AETrainer.evaluate_`` on tiny synthetic data sets."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_metrics_ref as ref  # noqa: E402
from gpu_util import dev, host  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = np.float64


def _u8(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(shape, kind=None, **kw):
    from deep_fluids_amd import ops
    g, x = ref.inputs(shape)
    mask = None if kind is None else ref.case_mask(shape, kind)
    return ops.field_metrics(dev(g), dev(x), mask=_u8(mask), **kw)


def _check(fm, twin, truth, what):
    """exact against the twin, and 4 x the twin's own deviation against fp64"""
    raw = host(fm.raw)
    want = ref.raw_words(twin)
    for name in ref.INTS + ref.MAXES + ref.SUMS:
        w = ref.WORD[name]
        assert (raw[:, w] == want[:, w]).all(), "%s %s: got %r, twin %r" % (what, name, host(getattr(fm, name)), twin[name])
    np.testing.assert_array_equal(raw, want)                              # the reserved words are 0 as well
    for name in ref.SUMS:
        got = host(getattr(fm, name)).astype(F64)
        e_gpu, e_twin = np.abs(got - truth[name]), np.abs(twin[name].astype(F64) - truth[name])
        print("%s %s: |gpu - fp64| %s, |twin - fp64| %s" % (what, name, e_gpu, e_twin))
        assert (e_gpu <= 4 * e_twin).all(), (what, name)
    for name in ref.INTS:
        np.testing.assert_array_equal(twin[name], truth[name])             # what is counted does not depend on the precision


@pytest.mark.parametrize("shape", [s for s, _ in ref.SHAPES], ids=str)
def test_every_quantity_is_the_twin_bit_for_bit(shape):
    twin, truth = ref.reference(shape)
    fm = _run(shape)
    assert fm.batch == shape[0] and fm.dim == len(shape) - 1
    _check(fm, twin, truth, str(shape))
    d = ref.derived(twin, fm.dim)
    for k in fm.DERIVED:
        np.testing.assert_allclose(host(getattr(fm, k)), d[k], rtol=1e-15, err_msg=k)


@pytest.mark.parametrize("kind", ["shared", "per_entry", "one_empty", "single"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (3, 17, 130)], ids=str)
def test_masks(shape, kind):
    twin, truth = ref.reference(shape, kind)
    fm = _run(shape, kind)
    _check(fm, twin, truth, "%s %s" % (shape, kind))
    if kind == "one_empty":                                               # nothing counted: zeros, argmax -1, nan means
        assert int(fm.count[0]) == 0 and int(fm.argmax[0]) == -1 and not host(fm.raw)[0, 3:].any()
        assert all(bool(torch.isnan(getattr(fm, k)[0])) for k in fm.DERIVED)
        assert not any(bool(torch.isnan(getattr(fm, k)[1:]).any()) for k in fm.DERIVED)
    if kind == "single":
        assert (host(fm.count) == 1).all()


def test_a_tie_goes_to_the_lowest_counted_cell_across_workgroups():
    from deep_fluids_amd import ops
    shape = (1, 3, 40, 40)                                               # five workgroups
    x = np.zeros(shape + (3,), np.float32)
    g = x.copy()
    for i, c in enumerate([4444, 1500, 77, 1501]):
        g.reshape(-1, 3)[c, i % 3] = -0.5 if i % 2 else 0.5
    fm = ops.field_metrics(dev(g), dev(x))
    assert int(fm.argmax[0]) == 77 and float(fm.max_abs[0]) == 0.5
    m = np.ones(shape[1:], np.uint8)
    m.reshape(-1)[77] = 0
    fm = ops.field_metrics(dev(g), dev(x), mask=_u8(m))
    assert int(fm.argmax[0]) == 1500
    np.testing.assert_array_equal(host(fm.raw), ref.raw_words(ref.metrics(g, x, m)))
    assert bool(torch.isnan(fm.rel_l1[0])) and bool(torch.isnan(fm.rel_l2[0]))      # sum |x| == 0


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (3, 17, 130)], ids=str)
def test_an_entry_does_not_depend_on_its_batch_and_runs_repeat(shape):
    from deep_fluids_amd import ops
    g, x = ref.inputs(shape)
    mask = ref.case_mask(shape, "per_entry")
    gd, xd, md = dev(g), dev(x), _u8(mask)
    whole = host(ops.field_metrics(gd, xd, mask=md).raw)
    for e in range(shape[0]):                                            # entry e alone, B = 1
        one = host(ops.field_metrics(gd[e:e + 1].contiguous(), xd[e:e + 1].contiguous(), mask=md[e:e + 1].contiguous()).raw)
        np.testing.assert_array_equal(one[0], whole[e])
    np.testing.assert_array_equal(host(ops.field_metrics(gd, xd, mask=md).raw), whole)           # twice: the same bits
    ws = ops.field_metrics_workspace(gd)
    assert ws.numel() * ws.element_size() == ops.query("df_field_metrics_workspace_bytes", len(shape) - 1, shape[0],
                                                       *((1,) * (4 - len(shape)) + shape[1:]))
    a = host(ops.field_metrics(gd, xd, mask=md, workspace=ws).raw)
    ws.view(torch.int64).fill_(-1)                                       # whatever an earlier call left is not read
    b = host(ops.field_metrics(gd, xd, mask=md, workspace=ws).raw)
    np.testing.assert_array_equal(a, whole)
    np.testing.assert_array_equal(b, whole)
    with pytest.raises(ValueError, match="workspace must be a contiguous tensor"):
        ops.field_metrics(gd, xd, workspace=ws[:-1])


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (3, 17, 130)], ids=str)
def test_the_jacobian_and_divergence_are_those_of_the_ops(shape):
    """sum |J(g) - J(x)| and sum |div g| against the existing ops: ``jacobian(3)`` / ``divergence(3)`` on the GPU, |.| and the differences
    by torch in fp32 (element for element what the fused kernel forms), summed by torch in fp64 so that no second summation order
    enters; the fused sums must agree within 4 x the twin's deviation from the fp64 truth."""
    from deep_fluids_amd import ops
    g, x = ref.inputs(shape)
    gd, xd = dev(g), dev(x)
    is_3d = len(shape) == 4
    fm = ops.field_metrics(gd, xd)
    twin, truth = ref.reference(shape)
    jac, div = (ops.jacobian3, ops.divergence3) if is_3d else (ops.jacobian, ops.divergence)
    jsum = host((jac(gd)[0] - jac(xd)[0]).abs().reshape(shape[0], -1).double().sum(1))
    dsum = host(div(gd).abs().reshape(shape[0], -1).double().sum(1))
    dmax = host(div(gd).abs().reshape(shape[0], -1).max(1).values)
    np.testing.assert_array_equal(host(fm.max_abs_div_g), dmax)           # the same values, so the same maximum
    for name, composed in (("sum_abs_jac", jsum), ("sum_abs_div_g", dsum)):
        e = np.abs(host(getattr(fm, name)).astype(F64) - composed)
        e_twin = np.abs(twin[name].astype(F64) - truth[name])
        print("%s %s: |fused - ops| %s, |twin - fp64| %s" % (shape, name, e, e_twin))
        assert (e <= 4 * e_twin).all(), name


def test_cabi_refusals_on_device_buffers_launch_nothing():
    from deep_fluids_amd import _lib
    h = _lib.metrics_lib()
    shape = (2, 4, 5, 6)
    g, x = (dev(a) for a in ref.inputs(shape))
    out = torch.full((2, _lib.DF_FM_WORDS), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((2 * 80 // 8,), -7, dtype=torch.int64, device="cuda")
    args = (2, 4, 5, 6, None)
    assert h.df_field_metrics3d(None, x.data_ptr(), None, 0, out.data_ptr(), ws.data_ptr(), 160, *args) == _lib.DF_EINVAL
    assert h.df_field_metrics3d(g.data_ptr(), x.data_ptr(), None, 0, g.data_ptr() + 64, ws.data_ptr(), 160, *args) == _lib.DF_EINVAL
    assert b"out overlaps an input" in _lib.lib().df_last_error()
    assert h.df_field_metrics3d(g.data_ptr(), x.data_ptr(), None, 0, out.data_ptr(), ws.data_ptr(), 159, *args) == _lib.DF_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((ws == -7).all())
    np.testing.assert_array_equal(host(g), ref.inputs(shape)[0])
    assert h.df_field_metrics3d(g.data_ptr(), x.data_ptr(), None, 0, out.data_ptr(), ws.data_ptr(), 160, *args) == 0
    np.testing.assert_array_equal(host(out), ref.raw_words(ref.reference(shape)[0]))


# ---- evaluate_ -------------------------------------------------------------------------------------------------------------------------
def _data_cfg(root, spatial, arch):
    is_3d = len(spatial) == 3
    return SimpleNamespace(random_seed=1, data_path=root, is_3d=is_3d, arch=arch, data_type="velocity", batch_size=2, res_x=spatial[-1],
                           res_y=spatial[-2], res_z=spatial[0] if is_3d else 1, num_worker=1)


def _check_eval_files(summary, names, per_frame, x_range):
    """the files of one evaluate_ against ``per_frame``: name -> host FieldMetrics computed by hand"""
    from deep_fluids_amd import ops
    from deep_fluids_amd.trainer import EVAL_SUMMARY
    FM = ops.FieldMetrics
    assert sorted(os.listdir(summary["dir"])) == sorted([n + ".npz" for n in names] + ["summary.txt"])
    every = {q: [] for q in EVAL_SUMMARY}
    for n in names:
        with np.load(os.path.join(summary["dir"], n + ".npz")) as z:
            assert set(z.files) == set(FM.QUANTITIES + FM.DERIVED) | {k + "_denorm" for k in FM.LINEAR} | {"x_range"}
            for k in FM.QUANTITIES + FM.DERIVED:
                np.testing.assert_array_equal(z[k], getattr(per_frame[n], k).numpy(), err_msg="%s %s" % (n, k))
            for k in FM.LINEAR:
                np.testing.assert_array_equal(z[k + "_denorm"], z[k] * float(x_range))
            st = summary["groups"][n]
            assert st["frames"] == per_frame[n].batch and st["worst_frame"] == int(np.argmax(z["l1"]))
            for q in EVAL_SUMMARY:
                assert st[q + "_mean"] == float(np.mean(z[q])) and st[q + "_max"] == float(np.max(z[q]))
                every[q].append(z[q])
    for q in EVAL_SUMMARY:                                                # the totals follow from the per-frame arrays
        v = np.concatenate(every[q])
        assert summary["total"][q + "_mean"] == float(np.mean(v)) and summary["total"][q + "_max"] == float(np.max(v))
    assert summary["total"]["frames"] == sum(per_frame[n].batch for n in names)
    lines = open(os.path.join(summary["dir"], "summary.txt")).read().splitlines()
    assert [ln.split()[0] for ln in lines[1:]] == list(names) + ["total"]


@pytest.mark.parametrize("spatial,use_curl", [((16, 16), True), ((8, 16, 8), False)], ids=["2d", "3d-nocurl"])
def test_trainer_evaluate(tmp_path, spatial, use_curl):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset, preprocess
    from deep_fluids_amd.trainer import Trainer, default_config
    ops.reset_variables()
    is_3d = len(spatial) == 3
    root = str(tmp_path / "data")
    write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=4, seed=5)
    bm = BatchManager(_data_cfg(root, spatial, "de"), device=None)
    cfg = default_config(is_3d=is_3d, res_x=spatial[-1], res_y=spatial[-2], res_z=spatial[0] if is_3d else 1, filters=8, batch_size=2,
                         num_samples=24, use_curl=use_curl, model_dir=str(tmp_path / "model"), test_batch_size=2)
    tr = Trainer(cfg)                                                    # freshly initialised
    mask = np.ones(spatial, np.uint8)
    mask[..., 0] = 0
    pairs = [(2, 1), (0, 0)]
    summary = tr.evaluate_(bm, pairs=pairs, mask=mask)
    assert summary["dir"] == os.path.join(cfg.model_dir, "eval")
    per_frame = {}
    for p1, p2 in pairs:                                                 # by hand: generate and field_metrics on the loaded truth
        z_c, _, _ = tr._sweep_codes(bm, p1, p2, 4, "test")
        truth = np.stack([preprocess(p, bm.data_type, bm.x_range, bm.y_range)[0] for p in bm.list_from_p([(p1, p2, t) for t in range(4)])])
        parts = [ops.field_metrics(tr.generate(dev(z_c[i:i + 2])).contiguous(), dev(truth[i:i + 2]), mask=_u8(mask)) for i in (0, 2)]
        per_frame["%d_%d" % (p1, p2)] = ops.FieldMetrics.cat(parts).cpu()      # in the batches of test_batch_size evaluate_ runs
    _check_eval_files(summary, ["2_1", "0_0"], per_frame, bm.x_range)
    if not use_curl:                                                     # what the question was: how far from divergence free
        assert summary["total"]["div_l1_g_mean"] > 0
    full = tr.evaluate_(bm, model_dir=str(tmp_path / "all"), denorm=False)      # the default: every pair of the set
    assert sorted(full["groups"]) == sorted("%d_%d" % (i, j) for i in range(3) for j in range(2)) and full["total"]["frames"] == 24
    with np.load(os.path.join(full["dir"], "1_1.npz")) as z:
        assert "l1_denorm" not in z.files and (z["count"] == int(np.prod(spatial))).all()
    with pytest.raises(ValueError, match="not a parameter index"):
        tr.evaluate_(bm, pairs=[(3, 0)])
    ops.reset_variables()


@pytest.mark.parametrize("spatial", [(16, 16), (8, 16, 8)], ids=["2d", "3d"])
def test_ae_trainer_evaluate(tmp_path, spatial):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_ae_dataset, preprocess
    from deep_fluids_amd.trainer import AETrainer, default_config
    ops.reset_variables()
    is_3d = len(spatial) == 3
    root = str(tmp_path / "data")
    n = write_synthetic_ae_dataset(root, spatial, num_scenes=2, num_frames=3, seed=3)
    bm = BatchManager(_data_cfg(root, spatial, "ae"), device=None)
    cfg = default_config(is_3d=is_3d, res_x=spatial[-1], res_y=spatial[-2], res_z=spatial[0] if is_3d else 1, filters=8, batch_size=2,
                         num_samples=n, z_num=6, p_num=2 if is_3d else 1, arch="ae", model_dir=str(tmp_path / "model"), test_batch_size=4)
    tr = AETrainer(cfg)
    summary = tr.evaluate_(bm)                                           # batches of 4 and 2 frames over scenes of 3
    truth = np.stack([preprocess(p, bm.data_type, bm.x_range, bm.y_range)[0] for p in bm.paths])
    by_hand = ops.FieldMetrics.cat([ops.field_metrics(tr.reconstruct(x).contiguous(), x) for x in (dev(truth[:4]), dev(truth[4:]))]).cpu()
    per_frame = {str(s): ops.FieldMetrics(by_hand.raw[3 * s:3 * s + 3], by_hand.dim) for s in range(2)}
    _check_eval_files(summary, ["0", "1"], per_frame, bm.x_range)
    ops.reset_variables()
