"""The fused field metrics without a GPU: the properties of their NumPy restatement (tests/field_metrics_ref.py, the definition of
include/deepfluids_hip_metrics.h), every refusal of ``ops.field_metrics`` on CPU tensors, the size query and the argument errors of the
C ABI (all answered on the host), and the files ``evaluate_`` writes, from rows of the twin.  ``evaluate_`` itself runs
``field_metrics`` and is tested on the GPU (tests/test_gpu_field_metrics.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_metrics_ref as ref  # noqa: E402

import df_oracle as orc  # noqa: E402
from deep_fluids_amd import _lib, ops, trainer  # noqa: E402

F32, F64 = np.float32, np.float64
SMALL = [(2, 5, 7), (2, 4, 5, 6)]


@pytest.mark.parametrize("shape", SMALL, ids=str)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_equal_fields_have_no_error_and_keep_their_own_stencils(shape, dtype):
    g, x = ref.inputs(shape)
    D = len(shape) - 1
    r = ref.metrics(x, x, None, dtype)
    n = int(np.prod(shape[1:]))
    assert (r["count"] == n).all() and (r["div_count"] == int(np.prod([s - 1 for s in shape[1:]]))).all()
    for k in ("sum_abs", "sum_sq", "max_abs", "sum_abs_jac"):
        assert (r[k] == 0).all(), k
    assert (r["argmax"] == 0).all()                                      # every cell ties at 0: the lowest index
    # div and the sums of x are those of the pair (g, x): they do not depend on g
    q = ref.metrics(g, x, None, dtype)
    for k in ("sum_abs_x", "sum_sq_x", "sum_abs_div_x", "max_abs_div_x"):
        np.testing.assert_array_equal(r[k], q[k])
    np.testing.assert_array_equal(r["sum_abs_div_g"], r["sum_abs_div_x"])
    # ... and are the oracle's stencils summed: fp64 against a plain fp64 sum
    if dtype is F64:
        div = (orc.divergence3 if D == 3 else orc.divergence)(x.astype(F64))
        np.testing.assert_allclose(r["sum_abs_div_x"], np.abs(div).reshape(shape[0], -1).sum(1), rtol=1e-13)
        np.testing.assert_allclose(r["max_abs_div_x"], np.abs(div).reshape(shape[0], -1).max(1), rtol=0)
        jg = (orc.jacobian3 if D == 3 else orc.jacobian)(g.astype(F64))[0]
        jx = (orc.jacobian3 if D == 3 else orc.jacobian)(x.astype(F64))[0]
        np.testing.assert_allclose(q["sum_abs_jac"], np.abs(jg - jx).reshape(shape[0], -1).sum(1), rtol=1e-13)
        np.testing.assert_allclose(q["sum_abs"], np.abs(g.astype(F64) - x).reshape(shape[0], -1).sum(1), rtol=1e-13)
        d = ref.derived(q, D)
        np.testing.assert_allclose(d["l1"], np.abs(g.astype(F64) - x).reshape(shape[0], -1).mean(1), rtol=1e-13)
        np.testing.assert_allclose(d["jacobian_l1"], np.abs(jg - jx).reshape(shape[0], -1).mean(1), rtol=1e-13)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("dim", [2, 3])
def test_a_curl_field_is_divergence_free_to_rounding(dim, dtype):
    """u = curl(psi) with the stencils' own differences: D_x D_y = D_y D_x holds for the replicated differences too, so div u is 0 in
    exact arithmetic.  In ``dtype`` each of the <= 6 values a divergence reads carries <= 3 roundings of at most eps/2 * 4 max|psi|, and
    the divergence's own 3 differences and 2 sums <= 5 of at most eps/2 * 8 max|psi|: 56 eps max|psi| in all, asserted as 64."""
    rng = np.random.RandomState(5)
    shape = (2, 6, 7) if dim == 2 else (2, 4, 5, 6)
    psi = rng.uniform(-1, 1, shape + (1 if dim == 2 else 3,)).astype(dtype)
    u = orc.curl(psi) if dim == 2 else orc.curl3(psi)
    assert u.dtype == dtype
    r = ref.metrics(u, np.zeros_like(u), None, dtype)
    bound = 64 * np.finfo(dtype).eps * float(np.abs(psi).max())
    print("max |div curl psi| %.3e (bound %.3e)" % (r["max_abs_div_g"].max(), bound))
    assert (r["max_abs_div_g"] <= bound).all()
    assert (r["max_abs_div_x"] == 0).all() and (r["sum_abs_x"] == 0).all()
    d = ref.derived(r, dim)
    assert np.isnan(d["rel_l1"]).all() and np.isnan(d["rel_l2"]).all()     # sum |x| == 0: nan, not an exception
    assert (d["div_l1_g"] <= bound).all()


def test_the_mask_excludes_what_it_should():
    shape = (2, 4, 5, 6)
    g, x = ref.inputs(shape)
    mask = ref.case_mask(shape, "per_entry")
    r = ref.metrics(g, x, mask, F64)
    # the same numbers from the cells picked by hand
    d = np.abs(g.astype(F64) - x)
    jd = np.abs(orc.jacobian3(g.astype(F64))[0] - orc.jacobian3(x.astype(F64))[0]).sum(-1)
    dv = np.abs(orc.divergence3(g.astype(F64))[..., 0])
    for b in range(2):
        m = mask[b] != 0
        assert r["count"][b] == m.sum() and r["div_count"][b] == m[:-1, :-1, :-1].sum()
        np.testing.assert_allclose(r["sum_abs"][b], d[b][m].sum(), rtol=1e-13)
        np.testing.assert_allclose(r["sum_abs_jac"][b], jd[b][m].sum(), rtol=1e-13)
        np.testing.assert_allclose(r["sum_abs_div_g"][b], dv[b][m[:-1, :-1, :-1]].sum(), rtol=1e-13)
        assert r["max_abs"][b] == d[b][m].max()
        assert m.ravel()[r["argmax"][b]] and d[b].max(-1).ravel()[r["argmax"][b]] == r["max_abs"][b]
    # a shared mask is the per-entry mask repeated; one cell; no cell
    sh = ref.case_mask(shape, "shared")
    a, b = ref.metrics(g, x, sh, F32), ref.metrics(g, x, np.broadcast_to(sh, shape), F32)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    one = ref.metrics(g, x, ref.case_mask(shape, "single"), F32)
    assert (one["count"] == 1).all() and (one["div_count"] == 1).all()
    cell = np.ravel_multi_index(tuple(n // 2 for n in shape[1:]), shape[1:])
    assert (one["argmax"] == cell).all()
    np.testing.assert_array_equal(one["max_abs"], np.abs(g - x).reshape(2, -1, 3)[:, cell].max(-1))
    none = ref.metrics(g, x, np.zeros(shape[1:], np.uint8), F32)
    assert (none["count"] == 0).all() and (none["argmax"] == -1).all()
    assert all((none[k] == 0).all() for k in ref.SUMS + ref.MAXES)
    dn = ref.derived(none, 3)
    assert all(np.isnan(dn[k]).all() for k in dn)                         # nothing counted: zeros and nan means


def test_the_lowest_index_wins_a_tie():
    shape = (1, 3, 40, 40)                                               # 4800 cells: five workgroups
    x = np.zeros(shape + (3,), F32)
    g = x.copy()
    cells = [4444, 1500, 77, 1501]                                       # in three workgroups, two of them neighbours in one
    for i, c in enumerate(cells):
        g.reshape(-1, 3)[c, i % 3] = -0.5 if i % 2 else 0.5              # |.| ties across components and signs
    r = ref.metrics(g, x, None, F32)
    assert r["argmax"][0] == 77 and r["max_abs"][0] == F32(0.5)
    m = np.ones(shape[1:], np.uint8)
    m.reshape(-1)[77] = 0
    assert ref.metrics(g, x, m, F32)["argmax"][0] == 1500                # the lowest COUNTED cell


def test_refusals_of_field_metrics_without_a_device():
    g2, g3 = torch.zeros((2, 4, 6, 2)), torch.zeros((2, 4, 5, 6, 3))
    with pytest.raises(ValueError, match=r"\[B,Y,X,2\] or \[B,Z,Y,X,3\]"):
        ops.field_metrics(torch.zeros((2, 4, 6, 3)), torch.zeros((2, 4, 6, 3)))
    with pytest.raises(ValueError, match=r"\[B,Y,X,2\] or \[B,Z,Y,X,3\]"):
        ops.field_metrics(torch.zeros((4, 6, 2)), torch.zeros((4, 6, 2)))
    with pytest.raises(ValueError, match="disagree in shape"):
        ops.field_metrics(g2, torch.zeros((2, 4, 5, 2)))
    with pytest.raises(ValueError, match="disagree in shape"):
        ops.field_metrics(g3, g2)
    with pytest.raises(ValueError, match="x must be float32"):
        ops.field_metrics(g2, g2.double())
    with pytest.raises(ValueError, match="g must be float32"):
        ops.field_metrics(g3.half(), g3.half())
    with pytest.raises(ValueError, match="g must be contiguous"):
        ops.field_metrics(torch.zeros((2, 4, 12, 2))[:, :, ::2], g2)
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.field_metrics(g3, torch.zeros((2, 4, 5, 3, 6)).transpose(-1, -2))
    with pytest.raises(ValueError, match=">= 2"):
        ops.field_metrics(torch.zeros((1, 1, 6, 2)), torch.zeros((1, 1, 6, 2)))
    with pytest.raises(ValueError, match=">= 2"):
        ops.field_metrics(torch.zeros((0, 4, 6, 2)), torch.zeros((0, 4, 6, 2)))
    with pytest.raises(ValueError, match="int32 cell index"):
        ops.field_metrics(torch.empty((1, 2048, 1024, 1024, 3), device="meta"), torch.empty((1, 2048, 1024, 1024, 3), device="meta"))
    with pytest.raises(ValueError, match="mask must be a uint8"):
        ops.field_metrics(g2, g2, mask=torch.zeros((4, 6)))
    with pytest.raises(ValueError, match="mask must be a uint8"):
        ops.field_metrics(g2, g2, mask=np.zeros((4, 6), np.uint8))
    with pytest.raises(ValueError, match=r"mask must be \[\(Z,\)Y,X\]"):
        ops.field_metrics(g2, g2, mask=torch.zeros((6, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"mask must be \[\(Z,\)Y,X\]"):
        ops.field_metrics(g3, g3, mask=torch.zeros((1, 4, 5, 6), dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask must be contiguous"):
        ops.field_metrics(g2, g2, mask=torch.zeros((4, 12), dtype=torch.uint8)[:, ::2])
    need = _lib.query("df_field_metrics_workspace_bytes", 3, 2, 4, 5, 6)
    assert need == 2 * 80
    with pytest.raises(ValueError, match=r"workspace must be a contiguous tensor of >= 160 bytes"):
        ops.field_metrics(g3, g3, workspace=torch.zeros((need // 8 - 1,), dtype=torch.float64))
    with pytest.raises(ValueError, match="workspace must be a contiguous tensor"):
        ops.field_metrics(g3, g3, workspace=torch.zeros((need,), dtype=torch.float64)[::2])
    assert "field_metrics" in ops.__all__
    if not torch.cuda.is_available():                                    # everything above was refused before anything asked for a device
        with pytest.raises(_lib.DeepFluidsHipError, match="no CPU path"):
            ops.field_metrics(g3, g3, mask=torch.ones((4, 5, 6), dtype=torch.uint8), workspace=torch.zeros((need // 8,), dtype=torch.float64))


def test_workspace_query_answers_on_the_host():
    q = _lib.metrics_lib().df_field_metrics_workspace_bytes
    assert q(3, 16, 64, 96, 64) == 16 * 384 * 80 and q(2, 64, 1, 128, 96) == 64 * 12 * 80
    assert q(2, 1, 1, 2, 2) == 80 and q(3, 1, 2, 2, 2) == 80 and q(3, 1, 1, 1025, 1) == -1
    assert q(2, 3, 1, 17, 130) == 3 * 3 * 80
    for bad in ((1, 1, 1, 4, 4), (4, 1, 4, 4, 4),                         # dim
                (3, 0, 4, 4, 4), (3, 1, -1, 4, 4), (2, 1, 1, 0, 4),       # non-positive
                (3, 1, 1, 4, 4), (3, 1, 4, 1, 4), (3, 1, 4, 4, 1), (2, 1, 1, 1, 4), (2, 1, 1, 4, 1),      # below the stencils' extents
                (2, 1, 2, 4, 4),                                          # dim = 2 takes Z = 1
                (3, 1, 2048, 1024, 1024), (2, 1, 1, 1 << 16, 1 << 15), (3, 1, 2, 2, 1 << 31),             # N >= 2^31
                (2, 1 << 31, 1, 2, 2), (3, 1 << 23, 64, 96, 64)):         # more workgroups (2^23 x 384) than a launch holds
        assert q(*bad) == -1, bad
    assert q(2, 1, 1, 1 << 15, (1 << 15) + 0) == (1 << 20) * 80          # N = 2^30 still fits


def test_cabi_argument_errors_launch_nothing():
    h = _lib.metrics_lib()
    err = _lib.lib().df_last_error
    buf = ctypes.create_string_buffer(1 << 14)
    a = (ctypes.addressof(buf) + 15) & ~15
    g, x, out, ws = a, a + 4096, a + 8192, a + 8192 + 256                 # 2 x 4 x 5 x 6 x 3 floats = 2880 bytes each
    ok3 = (2, 4, 5, 6, None)
    assert h.df_field_metrics3d(None, x, None, 0, out, ws, 160, *ok3) == -1 and b"null field" in err()
    assert h.df_field_metrics3d(g, None, None, 0, out, ws, 160, *ok3) == -1 and b"null field" in err()
    assert h.df_field_metrics3d(g, x, None, 0, None, ws, 160, *ok3) == -1 and b"null out" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, None, 160, *ok3) == -1 and b"null workspace" in err()
    assert h.df_field_metrics3d(g, x, None, 2, out, ws, 160, *ok3) == -1 and b"mask_per_entry" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, ws, 160, 0, 4, 5, 6, None) == -1 and b"non-positive" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, ws, 160, 2, 1, 5, 6, None) == -2 and b">= 2" in err()
    assert h.df_field_metrics2d(g, x, None, 0, out, ws, 160, 2, 5, 1, None) == -2 and b">= 2" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, ws, 1 << 40, 1, 2048, 1024, 1024, None) == -2 and b"int32 cell index" in err()
    assert h.df_field_metrics3d(g + 2, x, None, 0, out, ws, 160, *ok3) == -3
    assert h.df_field_metrics3d(g, x, None, 0, out + 2, ws, 160, *ok3) == -3
    assert h.df_field_metrics3d(g, x, None, 0, out, ws + 4, 160, *ok3) == -3 and b"8-byte" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, ws, 159, *ok3) == -4 and b"160 needed" in err()
    assert h.df_field_metrics2d(g, x, None, 0, out, ws, 79, 1, 4, 6, None) == -4
    # overlaps: out inside an input, out == ws, ws inside x, out inside the mask (per entry: 240 bytes; shared: 120)
    assert h.df_field_metrics3d(g, x, None, 0, g + 2880 - 4, ws, 160, *ok3) == -1 and b"out overlaps an input" in err()
    assert h.df_field_metrics3d(g, x, None, 0, x, ws, 160, *ok3) == -1 and b"out overlaps an input" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, out + 120, 160, *ok3) == -1 and b"out overlaps the workspace" in err()
    assert h.df_field_metrics3d(g, x, None, 0, out, x + 8, 160, *ok3) == -1 and b"workspace overlaps an input" in err()
    mask = out + 128 - 200
    assert h.df_field_metrics3d(g, x, mask, 1, out, ws, 160, *ok3) == -1 and b"out overlaps an input" in err()
    assert h.df_field_metrics3d(g, x, mask, 0, out, ws, 160, 2, 4, 5, 0, None) == -1      # (still refused: a bad extent comes first)


def test_evaluate_files_from_rows_of_the_twin(tmp_path):
    """the layout ``Trainer.evaluate_`` writes (its ``_eval_write``), fed with host rows: two groups of 3 and 2 frames"""
    shape = (5, 4, 5, 6)
    g, x = ref.inputs(shape)
    r = ref.metrics(g, x, None, F32)
    raw = torch.from_numpy(ref.raw_words(r))
    fm = ops.FieldMetrics(raw, 3)
    d = ref.derived(r, 3)
    for k in ops.FieldMetrics.DERIVED:                                    # the derived properties are the restatement's
        np.testing.assert_allclose(getattr(fm, k).numpy(), d[k], rtol=1e-15)
    for k in ops.FieldMetrics.QUANTITIES:
        np.testing.assert_array_equal(getattr(fm, k).numpy(), r[k])
    groups = [("0_1", ops.FieldMetrics(raw[:3], 3)), ("2_0", ops.FieldMetrics(raw[3:], 3))]
    s = trainer._eval_write(str(tmp_path), groups, 2.5)
    assert s["dir"] == str(tmp_path / "eval") and sorted(os.listdir(s["dir"])) == ["0_1.npz", "2_0.npz", "summary.txt"]
    with np.load(os.path.join(s["dir"], "2_0.npz")) as z:
        keys = set(z.files)
        want = set(ops.FieldMetrics.QUANTITIES + ops.FieldMetrics.DERIVED) | {k + "_denorm" for k in ops.FieldMetrics.LINEAR} | {"x_range"}
        assert keys == want
        np.testing.assert_array_equal(z["sum_abs"], r["sum_abs"][3:])
        np.testing.assert_allclose(z["l1_denorm"], d["l1"][3:] * 2.5, rtol=1e-15)
        assert z["count"].dtype == np.int32 and z["l1"].dtype == np.float64 and z["l1"].shape == (2,)
    assert s["groups"]["0_1"]["frames"] == 3 and s["groups"]["2_0"]["worst_frame"] == int(np.argmax(d["l1"][3:]))
    assert s["total"]["frames"] == 5
    np.testing.assert_allclose(s["total"]["l1_mean"], d["l1"].mean(), rtol=1e-15)
    np.testing.assert_allclose(s["total"]["rel_l2_max"], d["rel_l2"].max(), rtol=1e-15)
    w = int(np.argmax(d["l1"]))
    assert s["total"]["worst_frame"] == ("0_1:%d" % w if w < 3 else "2_0:%d" % (w - 3))
    lines = open(os.path.join(s["dir"], "summary.txt")).read().splitlines()
    assert lines[0].startswith("#") and [ln.split()[0] for ln in lines[1:]] == ["0_1", "2_0", "total"]
    assert len(lines[1].split()) == 2 + 2 * len(trainer.EVAL_SUMMARY) + 1
    np.testing.assert_allclose(float(lines[3].split()[2]), d["l1"].mean(), rtol=1e-8)
    without = trainer._eval_write(str(tmp_path / "n"), groups, None)       # denorm=False: normalised arrays only
    with np.load(os.path.join(without["dir"], "0_1.npz")) as z:
        assert set(z.files) == set(ops.FieldMetrics.QUANTITIES + ops.FieldMetrics.DERIVED)
