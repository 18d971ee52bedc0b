"""SSIM / MS-SSIM without a GPU: the NumPy restatement (tests/ssim_ref.py, the definition of include/deepfluids_hip_ssim.h) against
what the reference's own functions returned (tests/golden/ssim.npz), the fp32 twin's distance from it, the window and the pooling, the
C ABI (header, exports, binding, the size query, every argument error -- all answered on the host), the refusals of the ``ops`` entry
points, and the files ``evaluate_`` writes with and without the new keyword.  The kernels run in tests/test_gpu_ssim.py.

Measured on the golden (this file prints them): the fp64 restatement deviates from the reference's arrays by at most 2.5e-13 relative
(asserted at 4x: FP64_BOUND).  Only the separable window against the 2-D one differs, a few ulp per filtered plane; the rest is the
cancellation in E[x^2] - mu^2, largest for C = 1 where the map values come closest to zero (ssim_33x45_c1; every C >= 2 case stays
below 4e-15).  The fp32 twin deviates from the golden by at most 4.3e-5 absolute on a map (C = 1, the same cancellation in fp32; below
1e-6 for C >= 2), printed per case: the GPU test's yardstick."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssim_ref as ref  # noqa: E402
import test_field_metrics_host as fmh  # noqa: E402  (the host-side stand-in for evaluate_'s rows)

from deep_fluids_amd import _lib, ops, trainer  # noqa: E402

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim.npz")
FP64_BOUND = 4 * 2.5e-13


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got, F64) - want) / np.abs(want)))


def test_fp64_restatement_reproduces_the_golden_and_the_twin_is_close(golden):
    worst, twin_worst = 0.0, 0.0
    for (H, W), _ in ref.SSIM_SHAPES:
        for c in ref.SSIM_CHANNELS:
            key = "ssim_%dx%d_c%d" % (H, W, c)
            x, g = ref.inputs((H, W), c)
            np.testing.assert_array_equal(ref.checksum(g, x), golden[key + "_check"])      # the seeded inputs are the golden's
            if key + "_in_g" in golden:
                np.testing.assert_array_equal(g, golden[key + "_in_g"])
                np.testing.assert_array_equal(x, golden[key + "_in_x"])
            twin, truth = ref.reference((H, W), c)
            devs = [_rel(truth["mean"], golden[key + "_mean"]), _rel(truth["mean_cs"], golden[key + "_mean_cs"]),
                    _rel(ref.group_mean(truth["sum"], truth["count"], 1)[0], golden[key + "_batch_mean"])]
            tdev = float(np.max(np.abs(twin["mean"].astype(F64) - golden[key + "_mean"])))
            if key + "_ssim_map" in golden:
                devs += [_rel(truth["ssim_map"], golden[key + "_ssim_map"]), _rel(truth["cs_map"], golden[key + "_cs_map"])]
                tdev = max(tdev, float(np.max(np.abs(twin["ssim_map"].astype(F64) - golden[key + "_ssim_map"]))),
                           float(np.max(np.abs(twin["cs_map"].astype(F64) - golden[key + "_cs_map"]))))
            print("%s: fp64 rel %.2e   fp32 twin abs %.2e" % (key, max(devs), tdev))
            worst, twin_worst = max(worst, max(devs)), max(twin_worst, tdev)
            assert (truth["ssim_map"] <= 1 + 1e-12).all()
    for (H, W), c in ref.MS_CASES:
        for noise in ref.MS_NOISE:
            key = "ms_%dx%d_c%d_s%d" % (H, W, c, int(round(noise * 1000)))
            x, g = ref.inputs((H, W), c, noise, ref.MS_N)
            np.testing.assert_array_equal(ref.checksum(g, x), golden[key + "_check"])
            twin, truth = ref.ms_reference((H, W), c, noise)
            # the condition on the inputs: no fractional power of a non-positive number on either side
            assert golden[key + "_mcs"][:-1].min() > 0 and golden[key + "_mssim"][-1] > 0
            assert twin["mcs"][:-1].min() > 0 and twin["mssim"][-1].min() > 0
            devs = [_rel(truth["mssim"][:, 0], golden[key + "_mssim"]), _rel(truth["mcs"][:, 0], golden[key + "_mcs"]),
                    _rel(truth["value"][0], golden[key + "_value"])]
            tdev = abs(float(twin["value"][0]) - float(golden[key + "_value"]))
            print("%s: fp64 rel %.2e   fp32 twin abs %.2e (value %.6f)" % (key, max(devs), tdev, golden[key + "_value"]))
            worst, twin_worst = max(worst, max(devs)), max(twin_worst, tdev)
    print("largest relative deviation of the fp64 restatement: %.3e; of the fp32 twin (absolute): %.3e" % (worst, twin_worst))
    assert worst <= FP64_BOUND
    # fp32 with the cancellation E[x^2] - mu^2 (1e-7 absolute) against v2 of a few 1e-3: not a tolerance of the kernel (that is the twin, bit
    # for bit), only a guard that the twin restates the same thing
    assert twin_worst <= 4 * 4.3e-5
    twin, truth = ref.ms_reference(ref.MS_CASES[0][0], ref.MS_CASES[0][1], ref.MS_NOISE[0], True)
    assert np.isnan(golden["ms_negated_value"]) and np.isnan(truth["value"][0]) and np.isnan(twin["value"][0])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size,sigma", ref.WINDOWS, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_window_is_the_references(golden, size, sigma, channels):
    want = golden["g_s%d_c%d" % (size, channels)]
    assert want.shape == (size, size, channels, channels)
    np.testing.assert_allclose(ref.window(size, sigma, channels), want, rtol=1e-14, atol=0)
    np.testing.assert_allclose(want.sum(), 1.0, rtol=1e-14)           # normalised over ALL entries: each channel pair holds 1 / C^2
    got = ops.fspecial_gauss(size, sigma, channels)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.numpy(), want.astype(F32))
    # the taps the kernel is handed: their outer product over C^2 is the window, to fp32 rounding of each tap
    t = ops._ssim_taps(size, sigma)[0]
    np.testing.assert_array_equal(t, ref.taps(size, sigma, F32))
    np.testing.assert_allclose(np.outer(t, t) / channels ** 2, want[:, :, 0, 0], rtol=3e-7, atol=0)
    if size % 2 == 0:                                                 # the half-cell offset: symmetric, the two middle taps equal
        assert t[size // 2 - 1] == t[size // 2] and np.array_equal(t, t[::-1])


def test_avg_pool_same_on_odd_extents(golden):
    (H, W), c = ref.POOL_CASE
    key = "ms_%dx%d_c%d_s%d" % (H, W, c, int(round(ref.MS_NOISE[0] * 1000)))
    x, g = ref.inputs((H, W), c, ref.MS_NOISE[0], ref.MS_N)
    a64, a32 = g.astype(F64), g
    for k, shape in enumerate([(19, 25), (10, 13), (5, 7), (3, 4)], 1):
        a64, a32 = ref.pool(a64, F64), ref.pool(a32, F32)
        want = golden[key + "_pool%d_g" % k]
        assert want.shape == (ref.MS_N,) + shape + (c,) and a64.shape == want.shape and a32.shape == want.shape and a32.dtype == F32
        np.testing.assert_allclose(a64, want, rtol=1e-14, atol=1e-16)
        np.testing.assert_allclose(a32, want, rtol=0, atol=4 * k * 2.0 ** -24)      # <= 3 roundings of values below 2 per level
    one = np.arange(15, dtype=F64).reshape(1, 3, 5, 1)                  # an edge cell averages what exists
    np.testing.assert_array_equal(ref.pool(one, F64)[0, :, :, 0], [[3, 5, 6.5], [10.5, 12.5, 14]])


def test_header_library_and_binding_agree():
    sigs, consts = _lib.parse_header(open(_lib.SSIM_HEADER_PATH).read())
    assert sigs == _lib.SSIM_SIGNATURES and consts == _lib.SSIM_CONSTANTS
    assert sorted(sigs) == ["df_ssim", "df_ssim_group_mean", "df_ssim_workspace_bytes"]
    assert consts["DF_SSIM_WORDS"] == 8 and consts["DF_SSIM_MAX_SIZE"] == 11 and _lib.DF_SSIM_TILE == 32
    assert os.path.exists(_lib.SSIM_LIB_PATH), "build it first: python -c 'import __graft_entry__ as g; g.build()'"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SSIM_LIB_PATH]).decode()
    exported = sorted(line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("df_"))
    assert exported == sorted(sigs)                                    # both directions: nothing undeclared is exported
    h = _lib.ssim_lib()
    for name, (res, args) in sigs.items():
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert _lib._handle("df_ssim") is h and _lib._handle("df_field_metrics2d") is _lib.metrics_lib()
    assert not set(sigs) & (set(_lib.SIGNATURES) | set(_lib.METRICS_SIGNATURES) | set(_lib.NN_SIGNATURES))
    needed = subprocess.check_output(["readelf", "-d", _lib.SSIM_LIB_PATH]).decode()
    assert "libdeepfluids_hip.so" in needed and "$ORIGIN" in needed
    assert _lib.query("df_version") == 207                             # the main header stays frozen


def test_workspace_query_answers_on_the_host():
    q = _lib.ssim_lib().df_ssim_workspace_bytes
    assert q(64, 128, 96, 11) == 64 * 4 * 3 * 16 and q(1, 11, 11, 11) == 16 and q(3, 64, 70, 11) == 3 * 4 * 16
    assert q(1, 1, 5, 11) == 16 and q(2, 43, 42, 11) == 2 * 2 * 16 and q(1, 5, 5, 100) == 16      # the window shrinks to the image
    for bad in ((0, 8, 8, 11), (1, 0, 8, 11), (1, 8, -1, 11), (1, 8, 8, 0), (1, 8, 8, -3),
                (1, 12, 12, 12), (1, 64, 64, 100),                    # more taps than the staged tile holds
                (1, 1 << 15, 1 << 14, 11), (1, 1 << 31, 1, 1),        # H W C >= 2^31
                (1 << 31, 8, 8, 3), (1 << 22, 1024, 1024, 11)):       # more workgroups than a launch holds
        assert q(*bad) == -1, bad
    assert q(1, 1 << 14, 1 << 14, 11) > 0


def test_cabi_argument_errors_launch_nothing():
    h = _lib.ssim_lib()
    err = _lib.lib().df_last_error
    buf = ctypes.create_string_buffer(1 << 17)
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, out, ws, sm, cm, pa, pb = (base + 8192 * i for i in range(8))      # 2 x 12 x 17 x 3 floats = 4896 bytes per image batch
    taps = (ctypes.c_float * 11)(*ref.taps(11, 1.5))
    ok = (2, 12, 17, 3, 11, 0.01, 0.03, -1.0, 1.0, None)

    def run(a=a, b=b, taps=taps, sm=sm, cm=cm, pa=pa, pb=pb, out=out, ws=ws, wsb=32, tail=ok):
        return h.df_ssim(a, b, taps, sm, cm, pa, pb, out, ws, wsb, *tail)
    assert run(a=None) == -1 and b"null image" in err()
    assert run(b=None) == -1 and b"null image" in err()
    assert run(taps=None) == -1 and b"null taps" in err()
    assert run(out=None) == -1 and b"null out" in err()
    assert run(ws=None) == -1 and b"null workspace" in err()
    assert run(cm=None) == -1 and b"go together" in err()
    assert run(pa=None) == -1 and b"go together" in err()
    for c in (0, 5, -1):
        assert run(tail=(2, 12, 17, c) + ok[4:]) == -1 and b"C must be in 1..4" in err()
    assert run(tail=(0, 12, 17, 3) + ok[4:]) == -1 and b"non-positive" in err()
    assert run(tail=(2, 12, 0, 3) + ok[4:]) == -1 and b"non-positive" in err()
    assert run(tail=ok[:4] + (0,) + ok[5:]) == -1 and b"filter_size" in err()
    assert run(tail=ok[:4] + (-2,) + ok[5:]) == -1 and b"filter_size" in err()
    assert run(tail=ok[:7] + (0.5, 0.5, None)) == -1 and b"differ" in err()
    assert run(tail=ok[:7] + (float("nan"), 1.0, None)) == -1 and b"finite" in err()
    assert run(tail=(2, 12, 17, 3, 12) + ok[5:]) == -2 and b"12 taps" in err()
    assert run(tail=(1, 1 << 15, 1 << 14, 3) + ok[4:], wsb=1 << 40) == -2 and b"int32 index" in err()
    assert run(a=a + 2) == -3 and run(sm=sm + 1) == -3 and run(pb=pb + 2) == -3
    assert run(out=out + 4) == -3 and b"8-byte" in err()
    assert run(ws=ws + 4) == -3 and b"8-byte" in err()
    assert run(wsb=31) == -4 and b"32 needed" in err()
    # overlaps: wherever one of the two is written
    assert run(out=a + 4888) == -1 and b"out overlaps a" in err()
    assert run(ws=out + 32) == -1 and b"the workspace overlaps out" in err()
    assert run(sm=b) == -1 and b"ssim_map overlaps b" in err()
    assert run(cm=sm + 4 * 2 * 2 * 7 - 4) == -1 and b"cs_map overlaps ssim_map" in err()
    assert run(pa=a) == -1 and b"pool_a overlaps a" in err()
    assert run(pb=pa + 4 * 2 * 6 * 9 * 3 - 4) == -1 and b"pool_b overlaps pool_a" in err()
    g = h.df_ssim_group_mean
    assert g(None, ws, 1, 2, None) == -1 and b"null out" in err()
    assert g(out, None, 1, 2, None) == -1 and b"null mean" in err()
    assert g(out, ws, 0, 2, None) == -1 and g(out, ws, 1, 0, None) == -1 and b"non-positive" in err()
    assert g(out, ws, 1 << 31, 1, None) == -2
    assert g(out + 4, ws, 1, 2, None) == -3 and g(out, ws + 4, 1, 2, None) == -3
    assert g(out, out + 56, 1, 2, None) == -1 and b"overlaps" in err()


def test_refusals_of_the_ops_without_a_device():
    a = torch.zeros((2, 12, 17, 3))
    for fn in (ops.ssim, ops.ms_ssim):
        with pytest.raises(NotImplementedError, match="requires grad"):
            fn(torch.zeros((2, 12, 17, 3), requires_grad=True), a)
        with pytest.raises(NotImplementedError, match="requires grad"):
            fn(a, torch.zeros((2, 12, 17, 3), requires_grad=True))
        with pytest.raises(ValueError, match="disagree in shape"):
            fn(a, torch.zeros((2, 12, 16, 3)))
        with pytest.raises(ValueError, match="must be float32"):
            fn(a, a.double())
        with pytest.raises(ValueError, match="must be float32"):
            fn(a.half(), a.half())
        with pytest.raises(ValueError, match="must be contiguous"):
            fn(torch.zeros((2, 12, 34, 3))[:, :, ::2], a)
        with pytest.raises(ValueError, match=r"\[N,H,W,C\] with C in 1..4"):
            fn(torch.zeros((2, 12, 17, 5)), torch.zeros((2, 12, 17, 5)))
        with pytest.raises(ValueError, match=r"\[N,H,W,C\] with C in 1..4"):
            fn(torch.zeros((12, 17, 3)), torch.zeros((12, 17, 3)))
        with pytest.raises(ValueError, match="finite and differ"):
            fn(a, a, min_val=1.0, max_val=1.0)
        with pytest.raises(TypeError, match="torch.Tensor"):
            fn(a.numpy(), a)
    with pytest.raises(ValueError, match="filter_size must be an integer >= 1"):
        ops.ssim(a, a, filter_size=0)
    with pytest.raises(ValueError, match="at most 11"):
        ops.ssim(torch.zeros((1, 20, 20, 1)), torch.zeros((1, 20, 20, 1)), filter_size=13)
    with pytest.raises(ValueError, match="filter_sigma"):
        ops.ssim(a, a, filter_sigma=0.0)
    with pytest.raises(ValueError, match=r"\[B,Y,X,C\] or \[B,Z,Y,X,C\]"):
        ops.field_ssim(torch.zeros((4, 5, 2)), torch.zeros((4, 5, 2)))
    with pytest.raises(ValueError, match="filter_size"):
        ops.field_ssim(a, a, filter_size=0)
    with pytest.raises(TypeError, match="unexpected argument"):
        ops.field_ssim(a, a, multiscale=True, filter_size=7)
    with pytest.raises(NotImplementedError):
        ops.field_ssim(torch.zeros((2, 3, 12, 17, 3), requires_grad=True), torch.zeros((2, 3, 12, 17, 3)))
    for name in ("fspecial_gauss", "ssim", "ms_ssim", "field_ssim", "ssim_workspace"):
        assert name in ops.__all__
    if not torch.cuda.is_available():                                    # everything above was refused before anything asked for a device
        for fn in (ops.ssim, ops.ms_ssim, ops.field_ssim):
            with pytest.raises(_lib.DeepFluidsHipError, match="no CPU path"):
                fn(a, a)


def test_evaluate_files_are_unchanged_by_default_and_gain_the_ssim_arrays(tmp_path):
    """``_eval_write`` fed with host rows of the field-metrics twin, as tests/test_field_metrics_host.py does"""
    fref = fmh.ref
    shape = (5, 4, 5, 6)
    g, x = fref.inputs(shape)
    raw = torch.from_numpy(fref.raw_words(fref.metrics(g, x, None, F32)))
    groups = [("0_1", ops.FieldMetrics(raw[:3], 3)), ("2_0", ops.FieldMetrics(raw[3:], 3))]
    FM = ops.FieldMetrics
    plain = trainer._eval_write(str(tmp_path / "a"), groups, 2.5)
    assert sorted(os.listdir(plain["dir"])) == ["0_1.npz", "2_0.npz", "summary.txt"]
    want = set(FM.QUANTITIES + FM.DERIVED) | {k + "_denorm" for k in FM.LINEAR} | {"x_range"}
    with np.load(os.path.join(plain["dir"], "2_0.npz")) as z:
        assert set(z.files) == want
    lines = open(os.path.join(plain["dir"], "summary.txt")).read().splitlines()
    assert len(lines) == 4 and [ln.split()[0] for ln in lines] == ["#", "0_1", "2_0", "total"]
    assert set(plain["total"]) == {"frames", "worst_frame"} | {q + s for q in trainer.EVAL_SUMMARY for s in ("_mean", "_max")}
    sims = {"0_1": {"ssim": np.array([0.9, 0.8, 1.0]), "ms_ssim": np.array([0.95, 0.85, 1.0])},
            "2_0": {"ssim": np.array([0.5, 0.7]), "ms_ssim": np.array([0.6, np.nan])}}
    with_ = trainer._eval_write(str(tmp_path / "b"), groups, 2.5, sims)
    with np.load(os.path.join(with_["dir"], "2_0.npz")) as z:
        assert set(z.files) == want | {"ssim", "ms_ssim"}
        np.testing.assert_array_equal(z["ssim"], sims["2_0"]["ssim"])
        assert z["ms_ssim"].dtype == np.float64
    assert with_["groups"]["0_1"]["ssim_min"] == 0.8 and with_["groups"]["0_1"]["ms_ssim_max"] == 1.0
    assert with_["total"]["ssim_min"] == 0.5 and with_["total"]["ssim_mean"] == np.mean([0.9, 0.8, 1.0, 0.5, 0.7])
    assert np.isnan(with_["total"]["ms_ssim_mean"])                       # a NaN frame is not hidden
    more = open(os.path.join(with_["dir"], "summary.txt")).read().splitlines()
    assert more[:4] == lines                                              # the first block is the text of today
    assert more[4].startswith("# group ssim_mean ssim_min ssim_max ms_ssim_mean") and [ln.split()[0] for ln in more[5:]] == ["0_1", "2_0", "total"]
    import inspect
    for cls in (trainer.Trainer, trainer.AETrainer):
        assert inspect.signature(cls.evaluate_).parameters["ssim"].default is False
