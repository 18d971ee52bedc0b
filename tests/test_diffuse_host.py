"""CPU checks of the implicit velocity diffusion's restatement (tests/diffuse_ref.py) and of the host arithmetic of the viscous liquid
set: the restatement against a dense solve, the structure of the system matrix, the identity at alpha = 0, the script's alphas and the
frame-to-step map.  The GPU side is tests/test_gpu_diffuse.py."""
import numpy as np
import pytest

import diffuse_ref as ref
from smoke_ref import interior_mask

CASES = [(9, 30), (6, 7, 9)]
ALPHA = (0.23, 23.04)


def _vel(shape, B=2, seed=7):
    return np.random.RandomState(seed).standard_normal((B,) + shape + (len(shape),)).astype(np.float32)


@pytest.mark.parametrize("shape", CASES)
def test_fp64_cg_agrees_with_the_dense_solve(shape):
    v = _vel(shape)
    x, iters, r, _ = ref.cg(v, ALPHA, 1, 1e-13, 2000, np.float64)
    want = ref.dense(v, ALPHA, 1)
    err = float(np.abs(x - want).max())
    print("%s: fp64 CG vs dense %.3e after %s iterations" % (shape, err, iters.tolist()))
    assert err <= 1e-10
    assert (iters > 0).all() and (iters < 2000).all()
    band = ~interior_mask(shape, 1)
    assert (x[:, band] == v[:, band].astype(np.float64)).all()
    # the residual helper sees the same system
    assert float(np.abs(ref.residual(want, v, ALPHA, 1)).max()) <= 1e-10


@pytest.mark.parametrize("shape", CASES)
def test_fp32_twin_iteration_counts_at_the_test_shapes(shape):
    """what tests/test_gpu_diffuse.py relies on: at accuracy 1e-4 the twin converges far inside max_iter = 200, and on (6,7,9) the default
    cap (9) lies below the count of every pair at alpha = 23.04"""
    v = _vel(shape)
    _, iters, _, _ = ref.cg(v, ALPHA, 1, 1e-4, 200, np.float32)
    print("%s: twin iterations %s (default cap %d)" % (shape, iters.tolist(), ref.default_max_iter(shape)))
    assert (iters > 0).all() and (iters <= 100).all()
    if len(shape) == 3:
        _, hot, _, _ = ref.cg(v, 23.04, 1, 1e-4, 200, np.float32)
        assert (hot > ref.default_max_iter(shape)).all()


@pytest.mark.parametrize("shape", [(5, 6), (4, 5, 6)])
@pytest.mark.parametrize("bnd", [1, 2])
def test_the_matrix_is_symmetric_and_its_rows_sum_to_one(shape, bnd):
    shape = tuple(n + 2 * (bnd - 1) for n in shape)
    A, G, cells, band = ref.matrices(shape, 2.3, bnd)
    al = np.float64(np.float32(2.3))
    D = len(shape)
    assert (A == A.T).all()
    assert np.allclose(np.diag(A), 1 + 2 * D * al, rtol=0, atol=1e-12)
    assert ((A - np.diag(np.diag(A)) == 0) | (A - np.diag(np.diag(A)) == -al)).all() and ((G == 0) | (G == al)).all()
    # with the Dirichlet terms moved back to the left every row of (I - alpha * Laplacian) sums to 1: 2D neighbours in all
    np.testing.assert_allclose(A.sum(axis=1) - G.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert ((A != 0).sum(axis=1) - 1 + (G != 0).sum(axis=1) == 2 * D).all()
    assert np.linalg.eigvalsh(A).min() >= 1.0 - 1e-12                      # I + alpha * (a positive semi-definite matrix)


@pytest.mark.parametrize("shape", CASES)
def test_alpha_zero_is_the_identity(shape):
    v = _vel(shape)
    for dtype in (np.float32, np.float64):
        x, iters, r, _ = ref.cg(v, 0.0, 1, 1e-4, 200, dtype)
        assert not iters.any() and not r.any()
        assert (x == v.astype(dtype)).all()
    x, iters, _, _ = ref.cg(v, (0.0, 2.3), 1, 1e-4, 200, np.float32)
    assert (x[0].view(np.uint32) == v[0].view(np.uint32)).all() and not iters[0].any() and (iters[1] > 0).all()
    x, iters, _, _ = ref.cg(v, ALPHA, 1, 1e-4, 0, np.float32)
    assert (x.view(np.uint32) == v.view(np.uint32)).all() and not iters.any()


def test_the_scripts_alphas_and_the_default_cap():
    from deep_fluids_amd import ops
    vis_list = 2 * np.logspace(-5, -2, 4)
    p_list = np.linspace(0, 3, 4)
    alphas = [ops.diffusion_alpha(vis_list[int(p)], 0.125, 96) for p in p_list]
    np.testing.assert_allclose(alphas, [0.02304, 0.2304, 2.304, 23.04], rtol=1e-12)
    assert ops.diffusion_alpha(2e-5, 0.125, 96) == 2e-5 * 0.125 * 96 ** 2       # x, not the largest extent
    assert ops.default_diffusion_max_iter((48, 72, 96)) == 96 and ops.default_diffusion_max_iter((64, 128)) == 512
    assert ops.default_diffusion_max_iter((6, 7, 9)) == ref.default_max_iter((6, 7, 9)) == 9
    assert ops.default_diffusion_max_iter((9, 30)) == ref.default_max_iter((9, 30)) == 120


def test_frame_to_step_map():
    """frame f of the script is saved when timeTotal, which advances by time_step = 1/8 per step, is a whole number: step f * 8"""
    time_step, frames = 0.125, 5
    substeps = int(round(1 / time_step))
    assert substeps == 8
    total, fired = 0.0, []
    for step in range((frames - 1) * substeps + 1):
        if float(total).is_integer():
            fired.append(step)
        total += time_step
    assert fired == [f * 8 for f in range(frames)]
    # keep_every of ops.simulate_liquid: steps 0, k, 2k, ...
    assert [t for t in range((frames - 1) * substeps + 1) if t % substeps == 0] == fired


def test_the_generator_refuses_what_it_does_not_do(tmp_path):
    from deep_fluids_amd.data import generate_liquid3_vis_dataset
    with pytest.raises(NotImplementedError):
        generate_liquid3_vis_dataset(str(tmp_path / "open"), open_bound=True)
    with pytest.raises(ValueError):
        generate_liquid3_vis_dataset(str(tmp_path / "p0"), p0="src_x_pos")
    with pytest.raises(ValueError):
        generate_liquid3_vis_dataset(str(tmp_path / "dt"), time_step=0.3)
