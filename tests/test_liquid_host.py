"""CPU tests of the restatement of the liquid solver step itself (tests/liquid_ref.py): the properties the definition in
include/deepfluids_hip.h is meant to have, checked in fp64 before any kernel is compared with it; and the argument checks of the Python
surface that need no GPU."""
import numpy as np
import pytest

import liquid_ref as ref
import particles_ref as pref
from smoke_ref import interior_mask

SHAPES = [(9, 7), (6, 7, 5)]


def _particles(shape, B, N, seed, bnd=1):
    rng = np.random.RandomState(seed)
    pos = pref.make_positions(shape, B, N, bnd, seed)
    pvel = rng.uniform(-1, 1, pos.shape).astype(np.float32)
    return pos, pvel


@pytest.mark.parametrize("shape", SHAPES)
def test_p2g_weights_sum_to_one_and_uniform_velocity_comes_back(shape):
    D = len(shape)
    pos, _ = _particles(shape, 2, 200, 3)
    W, _ = ref.face_weights(pos[0].astype(np.float64), shape)
    np.testing.assert_allclose(W.sum(axis=-1), 1.0, rtol=0, atol=4e-16)
    u0 = np.array([0.25, -1.5, 0.75][:D])
    pvel = np.broadcast_to(u0, pos.shape).copy()
    sp, su, cs, _ = ref.sort_particles(pos, pvel, shape)
    vel, weight, known = ref.p2g(sp, su, cs, shape, np.float64)
    assert known.any() and not known.all()
    for a in range(D):
        hit = weight[..., a] > 0
        np.testing.assert_allclose(vel[..., a][hit], u0[a], rtol=1e-14)
        assert not vel[..., a][~hit].any()
    # the total weight of component a is the number of particles: every particle's weights sum to 1
    np.testing.assert_allclose(weight.reshape(2, -1, D).sum(axis=1), 200.0, rtol=1e-13)


@pytest.mark.parametrize("shape", SHAPES)
def test_scatter_is_the_transpose_of_the_sample(shape):
    D = len(shape)
    rng = np.random.RandomState(5)
    pos, pvel = _particles(shape, 2, 300, 7)
    sp, su, cs, _ = ref.sort_particles(pos, pvel, shape)
    g = rng.standard_normal((2,) + shape + (D,))
    num, _, _ = ref.p2g(sp, su, cs, shape, np.float64, normalise=False)
    lhs = float((num * g).sum())
    rhs = float((su.astype(np.float64) * ref.sample(g, sp, np.float64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(rhs))
    # the fp32 twin's sums are those of a sequential loop
    n32, d32, _ = ref.p2g(sp, su, cs, shape, np.float32, normalise=False)
    assert n32.dtype == np.float32 and ref.max_err(n32, num) < 1e-4


def _ragged_liquid(shape, bnd, seed, B=2):
    rng = np.random.RandomState(seed)
    liquid = (rng.uniform(size=(B,) + shape) < 0.7) & interior_mask(shape, bnd)[None]
    return liquid


@pytest.mark.parametrize("shape", [(8, 8), (6, 6, 6)])
def test_dense_projection_leaves_liquid_cells_divergence_free(shape):
    D = len(shape)
    rng = np.random.RandomState(11)
    liquid = _ragged_liquid(shape, 1, 2)
    vel = ref.forces(rng.standard_normal((2,) + shape + (D,)), liquid, (0.0,) * D, 1)
    out, p = ref.exact_projection(vel, liquid, 1)
    assert float(np.abs(ref.divergence(out, liquid)).max()) <= 1e-12
    assert not p[~liquid].any()
    # faces with no liquid cell are left alone, wall faces are 0
    for a in range(D):
        live = ref.live_face(liquid, 1, a)
        kept = ref.both_interior(shape, 1, a)[None]
        np.testing.assert_array_equal(out[..., a][kept & ~live], vel[..., a][kept & ~live])
        assert not out[..., a][np.broadcast_to(~kept, live.shape)].any()
    # with every interior cell liquid the system is the closed box's
    import smoke_ref as sref
    full = np.broadcast_to(interior_mask(shape, 1), (1,) + shape).copy()
    x = rng.standard_normal((1,) + shape) * full
    np.testing.assert_array_equal(ref.apply_A(x, full, 1), sref.apply_A(x, 1))


@pytest.mark.parametrize("shape", [(12, 16), (8, 10, 8)])
def test_hydrostatic_rest(shape):
    """a flat basin at rest under gravity: one force + projection gives back zero velocity, to the solve's accuracy"""
    D = len(shape)
    liquid = np.zeros((1,) + shape, bool)
    liquid[(slice(None),) * (D - 1) + (slice(0, shape[-2] // 2),)] = True
    liquid &= interior_mask(shape, 1)[None]
    g = -0.05
    force = (0.0, g, 0.0)[:D]
    v = ref.forces(np.zeros((1,) + shape + (D,)), liquid, force, 1)
    assert float(np.abs(v).max()) == abs(g)
    out, p = ref.exact_projection(v, liquid, 1)
    for a in range(D):
        assert float(np.abs(out[..., a][ref.live_face(liquid, 1, a)]).max()) <= 1e-12
    acc = 1e-6
    out, p, iters = ref.solve_pressure(v, liquid, 1, acc, None, np.float64)
    for a in range(D):
        # |v| <= the pressure error across a face; the residual bound times the depth of the column is generous
        assert float(np.abs(out[..., a][ref.live_face(liquid, 1, a)]).max()) <= acc * shape[-2]
    assert 0 < int(iters[0]) < ref.default_max_iter(shape)


def test_extrapolation_layers_and_marks():
    shape = (9, 7)
    v = np.zeros((1,) + shape + (2,))
    m = np.zeros((1,) + shape + (2,), np.uint8)
    v[0, 3, 4, 0] = 2.0
    m[0, 3, 4, 0] = 1
    for dist in (0, 1, 2, 4):
        out, mk = ref.extrapolate(v, m, dist, 1)
        assert int(mk.max()) == (1 if dist == 0 else dist + 1)
        # a single source: every filled face carries its value, and the filled set is the |.|_1 ball clipped to the kept faces
        filled = mk[0, ..., 0] > 0
        assert (out[0, ..., 0][filled] == 2.0).all() and not mk[..., 1].any()
        yy, xx = np.mgrid[:shape[0], :shape[1]]
        want = (np.abs(yy - 3) + np.abs(xx - 4) <= dist) & ref.both_interior(shape, 1, 0)
        np.testing.assert_array_equal(filled, want)


def test_surface_argument_validation_without_a_gpu():
    from deep_fluids_amd import ops
    with pytest.raises(NotImplementedError):
        ops.liquid_step(None, None, None, 0.5, open_bound=True)
    with pytest.raises(NotImplementedError):
        ops.simulate_liquid(None, None, None, 3, open_bound=True)
    with pytest.raises(ValueError):
        ops.liquid_initial_state((8, 8), np.zeros((8, 9), np.float32))
    f = ops.default_gravity_force((64, 128), 0.5)
    assert f == (0.0, -1e-3 * 0.5 * 128) and f == ref.default_force((64, 128), 0.5)
    f3 = ops.default_gravity_force((96, 48, 96), 0.5)
    assert f3[0] == 0.0 and f3[2] == 0.0 and f3[1] < 0
    # the initial velocity stamp is host NumPy: the y faces inside the sphere, nothing else
    want = ref.initial_velocity((12, 16), [((8.0, 7.0), 3.0)])
    assert want[..., 0].any() == False and (want[..., 1] == -1).sum() > 20       # noqa: E712


def test_generator_argument_validation_without_a_gpu(tmp_path):
    from deep_fluids_amd.data import generate_liquid3_d_r_dataset, generate_liquid_dataset
    for gen in (generate_liquid_dataset, generate_liquid3_d_r_dataset):
        with pytest.raises(NotImplementedError):
            gen(str(tmp_path / "a"), open_bound=True)
        with pytest.raises(ValueError):
            gen(str(tmp_path / "b"), num_param=2)
        with pytest.raises(ValueError):
            gen(str(tmp_path / "c"), p0="frames")
    assert not list(tmp_path.iterdir())                                      # refused before anything is written
