"""CPU tests of the restatement of the liquid solver's surface (tests/liquid_gf_ref.py): the averaged level set against closed forms,
the ghost-fluid system's properties in fp64, the condition the GPU tests rest on (the fp32 twin's preconditioned CG reaches `accuracy`
below the iteration cap on every input they use), and the argument checks of the Python surface that need no GPU."""
import inspect

import numpy as np
import pytest

import liquid_gf_ref as gref
import liquid_ref as ref
import particles_ref as pref


@pytest.mark.parametrize("shape", [(7, 9), (5, 7, 6)])
def test_levelset_closed_forms(shape):
    D = len(shape)
    R = float(pref.radius_of(D, 1.0, np.float64))
    # no particles: phi = R everywhere (and the band where asked for)
    none = gref.levelset_averaged(np.zeros((1, 0, D), np.float32), shape, bnd=0, smooth=0, smooth_neg=0)
    assert (none == R).all()
    band = gref.levelset_averaged(np.zeros((1, 0, D), np.float32), shape, bnd=1, smooth=2, smooth_neg=1, bound_value=3.0)
    inner = ref.interior_mask(shape, 1)[None]
    assert (band[~inner] == 3.0).all() and np.allclose(band[inner], R, rtol=1e-15)
    # one particle at a known offset: phi = |x_c - p| - R wherever its weight is positive and the window reaches it, R elsewhere
    p = (np.array([3.3, 2.6, 2.2][:D]))[None, None].astype(np.float32)
    phi = gref.levelset_averaged(p, shape, bnd=0, smooth=0, smooth_neg=0)[0]
    r = int(R) + 1
    cell = np.floor(p[0, 0]).astype(int)
    hit = 0
    for idx in np.ndindex(*shape):
        c = np.array(idx[::-1]) + 0.5
        d = float(np.sqrt(((c - p[0, 0].astype(np.float64)) ** 2).sum()))
        inside = all(abs(idx[::-1][a] - cell[a]) <= r for a in range(D)) and 1.0 - d * d / (4 * R * R) > 1e-6
        want = d - R if inside else R
        assert abs(phi[idx] - want) <= 1e-12, (idx, phi[idx], want)
        hit += inside
    assert hit >= 2 ** D                                                  # the support has radius 2R: at least the nearest 2^D centres
    # the twin is fp32 throughout and close
    p32 = gref.levelset_averaged(p, shape, bnd=0, smooth=0, smooth_neg=0, dtype=np.float32)
    assert p32.dtype == np.float32 and ref.max_err(p32[0], phi) < 1e-5


@pytest.mark.parametrize("shape,B,bnd", gref.LEVELSET_CASES)
@pytest.mark.parametrize("radius_factor", [1.0, 2.5])
def test_levelset_window_against_a_brute_force_over_all_particles(shape, B, bnd, radius_factor):
    """the restatement walks the sorted cell ranges as the kernel does; this one does not: it looks at every particle"""
    pos = gref.levelset_positions(shape, B, bnd, 11)
    raw = gref.levelset_averaged(pos, shape, radius_factor, 0, 0, 1.0, 0, np.float64)
    brute = gref.levelset_raw_brute(pos, shape, radius_factor)
    assert (brute < float(pref.radius_of(len(shape), radius_factor, np.float64))).any()
    assert ref.max_err(raw, brute) <= 1e-12


def test_smoothing_passes():
    rng = np.random.RandomState(1)
    phi = rng.standard_normal((2, 6, 7))
    s1 = gref.smooth_pass(phi, 1)
    inner = ref.interior_mask((6, 7), 1)[None]
    assert (s1[~np.broadcast_to(inner, phi.shape)] == phi[~np.broadcast_to(inner, phi.shape)]).all()
    want = (phi[0, 2, 3] + phi[0, 2, 2] + phi[0, 2, 4] + phi[0, 1, 3] + phi[0, 3, 3]) / 5
    assert abs(s1[0, 2, 3] - want) < 1e-15
    s2 = gref.smooth_pass(phi, 2)
    assert (s2 <= phi).all() and (s2 < phi).any() and ((s2 == phi) | (s2 == s1)).all()
    assert (gref.smooth_pass(phi, 0, 2, 9.0)[~np.broadcast_to(ref.interior_mask((6, 7), 2)[None], phi.shape)] == 9.0).all()


@pytest.mark.parametrize("shape", [(8, 8), (6, 6, 6)])
def test_dense_matrix_is_symmetric_with_positive_diagonal_and_projects(shape):
    liquid, vel = gref.ragged(shape, 2, 3)
    phi = gref.branch_phi(liquid, 7)
    for c in gref.GF_CLAMPS:
        assert all(n > 0 for n in gref.theta_branches(phi, liquid, c)), gref.theta_branches(phi, liquid, c)
        for e in range(2):
            A, cells = gref.dense_matrix(liquid[e], phi[e].astype(np.float64), 1, c)
            assert np.array_equal(A, A.T) and (np.diag(A) > 0).all()
            off = A - np.diag(np.diag(A))
            assert set(np.unique(off)) <= {0.0, -1.0}
            assert (np.diag(A) >= -off.sum(axis=1)).all() and np.diag(A).max() <= 6.0 / c
            assert np.linalg.eigvalsh(A).min() > -1e-9
        out, p = gref.exact_projection(vel, liquid, phi, 1, c)
        assert float(np.abs(gref.residual(vel, p, liquid, phi, 1, c)).max()) <= 1e-9
        assert not p[~liquid].any()
    # every theta 1: the first-order system; every liquid region of these masks touches air, so it is non-singular (the GPU test's
    # comparison of the two paths' pressures rests on that)
    one = gref.unit_theta_phi(liquid)
    for e in range(2):
        assert np.linalg.cond(gref.dense_matrix(liquid[e], one[e].astype(np.float64))[0]) < 1e6
    x = np.random.RandomState(2).standard_normal(liquid.shape) * liquid
    np.testing.assert_array_equal(gref.apply_A(x, liquid, gref.diagonal(one, liquid)), ref.apply_A(x, liquid, 1))
    np.testing.assert_array_equal(gref.correct(vel, x, liquid, one), ref.correct(vel, x, liquid, 1))


@pytest.mark.parametrize("shape", gref.HYDRO_SHAPES)
@pytest.mark.parametrize("s", gref.HYDRO_S)
def test_hydrostatic_column_in_fp64(shape, s):
    D = len(shape)
    g = gref.HYDRO_G
    liquid, vel, phi, depth = gref.hydrostatic_case(shape, s)
    out, p = gref.exact_projection(vel, liquid, phi)
    # phi is handed over in fp32: theta = s up to its rounding
    assert float(np.abs(p - abs(g) * depth).max()) <= 1e-6 * abs(g) * depth.max()
    assert float(np.abs(out).max()) <= 1e-6 * abs(g)
    # the first-order surface puts |g| * 1 into the top cell: the two paths differ where they should
    _, p1 = ref.exact_projection(vel, liquid, 1)
    top = (slice(None),) * (D - 1) + (shape[-2] // 2 - 1,)
    np.testing.assert_allclose(p1[top][liquid[top]], abs(g), rtol=1e-12)
    np.testing.assert_allclose(p[top][liquid[top]], abs(g) * s, rtol=1e-6)


def _solver_inputs():
    for name, liquid, vel, phi, c in gref.solve_cases():
        yield name, liquid, vel, phi, c, 1e-4
    for shape in (8, 8), (6, 6, 6):
        liquid, vel = gref.ragged(shape, 2, 3)
        yield "unit-theta-%d" % len(shape), liquid, vel, gref.unit_theta_phi(liquid), 1e-4, 1e-5
    for shape in gref.HYDRO_SHAPES:
        for s in gref.HYDRO_S:
            liquid, vel, phi, _ = gref.hydrostatic_case(shape, s)
            yield "hydro-%d-%g" % (len(shape), s), liquid, vel, phi, 1e-4, 1e-6


def test_twin_pcg_reaches_accuracy_below_the_cap_on_every_gpu_solver_input():
    for name, liquid, vel, phi, c, acc in _solver_inputs():
        cap = ref.default_max_iter(liquid.shape[1:])
        x, iters, r = gref.pcg(vel, liquid, phi, 1, acc, cap, c, np.float32)
        print("%s: twin iterations %s of %d, max|r| %.3e" % (name, iters.tolist(), cap, float(np.abs(r).max())))
        assert (iters > 0).all() and (iters < cap).all(), (name, iters, cap)
        assert float(np.abs(r).max()) <= acc, name


@pytest.mark.parametrize("shape", gref.STEP_SHAPES)
def test_the_step_inputs_sort_alike_and_converge(shape):
    """what the GPU's four-step test rests on: twin and fp64 sort every particle into the same cell, every solve stops below the cap"""
    from test_gpu_liquid import drop_scene                               # the scene of the GPU step test itself
    pos0, vel0 = drop_scene(shape, gref.STEP_SEEDS[shape])
    pvel0 = ref.sample(vel0, pos0, np.float32)
    s64 = dict(pos=pos0.astype(np.float64), pvel=pvel0.astype(np.float64), vel=vel0.astype(np.float64))
    s32 = dict(pos=pos0, pvel=pvel0, vel=vel0)
    cap = ref.default_max_iter(shape)
    for t in range(4):
        s64 = gref.step(s64["pos"], s64["pvel"], s64["vel"], 0.5, accuracy=1e-9, dtype=np.float64)
        s32 = gref.step(s32["pos"], s32["pvel"], s32["vel"], 0.5, accuracy=1e-6, dtype=np.float32)
        np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
        assert (s32["iters"] < cap).all() and (s64["iters"] < cap).all(), (t, s32["iters"], s64["iters"], cap)


def test_surface_argument_validation_without_a_gpu():
    import torch
    from deep_fluids_amd import ops
    vel = torch.zeros((2, 6, 7, 2))
    flags = torch.zeros((2, 6, 7), dtype=torch.uint8)
    for bad in (torch.zeros((2, 6, 8)), torch.zeros((2, 6, 7), dtype=torch.float64), torch.zeros((2, 6, 7)), np.zeros((2, 6, 7), np.float32)):
        with pytest.raises(ValueError, match="phi must be"):              # shape, dtype, device (no GPU tensor here), type
            ops.solve_pressure_liquid(vel, flags, phi=bad)
    for c in (0.0, -1e-4, 1.5, float("nan")):
        with pytest.raises(ValueError, match="gf_clamp"):
            ops.solve_pressure_liquid(vel, flags, phi=torch.zeros((2, 6, 7)), gf_clamp=c)
        with pytest.raises(ValueError, match="gf_clamp"):
            ops.liquid_step(None, None, None, 0.5, ghost_fluid=True, gf_clamp=c)
        with pytest.raises(ValueError, match="gf_clamp"):
            ops.simulate_liquid(None, None, None, 2, ghost_fluid=True, gf_clamp=c)
    pos = torch.zeros((1, 4, 2))
    for kw in (dict(smooth=-1), dict(smooth_neg=-2), dict(bnd=-1), dict(radius_factor=-1.0)):
        with pytest.raises(ValueError):
            ops.particle_levelset_averaged(pos, (6, 7), **kw)
    assert "particle_levelset_averaged" in ops.__all__


def test_defaults_call_nothing_new(monkeypatch):
    """the new arguments default to the old behaviour in every signature, and a default solve names no `_gf` entry point"""
    import torch
    from deep_fluids_amd import data, ops
    for fn, want in ((ops.solve_pressure_liquid, dict(phi=None, gf_clamp=1e-4)), (ops.liquid_step, dict(ghost_fluid=False, radius_factor=1.0, gf_clamp=1e-4)),
                     (ops.simulate_liquid, dict(ghost_fluid=False, radius_factor=1.0, gf_clamp=1e-4)), (ops.pressure_workspace, dict(ghost_fluid=False)),
                     (data.generate_liquid_dataset, dict(ghost_fluid=False)), (data.generate_liquid3_d_r_dataset, dict(ghost_fluid=False)),
                     (data.generate_liquid3_vis_dataset, dict(ghost_fluid=False))):
        par = inspect.signature(fn).parameters
        for k, v in want.items():
            assert par[k].default == v or (v is None and par[k].default is None), (fn.__name__, k)
    # record the entry points a default solve and a default workspace would call, with the tensors' checks and the launches stubbed out
    names = []
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name))
    monkeypatch.setattr(ops, "query", lambda name, *a: names.append(name) or 4096)
    monkeypatch.setattr(ops, "_prep", lambda t, name="tensor": t)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_read_word", lambda t: 0)
    monkeypatch.setattr(ops, "_liquid_flags_arg", lambda f, v, who: f)
    monkeypatch.setattr(ops, "_smoke_out", lambda out, like, who: like)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    vel = torch.zeros((1, 6, 7, 2))
    ops.solve_pressure_liquid(vel, torch.zeros((1, 6, 7), dtype=torch.uint8))
    assert names and not [n for n in names if n.endswith("_gf") or "levelset" in n], names
    default = list(names)
    del names[:]
    ops.solve_pressure_liquid(vel, torch.zeros((1, 6, 7), dtype=torch.uint8), phi=torch.zeros((1, 6, 7)))
    assert [n for n in names if n.endswith("_gf")] and len(names) == len(default), names
