"""Host side of the multigrid preconditioner of the smoke pressure solve (no GPU): properties of the NumPy restatement
tests/smoke_mg_ref.py that the GPU tests lean on -- the coarse weights are the dense Galerkin products, the V-cycle is symmetric and
positive on the active cells, preconditioned CG reaches the exact projection, the fp32 twin holds the iteration cap -- and the refusals
of the ``preconditioner=`` keyword that need no device."""
import numpy as np
import pytest

import smoke_mg_ref as mg
import smoke_obs_ref as oref
import smoke_open_ref as pref
from deep_fluids_amd import _lib, ops

# The restatement is pinned to the library it restates: its parameters are the ones the C ABI answers and ops defaults to, so every test
# below is a statement about the shipped scheme (and this module does not import without it).
assert mg.ALPHA == ops.DEFAULT_MG_ALPHA
assert mg.NU == _lib.lib().df_mg_sweeps(0) and mg.COARSEST_SWEEPS == _lib.lib().df_mg_sweeps(1)
assert np.float32(_lib.lib().df_mg_omega()) == mg.omega(np.float32)


def _abi_levels(shape):
    dims = ([1] if len(shape) == 2 else []) + list(shape)
    return _lib.lib().df_mg_levels(len(shape), *dims)


SMALL = [((6, 6), 1), ((9, 7), 1), ((7, 8, 6), 1)]
CAP_SHAPES = [((17, 130), 1), ((24, 32, 24), 1)]


def _cases(shape, bnd):
    """(name, obstacle [1,..], bits): every obstacle case on the closed box, and one open-side case"""
    c = oref.obstacle_cases(shape, bnd)
    out = [(n, c[n][None], 0) for n in sorted(c)]
    out.append(("none-open", c["none"][None], pref.sides("XyY", len(shape))))
    out.append(("block-open", c["block"][None], pref.sides("XyY", len(shape))))
    return out


@pytest.mark.parametrize("shape,bnd", SMALL)
def test_coarse_weights_are_the_dense_galerkin_product(shape, bnd):
    for name, obs, bits in _cases(shape, bnd):
        levs = mg.hierarchy(obs, bnd, bits)
        A0, _ = pref.dense_A(shape, bnd, obs[0], bits)
        cells = np.flatnonzero(oref.fluid_mask(obs, bnd).ravel())
        full = mg.dense_level(levs[0])
        assert np.array_equal(full[np.ix_(cells, cells)], A0), name          # level 0 is the solve's own matrix
        full[np.ix_(cells, cells)] = 0
        assert not full.any(), name                                           # and nothing else
        s = shape
        for l in range(len(levs) - 1):
            P = mg.dense_P(s)
            assert np.array_equal(P.T @ mg.dense_level(levs[l]) @ P, mg.dense_level(levs[l + 1])), (name, l)
            s = tuple((n + 1) // 2 for n in s)
        assert max(s) <= 2 and levs[-1]["diag"].shape[1:] == s and len(levs) == _abi_levels(shape)
        for lev, l32 in zip(levs, mg.hierarchy(obs, bnd, bits, np.float32)):  # the counts are exact in float32
            for k in ("dir", "diag", "w"):
                assert np.asarray(l32[k]).dtype == np.float32 and np.array_equal(np.asarray(l32[k], np.float64), np.asarray(lev[k])), (name, k)


@pytest.mark.parametrize("shape,bnd", SMALL)
def test_the_cycle_is_symmetric_and_positive_on_the_active_cells(shape, bnd):
    rng = np.random.RandomState(3)
    for name, obs, bits in _cases(shape, bnd):
        levs = mg.hierarchy(obs, bnd, bits)
        for alpha in (1.0, ops.DEFAULT_MG_ALPHA):
            for _ in range(3):
                u, v = rng.standard_normal((2, 1) + shape)
                a, b = float((u * mg.vcycle(levs, v, alpha)).sum()), float((mg.vcycle(levs, u, alpha) * v).sum())
                assert abs(a - b) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(v), (name, alpha)
            if alpha != ops.DEFAULT_MG_ALPHA:
                continue
            M = mg.dense_M(levs, alpha)
            act = np.flatnonzero((levs[0]["diag"] > 0).ravel())
            off = np.setdiff1d(np.arange(M.shape[0]), act)
            assert not M[off].any() and not M[:, off].any(), name              # z = 0 on inactive cells, which feed nothing
            if act.size:
                lo = float(np.linalg.eigvalsh(0.5 * (M + M.T)[np.ix_(act, act)]).min())
                assert lo > 0, (name, alpha, lo)                               # <r, M r> > 0 for every r with a component on an active cell


def test_solid_entry_and_enclosed_cell_give_zero():
    shape, bnd = (9, 7), 1
    c = oref.obstacle_cases(shape, bnd)
    obs = np.stack([c["solid"], c["enclosed"]])
    rng = np.random.RandomState(5)
    r = rng.standard_normal((2,) + shape)
    for dtype in (np.float64, np.float32):
        levs = mg.hierarchy(obs, bnd, 0, dtype)
        assert len(levs) == _abi_levels(shape)
        z = mg.vcycle(levs, r.astype(dtype), ops.DEFAULT_MG_ALPHA)
        mid = tuple(n // 2 for n in shape)
        assert z.dtype == dtype and not z[0].any() and z[1][mid] == 0 and oref.fluid_mask(obs, bnd)[1][mid] and z[1].any()


@pytest.mark.parametrize("shape,bnd", SMALL)
def test_fp64_preconditioned_cg_reaches_the_exact_projection(shape, bnd):
    names = sorted(oref.obstacle_cases(shape, bnd))
    obs = np.stack([oref.obstacle_cases(shape, bnd)[n] for n in names])
    for bits in (0, pref.sides("XyY", len(shape))):
        w = pref.solve_input(shape, bnd, obs, bits)
        vex, _ = pref.exact_projection(w, obs, bits, bnd)
        xp, itp, _, broke = mg.pcg(w, obs, bits, bnd, 1e-10, 400, np.float64, ops.DEFAULT_MG_ALPHA)
        x0, it0, _, _ = mg.pcg(w, obs, bits, bnd, 1e-10, 400, np.float64, precondition=False)
        dist = [float(np.abs(pref.extrapolate(pref.correct(w, x, obs, bits, bnd, np.float64), bits, bnd) - vex).max()) for x in (xp, x0)]
        print("%s open %d: iterations mg %s plain %s  distance from the exact projection mg %.3e plain %.3e" % (shape, bits, itp.tolist(), it0.tolist(), dist[0], dist[1]))
        assert not broke.any() and (itp < 400).all()
        assert dist[0] <= max(dist[1], 1e-9)


@pytest.mark.parametrize("shape,bnd", CAP_SHAPES)
def test_the_fp32_twin_needs_a_quarter_of_the_plain_iterations(shape, bnd):
    """a condition, not a measurement: closed box, every obstacle case, one open-side case"""
    nd = len(shape)
    c = oref.obstacle_cases(shape, bnd)
    names = sorted(c)
    obs = np.stack([c[n] for n in names])
    max_iter = ops.default_max_iter(shape)
    assert len(mg.hierarchy(obs[:1], bnd)) == _abi_levels(shape)
    for bits in (0, pref.sides("XyY", nd)):
        w = pref.solve_input(shape, bnd, obs, bits)
        _, it0, _, _ = mg.pcg(w, obs, bits, bnd, 1e-4, max_iter, np.float32, precondition=False)
        _, it, _, broke = mg.pcg(w, obs, bits, bnd, 1e-4, max_iter, np.float32, ops.DEFAULT_MG_ALPHA)
        print("%s open %d %s: plain %s mg %s" % (shape, bits, names, it0.tolist(), it.tolist()))
        assert not broke.any()
        assert (4 * it <= it0).all()
        assert (it[[n != "solid" for n in names]] > 0).all()


def test_refusals_that_need_no_gpu():
    import torch
    v = torch.zeros((1, 8, 8, 2))
    d = torch.zeros((1, 8, 8))
    for bad in ("mic0", "MG", 1, True, object()):
        with pytest.raises(ValueError, match="preconditioner"):
            ops.solve_pressure(v, preconditioner=bad)
        with pytest.raises(ValueError, match="preconditioner"):
            ops.smoke_step(d, v, 0.5, preconditioner=bad)
        with pytest.raises(ValueError, match="preconditioner"):
            ops.simulate_smoke(d, v, 2, preconditioner=bad)
    for pre in ("mg", "mic0"):
        with pytest.raises(ValueError, match="preconditioner"):
            ops.solve_pressure_liquid(v, None, preconditioner=pre)
        with pytest.raises(ValueError, match="preconditioner"):
            ops.diffuse_velocity(v, 1.0, preconditioner=pre)
        with pytest.raises(ValueError, match="preconditioner"):
            ops.liquid_step(None, None, v, 0.5, preconditioner=pre)
        with pytest.raises(ValueError, match="preconditioner"):
            ops.simulate_liquid(None, None, v, 2, preconditioner=pre)
    with pytest.raises(ValueError):
        ops.multigrid_apply("mg", d)


def test_the_c_abi_answers_sizes_without_a_device():
    h = _lib.lib()
    assert h.df_mg_sweeps(2) == -1
    assert h.df_mg_levels(2, 1, 130, 17) == len(mg.hierarchy(np.zeros((1, 130, 17), np.uint8), 1))
    assert h.df_mg_levels(3, 33, 20, 18) == len(mg.hierarchy(np.zeros((1, 33, 20, 18), np.uint8), 1))
    assert h.df_mg_levels(2, 2, 8, 8) == -1 and h.df_mg_levels(2, 1, 3, 8) == -1 and h.df_mg_hierarchy_bytes(4, 1, 1, 8, 8) == -1
    n = sum(int(np.prod(l["diag"].shape)) for l in mg.hierarchy(np.zeros((3, 12, 10), np.uint8), 1))
    assert h.df_mg_hierarchy_bytes(2, 3, 1, 12, 10) == 4 * 7 * n                    # D weights, dir, diag, r | z, two x buffers
    assert h.df_mg_level_offset(2, 3, 1, 12, 10, 0, 0) == 0 and h.df_mg_level_offset(2, 3, 1, 12, 10, 1, 0) == 7 * 3 * 120
    assert h.df_mg_level_offset(2, 3, 1, 12, 10, 0, 7) == -1 and h.df_mg_level_offset(2, 3, 1, 12, 10, 9, 0) == -1
    assert h.df_mg_apply(None, 0, None, 2, 1, 1, 8, 8, 1.8, None) != 0 and b"hierarchy" in h.df_last_error()
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    assert h.df_mg_apply(a, 1 << 15, a + (1 << 15), 2, 1, 1, 8, 8, 2.0, None) != 0 and b"alpha" in h.df_last_error()
    assert h.df_mg_apply(a, 16, a + (1 << 15), 2, 1, 1, 8, 8, 1.8, None) != 0 and b"needed" in h.df_last_error()
    assert h.df_mg_build(a, 1 << 15, None, 2, 1, 1, 8, 8, 0, 0, None) != 0 and b"boundary width" in h.df_last_error()
    assert h.df_mg_build(a, 1 << 15, None, 2, 1, 1, 8, 8, 1, 16, None) != 0 and b"open_sides" in h.df_last_error()
