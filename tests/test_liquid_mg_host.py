"""CPU checks of the multigrid preconditioner for the liquid systems (include/deepfluids_hip_liquid_mg.h): level 0 of the three systems
against the restatements that are already tested, the scheme's symmetry, the iteration counts of the fp32 twin, plain against
multigrid, and the argument checks that need no GPU."""
import ctypes

import numpy as np
import pytest

import diffuse_ref as dref
import liquid_gf_ref as gref
import liquid_mg_ref as lmg
import liquid_ref as lref
import smoke_mg_ref as mg
from deep_fluids_amd import _lib, ops

SMALL = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((6, 6, 6), 1), ((7, 8, 6), 1), ((9, 10, 7), 2)]


def _name(shape):
    return "x".join(str(n) for n in shape)


@pytest.mark.parametrize("shape,bnd", SMALL, ids=lambda v: _name(v) if isinstance(v, tuple) else str(v))
def test_level0_is_the_matrix_of_the_existing_restatements(shape, bnd):
    rng = np.random.RandomState(7)
    liquid = lmg.geometry("batch3", shape, bnd)
    x = rng.standard_normal(liquid.shape)
    # free surface: liquid_ref.apply_A; integers, so the rows agree to the rounding of the sums
    lev = lmg.level0_liquid(liquid, bnd)
    np.testing.assert_allclose(mg.apply_A(lev, x), lref.apply_A(x, liquid, bnd), rtol=0, atol=1e-13)
    # ghost fluid: liquid_gf_ref.apply_A with its own diagonal; both clamps, every theta branch
    phi = gref.branch_phi(liquid, 11)
    for clamp in gref.GF_CLAMPS:
        lev = lmg.level0_gf(liquid, phi, bnd, clamp)
        want = gref.apply_A(x, liquid, gref.diagonal(phi, liquid, bnd, clamp))
        np.testing.assert_allclose(mg.apply_A(lev, x), want, rtol=0, atol=1e-12 / clamp)
        # ... and diag is the incident weights plus dir, to rounding: the level is a weighted graph Laplacian plus a diagonal
        np.testing.assert_allclose(lev["diag"], np.where(liquid & (mg._with_diag(lev["w"], lev["dir"])["diag"] == 0), 1.0,
                                                          mg._with_diag(lev["w"], lev["dir"])["diag"]), rtol=1e-14)
    # diffusion: diffuse_ref.apply_A on the B*D pairs
    B, D = 2, len(shape)
    alphas = np.array([0.23, 23.0])
    lev = lmg.level0_diffusion(shape, alphas, B, bnd)
    xd = rng.standard_normal((B * D,) + tuple(shape))
    xd = np.where(lmg.interior_mask(shape, bnd)[None], xd, 0.0)            # the direction is 0 off I
    np.testing.assert_allclose(mg.apply_A(lev, xd), dref.apply_A(xd, dref.pair_alpha(alphas, B, D, np.float64), bnd), rtol=0, atol=1e-11)


def test_the_level_sets_of_the_tests_take_every_theta_branch():
    """over the grids of the GPU tests (theta_branches counts with bnd = 1): the fallback, both clamps and ordinary fractions all occur"""
    for clamp in gref.GF_CLAMPS:
        total = np.zeros(4, np.int64)
        for shape, bnd in lmg.GRIDS:
            if bnd == 1:
                liquid = lmg.geometry("batch3", shape, bnd)
                total += np.array(gref.theta_branches(gref.branch_phi(liquid, 11), liquid, clamp))
        assert total.min() > 0, total


@pytest.mark.parametrize("shape,bnd", lmg.GRIDS, ids=lambda v: _name(v) if isinstance(v, tuple) else str(v))
def test_every_interior_cell_liquid_is_the_closed_box_of_the_smoke_block(shape, bnd):
    liquid = lmg.geometry("full", shape, bnd)
    for dtype in (np.float64, np.float32):
        got = lmg.hierarchy_liquid(liquid, bnd, dtype=dtype)
        want = mg.hierarchy(np.zeros(liquid.shape, np.uint8), bnd, 0, dtype)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g["diag"].dtype == np.dtype(dtype)
            for a in range(len(shape)):
                np.testing.assert_array_equal(g["w"][a], w["w"][a])
            np.testing.assert_array_equal(g["dir"], w["dir"])
            np.testing.assert_array_equal(g["diag"], w["diag"])


@pytest.mark.parametrize("shape,bnd", [((6, 7), 1), ((8, 8), 2), ((4, 5, 6), 1)], ids=lambda v: _name(v) if isinstance(v, tuple) else str(v))
def test_M_is_symmetric_positive_semidefinite(shape, bnd):
    liquid = lmg.geometry("batch3", shape, bnd)
    phi = gref.branch_phi(liquid, 5)
    systems = [("gf-%g" % c, lmg.hierarchy_liquid(liquid, bnd, phi.astype(np.float64), c), range(liquid.shape[0])) for c in gref.GF_CLAMPS]
    systems.append(("liquid", lmg.hierarchy_liquid(liquid, bnd), range(liquid.shape[0])))
    systems.append(("diffusion", lmg.hierarchy_diffusion(shape, np.array([0.23, 230.0]), 2, bnd), (0, len(shape))))
    for name, levs, entries in systems:
        for e in entries:
            M = mg.dense_M(levs, e=e)
            scale = np.abs(M).max()
            if scale == 0:
                continue
            assert np.abs(M - M.T).max() <= 1e-12 * scale, name
            assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() >= -1e-12 * scale, name
            # every level is symmetric with a non-negative diagonal surplus: the Galerkin products of a weighted Laplacian plus dir
            for lev in levs:
                A = mg.dense_level(lev, e)
                assert np.abs(A - A.T).max() <= 1e-12 * max(1.0, np.abs(A).max()), name


def _counts(label, plain, multi, broke, out):
    out.append("%-28s plain %4d   mg %3d" % (label, plain, multi))
    assert not broke, label


def test_iteration_counts_of_the_fp32_twin_plain_against_multigrid(capsys):
    """the asserted ratios of the issue on its grids, pool plus drop, fp32, random velocity, max|r| <= 1e-4: multigrid <= plain / 4 for both
    pressure systems, <= plain / 2 for the diffusion at alpha >= 2.3, <= plain below"""
    lines = []
    for shape, bnd in lmg.RATIO_GRIDS:
        liquid = lmg.geometry("pool_drop", shape, bnd)
        vel = lmg.velocity(shape, 1, 3, bnd)
        phi = gref.branch_phi(liquid, 9)
        cases = [("free surface", None, 1e-4), ("ghost fluid 1/theta<=20", phi, 0.05), ("ghost fluid 1/theta<=1e4", phi, 1e-4)]
        for label, ph, clamp in cases:
            kw = dict(phi=ph, bnd=bnd, gf_clamp=clamp, dtype=np.float32, max_iter=4000)
            _, ip, _, bp = lmg.solve_liquid(vel, liquid, precondition=False, **kw)
            _, im, _, bm = lmg.solve_liquid(vel, liquid, **kw)
            _counts("%s %s" % (_name(shape), label), int(ip[0]), int(im[0]), bool(bp.any() or bm.any()), lines)
            assert int(im[0]) * 4 <= int(ip[0]), lines[-1]
        for al in (0.23, 2.3, 23.0, 230.0):
            kw = dict(bnd=bnd, dtype=np.float32, max_iter=4000)
            _, ip, _, bp = lmg.solve_diffusion(vel, al, precondition=False, **kw)
            _, im, _, bm = lmg.solve_diffusion(vel, al, **kw)
            _counts("%s diffusion alpha=%g" % (_name(shape), al), int(ip.max()), int(im.max()), bool(bp.any() or bm.any()), lines)
            assert int(im.max()) * (2 if al >= 2.3 else 1) <= int(ip.max()), lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_multigrid_settings_and_refusals_that_need_no_gpu():
    import torch
    m = ops.Multigrid()
    assert m.alpha == ops.DEFAULT_MG_ALPHA and m.diffusion is True
    assert ops.Multigrid(1.0, diffusion=False).diffusion is False
    for bad in (0.99, 2.0, "1.8", None, True, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ops.Multigrid(bad)
    with pytest.raises(ValueError, match="diffusion"):
        ops.Multigrid(1.5, diffusion=1)
    v = torch.zeros((1, 8, 8, 2))
    d = torch.zeros((1, 8, 8))
    # the string stays the smoke calls'; the refusal names what to pass
    for call in (lambda: ops.solve_pressure_liquid(v, None, preconditioner="mg"), lambda: ops.diffuse_velocity(v, 1.0, preconditioner="mg"),
                 lambda: ops.liquid_step(None, None, v, 0.5, preconditioner="mg"), lambda: ops.simulate_liquid(None, None, v, 2, preconditioner="mg")):
        with pytest.raises(ValueError, match=r"preconditioner.*ops\.Multigrid"):
            call()
    # a Multigrid passes the argument check of every call (and the call then fails on its CPU tensors, not on the preconditioner)
    for call in (lambda: ops.solve_pressure(v, preconditioner=m), lambda: ops.smoke_step(d, v, 0.5, preconditioner=m),
                 lambda: ops.solve_pressure_liquid(v, None, preconditioner=m), lambda: ops.diffuse_velocity(v, 1.0, preconditioner=m)):
        with pytest.raises(Exception) as info:
            call()
        assert "preconditioner" not in str(info.value)
    # a hierarchy of the wrong system is refused before anything is launched
    block = torch.zeros((8,))
    for system, call in (("diffusion", lambda h: ops._hierarchy_for(h, v, 1, None, 0, "solve_pressure")),
                         ("smoke", lambda h: ops._hierarchy_for(h, v, 1, None, 0, "solve_pressure_liquid", "liquid")),
                         ("liquid", lambda h: ops._hierarchy_for(h, v, 1, None, 0, "solve_pressure_liquid", "gf")),
                         ("gf", lambda h: ops._hierarchy_for(h, v, 1, None, 0, "diffuse_velocity", "diffusion", 2))):
        h = ops.MultigridHierarchy(block, (8, 8), 1, 1, 0, 1.8, system)
        assert h.system == system and system in ops.MG_SYSTEMS
        with pytest.raises(ValueError, match="system"):
            call(h)
    assert ops.MultigridHierarchy(block, (8, 8), 1, 1, 0, 1.8).system == "smoke"
    with pytest.raises(ValueError, match="Multigrid"):
        ops.liquid_step(None, None, v, 0.5, preconditioner=ops.MultigridHierarchy(block, (8, 8), 1, 1, 0, 1.8, "liquid"))


def test_the_c_abi_checks_its_arguments_without_a_device():
    h, main = _lib.liquid_mg_lib(), _lib.lib()
    assert sorted(_lib.LIQUID_MG_SIGNATURES) == ["df_diffuse_cg_update_mg", "df_mg_build_diffusion", "df_mg_build_liquid",
                                                 "df_pressure_cg_direction_mg_rows"]
    # a diffusion hierarchy is one of B*D systems
    n = sum(int(np.prod(l["diag"].shape[1:])) for l in lmg.hierarchy_diffusion((12, 10), 1.0, 1, 1))
    hb = main.df_mg_hierarchy_bytes(2, 3 * 2, 1, 12, 10)
    assert hb == 4 * 7 * 6 * n
    buf = ctypes.create_string_buffer(1 << 18)
    a = (ctypes.addressof(buf) + 15) & ~15
    far = a + (1 << 17)

    def err():
        return main.df_last_error()
    assert h.df_mg_build_liquid(None, 0, far, None, 2, 1, 1, 8, 8, 1, 1e-4, None) != 0 and b"hierarchy" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, None, None, 2, 1, 1, 8, 8, 1, 1e-4, None) != 0 and b"null flags" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, far, None, 2, 1, 1, 8, 8, 0, 1e-4, None) != 0 and b"boundary width" in err()
    assert h.df_mg_build_liquid(a, 16, far, None, 2, 1, 1, 8, 8, 1, 1e-4, None) != 0 and b"needed" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, a + 64, None, 2, 1, 1, 8, 8, 1, 1e-4, None) != 0 and b"overlap" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, far, far + 4096, 2, 1, 1, 8, 8, 1, 0.0, None) != 0 and b"gf_clamp" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, far, far + 4097, 2, 1, 1, 8, 8, 1, 1e-4, None) != 0 and b"aligned" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, far, a + 128, 2, 1, 1, 8, 8, 1, 1e-4, None) != 0 and b"level set overlaps" in err()
    assert h.df_mg_build_liquid(a, 1 << 16, far, None, 2, 1, 2, 8, 8, 1, 1e-4, None) != 0 and b"Z = 1" in err()
    assert h.df_mg_build_diffusion(a, 1 << 16, None, 2, 1, 1, 8, 8, 1, None) != 0 and b"null alpha" in err()
    assert h.df_mg_build_diffusion(a, 1 << 16, a + 4, 2, 1, 1, 8, 8, 1, None) != 0 and b"overlaps" in err()
    assert h.df_mg_build_diffusion(a, 4 * 7 * 64, far, 2, 1, 1, 8, 8, 1, None) != 0 and b"needed" in err()      # room for B, not for B*D
    assert h.df_mg_build_diffusion(a, 1 << 16, far, 3, 1 << 23, 8, 8, 8, 1, None) != 0 and b"too large" in err()
    assert h.df_mg_build_diffusion(a, 1 << 16, far, 2, 0, 1, 8, 8, 1, None) != 0 and b"non-positive" in err()
    ws = main.df_pressure_workspace_bytes(1, 1, 8, 8)
    assert h.df_pressure_cg_direction_mg_rows(None, ws, a, 1 << 16, 2, 1, 1, 8, 8, 0, 1e-4, 10, None) != 0 and b"null workspace" in err()
    assert h.df_pressure_cg_direction_mg_rows(far, ws - 4, a, 1 << 16, 2, 1, 1, 8, 8, 0, 1e-4, 10, None) != 0 and b"needed" in err()
    assert h.df_pressure_cg_direction_mg_rows(a + 256, ws, a, 1 << 16, 2, 1, 1, 8, 8, 0, 1e-4, 10, None) != 0 and b"overlaps the hierarchy" in err()
    assert h.df_pressure_cg_direction_mg_rows(far, ws, a, 1 << 16, 2, 1, 1, 8, 8, -1, 1e-4, 10, None) != 0 and b"iteration" in err()
    assert h.df_pressure_cg_direction_mg_rows(far, ws, a, 1 << 16, 2, 1, 1, 8, 8, 0, -1.0, 10, None) != 0 and b"accuracy" in err()
    dws = main.df_diffuse_workspace_bytes(1, 1, 8, 8, 2)
    assert h.df_diffuse_cg_update_mg(far, dws - 4, 2, 1, 1, 8, 8, 1, 0, None) != 0 and b"needed" in err()
    assert h.df_diffuse_cg_update_mg(far, dws, 2, 1, 1, 8, 8, 1, -1, None) != 0 and b"iteration" in err()
    assert h.df_diffuse_cg_update_mg(far, dws, 2, 1, 1, 8, 8, 4, 0, None) != 0 and b"2*bnd + 2" in err()
    assert h.df_diffuse_cg_update_mg(None, dws, 2, 1, 1, 8, 8, 1, 0, None) != 0 and b"null workspace" in err()
