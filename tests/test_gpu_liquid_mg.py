"""GPU side of the multigrid preconditioner for the liquid systems (liquid_mg.hip; ops.Multigrid, ops.multigrid_hierarchy_liquid /
_diffusion, the ``preconditioner=`` of the liquid calls) against tests/liquid_mg_ref.py: the hierarchies and the V-cycle bit for bit
against the fp32 twin, the iteration against the fp64 recurrence within 4x the twin's own deviation, the full solves held to the bounds
the plain solves are held to in test_gpu_liquid.py / test_gpu_liquid_gf.py / test_gpu_diffuse.py.  Every parity test prints its figures
before it asserts.

Grids (liquid_mg_ref.GRIDS): the smallest where odd extents, bnd 2, more than one workgroup, one and two launched levels above the
one-workgroup kernel (34x66; 66x70 and 18x22x26, whose level 1 has more than 1024 cells and odd extents) can go wrong."""
import os

import numpy as np
import pytest
import torch

import cg_ref
import diffuse_ref as dref
import liquid_gf_ref as gref
import liquid_mg_ref as lmg
import liquid_ref as lref
import liquid_resample_ref as rr
from gpu_util import assert_bits, dev

pytestmark = pytest.mark.gpu

ACC = 1e-4
CLAMP = 1e-4
ORDERED = dict(dot=cg_ref.ordered_dot, amax=cg_ref.ordered_amax)
IDS = ["x".join(str(n) for n in s) + ("-bnd%d" % b if b != 1 else "") for s, b in lmg.GRIDS]


def _np(t):
    return t.cpu().numpy()


def _flags(liquid):
    return torch.from_numpy(np.ascontiguousarray(lref.flags_of(liquid)[0])).cuda()


def _cases(shape, bnd):
    """the liquid of every geometry in one batch (pool plus drop, full, isolated cell and blob, none), its phi and a velocity"""
    liquid = np.concatenate([lmg.geometry("batch3", shape, bnd), lmg.geometry("none", shape, bnd)])
    return liquid, gref.branch_phi(liquid, 11), lmg.velocity(shape, liquid.shape[0], 5, bnd)


def _assert_levels(h, levs, what):
    assert h.levels == len(levs)
    for l, lev in enumerate(levs):
        w, d, dg = h.weights(l)
        for a in range(len(w)):
            assert_bits(_np(w[a]), lev["w"][a], "%s level %d w_%d" % (what, l, a))
        assert_bits(_np(d), lev["dir"], "%s level %d dir" % (what, l))
        assert_bits(_np(dg), lev["diag"], "%s level %d diag" % (what, l))


def _systems(ops, shape, bnd):
    """(name, hierarchy, fp32 twin levels, fp64 levels) of the three systems on a grid"""
    liquid, phi, vel = _cases(shape, bnd)
    fl = _flags(liquid)
    B = liquid.shape[0]
    yield ("liquid", ops.multigrid_hierarchy_liquid(shape, fl, bnd), lmg.hierarchy_liquid(liquid, bnd, dtype=np.float32),
           lmg.hierarchy_liquid(liquid, bnd))
    yield ("gf", ops.multigrid_hierarchy_liquid(dev(vel), fl, bnd, phi=dev(phi), gf_clamp=CLAMP),
           lmg.hierarchy_liquid(liquid, bnd, phi, CLAMP, np.float32), lmg.hierarchy_liquid(liquid, bnd, phi.astype(np.float64), CLAMP))
    al = np.array(lmg.DIFFUSION_ALPHAS)
    yield ("diffusion", ops.multigrid_hierarchy_diffusion(dev(vel), al, bnd), lmg.hierarchy_diffusion(shape, al, B, bnd, np.float32),
           lmg.hierarchy_diffusion(shape, al, B, bnd))


# ---- 1. the hierarchies and the bare V-cycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", lmg.GRIDS, ids=IDS)
def test_hierarchy_and_cycle_are_bitwise_the_fp32_twin(shape, bnd):
    from deep_fluids_amd import ops
    nd = len(shape)
    rng = np.random.RandomState(7)
    for name, h, l32, l64 in _systems(ops, shape, bnd):
        assert h.system == name and h.batch == l32[0]["diag"].shape[0]
        _assert_levels(h, l32, "%s %s" % (shape, name))
        r = rng.standard_normal(l32[0]["diag"].shape).astype(np.float32)           # non-zero on air, band and wall cells too
        for l in range(h.levels):                                                  # nothing is read before it is written
            for a in (nd + 2, nd + 3, nd + 4):
                h._array(l, a).fill_(float("nan"))
        z = _np(ops.multigrid_apply(h, dev(r))).copy()
        z32 = lmg.vcycle(l32, r, h.alpha)
        z64 = lmg.vcycle(l64, r.astype(np.float64), h.alpha)
        e32, eg = float(np.abs(z32 - z64).max()), float(np.abs(z - z64).max())
        print("%s bnd %d %s: twin - fp64 %.3e  gpu - fp64 %.3e  |z| %.3e" % (shape, bnd, name, e32, eg, float(np.abs(z64).max())))
        assert_bits(z, z32, "%s %s: z" % (shape, name))
        assert not z[l32[0]["diag"] == 0].any()                                    # 0 on inactive cells
        if name != "diffusion":
            assert not z[-1].any()                                                 # the entry without liquid
            assert (l32[0]["diag"][-1] == 0).all()
    # with every interior cell liquid the free-surface hierarchy is the closed box of the smoke block
    full = lmg.geometry("full", shape, bnd)
    hs, hl = ops.multigrid_hierarchy(shape, bnd, batch=1), ops.multigrid_hierarchy_liquid(shape, _flags(full), bnd)
    assert hs.system == "smoke"
    for l in range(hs.levels):
        (w0, d0, g0), (w1, d1, g1) = hs.weights(l), hl.weights(l)
        assert all(torch.equal(a, b) for a, b in zip(w0, w1)) and torch.equal(d0, d1) and torch.equal(g0, g1)


@pytest.mark.parametrize("shape,bnd", [lmg.GRIDS[2], lmg.GRIDS[4], lmg.GRIDS[8]], ids=[IDS[2], IDS[4], IDS[8]])
def test_rebuilding_in_place_is_bitwise_a_fresh_build(shape, bnd):
    from deep_fluids_amd import ops
    liquid, phi, vel = _cases(shape, bnd)
    other = np.ascontiguousarray(liquid[::-1])
    for kw_a, kw_b in ((dict(), dict()), (dict(phi=dev(phi), gf_clamp=CLAMP), dict(phi=dev(np.ascontiguousarray(phi[::-1])), gf_clamp=1e-2))):
        fresh = ops.multigrid_hierarchy_liquid(shape, _flags(liquid), bnd, **kw_a)
        h = ops.multigrid_hierarchy_liquid(shape, _flags(other), bnd, alpha=1.2, **kw_b)
        ptr = h.block.data_ptr()
        again = ops.multigrid_hierarchy_liquid(shape, _flags(liquid), bnd, out=h, **kw_a)
        assert again is h and h.block.data_ptr() == ptr and h.alpha == ops.DEFAULT_MG_ALPHA
        for l in range(h.levels):
            (w0, d0, g0), (w1, d1, g1) = fresh.weights(l), h.weights(l)
            assert all(torch.equal(a, b) for a, b in zip(w0, w1)) and torch.equal(d0, d1) and torch.equal(g0, g1)
    fresh = ops.multigrid_hierarchy_diffusion(dev(vel), np.array(lmg.DIFFUSION_ALPHAS), bnd)
    h = ops.multigrid_hierarchy_diffusion(dev(vel), 3.0, bnd)
    assert ops.multigrid_hierarchy_diffusion(dev(vel), np.array(lmg.DIFFUSION_ALPHAS), bnd, out=h) is h
    for l in range(h.levels):
        (w0, d0, g0), (w1, d1, g1) = fresh.weights(l), h.weights(l)
        assert all(torch.equal(a, b) for a, b in zip(w0, w1)) and torch.equal(d0, d1) and torch.equal(g0, g1)
    with pytest.raises(ValueError, match="out must be"):
        ops.multigrid_hierarchy_liquid(shape, _flags(liquid), bnd, out=fresh)          # a diffusion hierarchy
    with pytest.raises(ValueError, match="system"):
        ops.solve_pressure_liquid(dev(vel), _flags(liquid), bnd=bnd, preconditioner=fresh)
    with pytest.raises(ValueError, match="system"):
        ops.diffuse_velocity(dev(vel), 1.0, bnd=bnd, preconditioner=ops.multigrid_hierarchy_liquid(shape, _flags(liquid), bnd))


# ---- 2. K iterations against the fp64 recurrence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", lmg.GRIDS, ids=IDS)
def test_k_iterations_against_the_fp64_recurrence(shape, bnd):
    """the project's rule: the GPU's deviation from the fp64 recurrence is within 4x the fp32 twin's own"""
    from deep_fluids_amd import ops
    liquid, phi, vel = _cases(shape, bnd)
    fl, m = _flags(liquid), ops.Multigrid()
    live = liquid.reshape(liquid.shape[0], -1).any(axis=1)
    al = np.array(lmg.DIFFUSION_ALPHAS)
    for k in (1, 2, 3):
        for name, ph in (("liquid", None), ("gf", phi)):
            kw = dict(phi=ph, bnd=bnd, gf_clamp=CLAMP, accuracy=0.0, max_iter=k)
            x64, it64, _, _ = lmg.solve_liquid(vel, liquid, dtype=np.float64, **kw)
            x32, it32, _, _ = lmg.solve_liquid(vel, liquid, dtype=np.float32, **ORDERED, **kw)
            _, p, iters = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, accuracy=0.0, max_iter=k, preconditioner=m,
                                                    **(dict(phi=dev(ph), gf_clamp=CLAMP) if ph is not None else {}))
            e32, err = float(np.abs(x32 - x64).max()), float(np.abs(_np(p) - x64).max())
            print("%s bnd %d %s k %d: twin %.3e  gpu %.3e (bound %.3e)  |x| %.3e  gpu - twin %.3e" %
                  (shape, bnd, name, k, e32, err, 4 * e32, float(np.abs(x64).max()), float(np.abs(_np(p) - x32).max())))
            # k iterations, or fewer where a system of a few cells is solved exactly before that (r.z = 0), as in the twin
            it = _np(iters)
            assert (it == it32).all() and (it[live] >= 1).all() and (it <= k).all() and (it64 <= k).all() and (it[~live] == 0).all()
            assert it.max() == k
            assert err <= 4 * e32
        x64, it64, _, _ = lmg.solve_diffusion(vel, al, bnd, 0.0, k, np.float64)
        x32, it32, _, _ = lmg.solve_diffusion(vel, al, bnd, 0.0, k, np.float32, **ORDERED)
        got, iters = ops.diffuse_velocity(dev(vel), al, bnd=bnd, accuracy=0.0, max_iter=k, preconditioner=m)
        e32, err = float(np.abs(x32 - x64).max()), float(np.abs(_np(got) - x64).max())
        print("%s bnd %d diffusion k %d: twin %.3e  gpu %.3e (bound %.3e)  gpu - twin %.3e" % (shape, bnd, k, e32, err, 4 * e32,
                                                                                                  float(np.abs(_np(got) - x32).max())))
        it = _np(iters)
        assert (it == it32).all() and (it[1:] >= 1).all() and (it <= k).all() and (it64 <= k).all() and (it[0] == 0).all()   # alpha = 0: no iteration
        assert it.max() == k
        assert_bits(_np(got)[0], vel[0], "alpha = 0 returns the input's bits")
        assert err <= 4 * e32


# ---- 3. the full solves ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", lmg.GRIDS, ids=IDS)
def test_pressure_solves_residual_projection_and_iterations(shape, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    liquid, phi, vel = _cases(shape, bnd)
    fl, m = _flags(liquid), ops.Multigrid()
    live = liquid.reshape(liquid.shape[0], -1).any(axis=1)
    max_iter = ops.default_max_iter(shape)
    b64 = lref.rhs(vel, liquid, np.float64)
    small = int(liquid.reshape(liquid.shape[0], -1).sum(axis=1).max()) <= 1200
    for name, ph in (("liquid", None), ("gf", phi)):
        gkw = dict(phi=dev(ph), gf_clamp=CLAMP) if ph is not None else {}
        v, p, iters = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, accuracy=ACC, preconditioner=m, **gkw)
        _, _, plain = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, accuracy=ACC, **gkw)
        x32, it32, r32, broke = lmg.solve_liquid(vel, liquid, ph, bnd, ACC, max_iter, CLAMP, np.float32, **ORDERED)
        if ph is None:
            A = lambda x: lref.apply_A(x, liquid, bnd)                                                    # noqa: E731
        else:
            dg = gref.diagonal(ph, liquid, bnd, CLAMP, np.float64)
            A = lambda x: gref.apply_A(x, liquid, dg)                                                     # noqa: E731
        excess = float(np.abs((b64 - A(x32.astype(np.float64))) - r32).max())
        res = float(np.abs(b64 - A(_np(p).astype(np.float64))).max())
        it = _np(iters)
        print("%s bnd %d %s: iterations gpu %s twin %s plain %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
              (shape, bnd, name, it.tolist(), it32.tolist(), _np(plain).tolist(), res, ACC, excess))
        assert not broke.any()
        assert (it[live] > 0).all() and (it < max_iter).all() and (it[~live] == 0).all()
        assert res <= ACC + excess
        assert (np.abs(it - it32) <= 2).all()
        if shape in ((66, 70), (18, 22, 26)):                                      # pool plus drop, where the host test sets its bar
            assert it[0] * 4 <= _np(plain)[0] if ph is None else it[0] < _np(plain)[0]      # (the ghost fluid's plain arm is Jacobi's)
        assert not _np(p)[~liquid].any()
        if small:
            if ph is None:
                vex, _ = lref.exact_projection(vel, liquid, bnd)
                v32 = lref.correct(vel, x32, liquid, bnd, np.float32)
            else:
                vex, _ = gref.exact_projection(vel, liquid, ph, bnd, CLAMP)
                v32 = gref.correct(vel, x32, liquid, ph, bnd, CLAMP, np.float32)
            d32, dg_ = float(np.abs(v32 - vex).max()), float(np.abs(_np(v) - vex).max())
            print("%s bnd %d %s: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (shape, bnd, name, d32, dg_))
            assert dg_ <= 3 * d32


@pytest.mark.parametrize("shape,bnd", lmg.GRIDS, ids=IDS)
def test_diffusion_solve_residual_dense_solution_and_iterations(shape, bnd):
    from deep_fluids_amd import ops
    liquid, _, vel = _cases(shape, bnd)
    al = np.array(lmg.DIFFUSION_ALPHAS)
    cap = 400
    got, iters = ops.diffuse_velocity(dev(vel), al, bnd=bnd, accuracy=ACC, max_iter=cap, preconditioner=ops.Multigrid())
    _, plain = ops.diffuse_velocity(dev(vel), al, bnd=bnd, accuracy=ACC, max_iter=cap)
    x32, it32, r32, broke = lmg.solve_diffusion(vel, al, bnd, ACC, cap, np.float32, **ORDERED)
    excess = float(np.abs(dref.residual(x32, vel, al, bnd) - r32).max())
    res = float(np.abs(dref.residual(_np(got), vel, al, bnd)).max())
    it = _np(iters)
    print("%s bnd %d diffusion: iterations gpu %s twin %s plain %s  fp64 residual %.4e (bound %.1e + twin's excess %.3e)" %
          (shape, bnd, it.tolist(), it32.tolist(), _np(plain).tolist(), res, ACC, excess))
    assert not broke.any() and iters.dtype == torch.int32 and tuple(iters.shape) == (4, len(shape))
    assert (it[0] == 0).all() and (it[1:] > 0).all() and (it < cap).all()
    assert res <= ACC + excess
    assert (np.abs(it - it32) <= 2).all()
    if shape in ((34, 66), (66, 70), (18, 22, 26)):
        assert (it[2:] * 2 <= _np(plain)[2:]).all()                                  # alpha 23 and 230: the host test's bar, on the device
    inter = lmg.interior_mask(shape, bnd)
    assert_bits(_np(got)[:, ~inter], vel[:, ~inter], "the band is copied through")
    if int(inter.sum()) <= 1500:
        exact = dref.dense(vel, al, bnd)
        d32, dg = float(np.abs(x32 - exact).max()), float(np.abs(_np(got) - exact).max())
        print("%s bnd %d diffusion: distance from the dense fp64 solution: twin %.3e  gpu %.3e" % (shape, bnd, d32, dg))
        assert dg <= 3 * d32


# ---- 4. invariance -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", [lmg.GRIDS[1], lmg.GRIDS[3], lmg.GRIDS[7]], ids=[IDS[1], IDS[3], IDS[7]])
def test_determinism_batch_invariance_check_every_and_reuse(shape, bnd):
    from deep_fluids_amd import ops
    liquid, phi, vel = _cases(shape, bnd)
    fl, m = _flags(liquid), ops.Multigrid()
    for ph in (None, phi):
        gkw = (lambda e=slice(None): dict(phi=dev(ph[e]), gf_clamp=CLAMP)) if ph is not None else (lambda e=None: {})
        v, p, iters = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, preconditioner=m, **gkw())
        v2, p2, i2 = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, preconditioner=m, **gkw())
        assert torch.equal(p, p2) and torch.equal(v, v2) and torch.equal(iters, i2)                        # two calls, the same bits
        for e in range(liquid.shape[0]):                                                                   # an entry does not depend on its batch
            ve, pe, ie = ops.solve_pressure_liquid(dev(vel[e:e + 1]), fl[e:e + 1].contiguous(), bnd=bnd, preconditioner=m, **gkw(slice(e, e + 1)))
            assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
            assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
            assert int(ie[0]) == int(iters[e])
        h = ops.multigrid_hierarchy_liquid(dev(vel), fl, bnd, **gkw())
        ws = ops.pressure_workspace(dev(vel), ghost_fluid=ph is not None)
        ws.fill_(float("nan"))                                                                             # nothing is read before it is written
        for ce in (None, 1, 16, 64):
            v3, p3, i3 = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, check_every=ce, workspace=ws, preconditioner=h, **gkw())   # and reused
            assert torch.equal(p3, p) and torch.equal(v3, v) and torch.equal(i3, iters), "check_every %s" % ce
        vi = dev(vel)
        assert ops.solve_pressure_liquid(vi, fl, bnd=bnd, out=vi, preconditioner=h, **gkw())[0] is vi and torch.equal(vi, v)        # in place
    al = np.array(lmg.DIFFUSION_ALPHAS)
    got, iters = ops.diffuse_velocity(dev(vel), al, bnd=bnd, preconditioner=m)
    g2, i2 = ops.diffuse_velocity(dev(vel), al, bnd=bnd, preconditioner=m)
    assert torch.equal(got, g2) and torch.equal(iters, i2)
    for e in range(4):
        ge, ie = ops.diffuse_velocity(dev(vel[e:e + 1]), al[e:e + 1], bnd=bnd, preconditioner=m)
        assert_bits(_np(ge)[0], _np(got)[e], "diffusion of entry %d alone" % e)
        assert torch.equal(ie[0], iters[e])
    h = ops.multigrid_hierarchy_diffusion(dev(vel), al, bnd)
    ws = ops.diffusion_workspace(dev(vel))
    ws.fill_(float("nan"))
    for ce in (None, 1, 16):
        g3, i3 = ops.diffuse_velocity(dev(vel), al, bnd=bnd, check_every=ce, workspace=ws, preconditioner=h)
        assert torch.equal(g3, got) and torch.equal(i3, iters), "check_every %s" % ce
    vi = dev(vel)
    assert ops.diffuse_velocity(vi, al, bnd=bnd, out=vi, preconditioner=h)[0] is vi and torch.equal(vi, got)


def test_an_entry_that_converges_early_is_frozen():
    from deep_fluids_amd import ops
    shape, bnd = (34, 66), 1
    liquid = np.repeat(lmg.geometry("pool_drop", shape, bnd), 2, axis=0)
    vel = np.repeat(lmg.velocity(shape, 1, 5, bnd), 2, axis=0)
    vel[1] *= np.float32(1e-3)                                 # entry 1 starts nearer the accuracy and stops first
    fl, m = _flags(liquid), ops.Multigrid()
    for gkw in ({}, dict(phi=dev(gref.branch_phi(liquid, 11)), gf_clamp=CLAMP)):
        _, p, iters = ops.solve_pressure_liquid(dev(vel), fl, bnd=bnd, preconditioner=m, **gkw)
        it = _np(iters)
        assert 0 < it[1] < it[0]
        one = {k: (t[1:2].contiguous() if isinstance(t, torch.Tensor) else t) for k, t in gkw.items()}
        _, p1, i1 = ops.solve_pressure_liquid(dev(vel[1:2]), fl[1:2].contiguous(), bnd=bnd, preconditioner=m, **one)
        assert_bits(_np(p1)[0], _np(p)[1], "the early entry")
        assert int(i1[0]) == it[1]
    got, iters = ops.diffuse_velocity(dev(vel), np.array([23.0, 23.0]), bnd=bnd, preconditioner=m)
    g1, i1 = ops.diffuse_velocity(dev(vel[1:2]), 23.0, bnd=bnd, preconditioner=m)
    assert (_np(iters)[1] < _np(iters)[0]).all() and torch.equal(i1[0], iters[1])
    assert_bits(_np(g1)[0], _np(got)[1], "the early entry's diffusion")


# ---- 5. preconditioner=None is the call without the keyword; the steps ---------------------------------------------------------------------
def _variants(ops):
    return [("plain", dict()), ("ghost_fluid", dict(ghost_fluid=True)), ("viscosity", dict(viscosity_alpha=[2.3, 23.0])),
            ("resample", dict(resample=lambda: ops.Resample(2)))]


def _kw(kw):
    return {k: (v() if callable(v) else v) for k, v in kw.items()}


def test_preconditioner_none_is_bitwise_the_call_without_the_keyword():
    from deep_fluids_amd import ops
    from test_gpu_liquid import STEP_SEEDS, drop_scene
    shape, bnd = (9, 7), 1
    liquid, phi, vel = _cases(shape, bnd)
    fl = _flags(liquid)
    for gkw in ({}, dict(phi=dev(phi), gf_clamp=CLAMP)):
        a, b = ops.solve_pressure_liquid(dev(vel), fl, **gkw), ops.solve_pressure_liquid(dev(vel), fl, preconditioner=None, **gkw)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = ops.diffuse_velocity(dev(vel), 2.3), ops.diffuse_velocity(dev(vel), 2.3, preconditioner=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    shape = (12, 16)
    pos0, vel0 = drop_scene(shape, STEP_SEEDS[shape])
    p, v = dev(pos0), dev(vel0)
    u = ops.sample_velocity(v, p)
    for name, kw in _variants(ops):
        a, b = ops.liquid_step(p, u, v, 0.5, **_kw(kw)), ops.liquid_step(p, u, v, 0.5, preconditioner=None, **_kw(kw))
        if name == "resample":                                  # ragged storage: the rows past entry_start[-1] are never written
            live = int(a[-1][-1])
            a, b = (a[0][:live], a[1][:live]) + a[2:], (b[0][:live], b[1][:live]) + b[2:]
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), name
    a, b = ops.simulate_liquid(p, u, v, 3, dt=0.5), ops.simulate_liquid(p, u, v, 3, dt=0.5, preconditioner=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


STEP_VARIANTS = ["plain", "ghost_fluid", "viscosity", "viscosity-converged"]


@pytest.mark.parametrize("variant", STEP_VARIANTS)
@pytest.mark.parametrize("shape", [(12, 16), (8, 10, 8)], ids=["12x16", "8x10x8"])
def test_four_steps_with_multigrid_against_the_fp64_step(shape, variant):
    """Both arms, chained step by step, against the fp64 step: vel, pos and pvel held to the bound of
    test_four_steps_of_a_drop_falling_into_a_basin (and its ghost-fluid and viscous twins) -- margin 3 over the fp32 restatement's own
    error plus the two solves' accuracy -- after the identity that bound rests on: the same particles in the same cells in fp32, in fp64
    and in both arms.
    The viscous alphas.  The fp64 step runs the PLAIN recurrence under the diffusion's own iteration cap (max(extent) in 3-D: 10 here), so
    it is a yardstick for another recurrence only where it has converged under that cap.  With kappa <= 1 + 4 D alpha and the CG rate
    (sqrt(kappa) - 1) / (sqrt(kappa) + 1), ten iterations reach 1e-9 for alpha <= 0.046 (rate 0.1) and not for 0.23 (rate 0.32):
    ``viscosity`` in 3-D takes (0.023, 0.046), the scene's own smallest alpha and twice it, and holds both arms; in 2-D the cap is
    4 * 16 = 64 and (2.3, 23) converge.  ``viscosity-converged`` holds the multigrid arm at alphas where the capped plain solve stops
    short -- (0.23, 0.46) in 3-D: the twin's plain solve needs 11 and more iterations at 0.23, its preconditioned one 6 -- to the step of
    liquid_mg_ref.viscous_step, whose diffusion runs to convergence (cap 400), and asserts that the multigrid diffusion ended below
    its cap; the plain arm is not compared there: it is the truncated one.
    Measured on the MI355X, 8x10x8 at (2.3, 23) against the capped fp64 step: plain arm 5.2e-07, multigrid arm 6.3e-03 (bound 2.2e-05):
    the cap's truncation, reported in profiles/liquid_mg.md."""
    from deep_fluids_amd import ops
    from test_gpu_liquid import STEP_SEEDS, drop_scene
    D = len(shape)
    pos0, vel0 = drop_scene(shape, STEP_SEEDS[shape])
    dt, tight, T = 0.5, 1e-6, 4
    pvel0 = lref.sample(vel0, pos0, np.float32)
    arms = [("plain", None), ("mg", ops.Multigrid())]
    cap = ops.default_diffusion_max_iter(shape)
    if variant == "plain":
        step, kw = (lambda s, acc, dtype: lref.step(s["pos"], s["pvel"], s["vel"], dt, accuracy=acc, dtype=dtype)), dict()
    elif variant == "ghost_fluid":
        step, kw = (lambda s, acc, dtype: gref.step(s["pos"], s["pvel"], s["vel"], dt, accuracy=acc, dtype=dtype)), dict(ghost_fluid=True)
    elif variant == "viscosity":
        alphas = [2.3, 23.0] if D == 2 else [0.023, 0.046]
        step = lambda s, acc, dtype: dref.step(s["pos"], s["pvel"], s["vel"], dt, alphas, accuracy=acc, dtype=dtype)      # noqa: E731
        kw = dict(viscosity_alpha=alphas)
    else:
        alphas = [2.3, 23.0] if D == 2 else [0.23, 0.46]
        step = lambda s, acc, dtype: lmg.viscous_step(s["pos"], s["pvel"], s["vel"], dt, alphas, 400, accuracy=acc, dtype=dtype)      # noqa: E731
        kw = dict(viscosity_alpha=alphas)
        arms = arms[1:]
    state = {name: (dev(pos0), ops.sample_velocity(dev(vel0), dev(pos0)), dev(vel0)) for name, _ in arms}
    total = {name: 0 for name, _ in arms}
    s64 = dict(pos=pos0.astype(np.float64), pvel=pvel0.astype(np.float64), vel=vel0.astype(np.float64))
    s32 = dict(pos=pos0, pvel=pvel0, vel=vel0)
    for t in range(T):
        s64, s32 = step(s64, tight * 1e-3, np.float64), step(s32, tight, np.float32)
        s64, s32 = (s64[0] if isinstance(s64, tuple) else s64), (s32[0] if isinstance(s32, tuple) else s32)
        np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
        assert (s32["liquid"] == s64["liquid"]).all()
        e32 = [lref.max_err(s32[k], s64[k]) for k in ("vel", "pos", "pvel")]
        for name, pre in arms:
            out = ops.liquid_step(*state[name], dt, accuracy=tight, preconditioner=pre, **kw)
            p, u, v, iters = out[:4]
            state[name] = (p, u, v)
            total[name] += int(iters.sum())
            _, gcs, _ = ops.particle_cells(p, shape)
            np.testing.assert_array_equal(_np(gcs), s64["cell_start"])          # the same particles in the same cells
            eg = [lref.max_err(_np(x), s64[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
            print("%s %s step %d %s arm: iterations %s%s  vel/pos/pvel twin-vs-fp64 %.3e %.3e %.3e  gpu-vs-fp64 %.3e %.3e %.3e" %
                  ((shape, variant, t + 1, name, _np(iters).tolist(), "" if len(out) == 4 else " diffusion %s" % _np(out[4]).tolist())
                   + tuple(e32) + tuple(eg)))
            for k in range(3):
                assert eg[k] <= 3 * e32[k] + 2 * tight * max(shape), (name, k, eg[k], e32[k])
            if variant == "viscosity-converged":
                assert (_np(out[4]) < cap).all()                               # the preconditioned diffusion converged under the cap
    if len(arms) == 2:
        assert total["mg"] < total["plain"]                                    # the lower iteration counts


@pytest.mark.parametrize("case", rr.STEP_CASES, ids=lambda c: c[0])
def test_chained_steps_with_resample_and_multigrid(case):
    """test_gpu_liquid_resample.test_three_chained_steps_with_resample for both arms: ragged storage, entry_start handed back in, with and
    without ghost fluid and viscosity, every step against liquid_resample_ref.step in fp64 and fp32 from the arm's own state; vel and
    pvel held to that test's bound, after the identities it rests on (entry_start and the cell ranges, bit for bit)."""
    from deep_fluids_amd import ops
    from test_liquid_resample_host import initial_step_state
    name, shape, gf, alpha = case
    minp = rr.STEP_MIN_P[len(shape)]
    pos0, pvel0, es0, vel0 = initial_step_state(shape)
    P = len(pos0)
    parts = [pos0[es0[b]:es0[b + 1]] for b in range(rr.B)]
    kw = dict(accuracy=rr.STEP_ACC, ghost_fluid=gf)
    if alpha is not None:
        kw["viscosity_alpha"] = list(alpha)
    tight = rr.STEP_ACC
    total = {}
    for arm, pre in (("plain", None), ("mg", ops.Multigrid())):
        gp, ges = ops.pack_particles([dev(q) for q in parts], capacity=P)
        gv = dev(vel0)
        gu = ops.sample_velocity(gv, gp, entry_start=ges)
        rs = ops.Resample(minp)
        total[arm] = 0
        for t in range(rr.STEP_T):
            st = (_np(gp), _np(gu), _np(ges), _np(gv))
            rk = dict(ghost_fluid=gf, alpha=None if alpha is None else np.asarray(alpha), step_no=t)
            s32 = rr.step(*st, rr.STEP_DT, minp, accuracy=tight, dtype=np.float32, **rk)
            s64 = rr.step(*st, rr.STEP_DT, minp, accuracy=tight * 1e-3, dtype=np.float64, **rk)
            out = ops.liquid_step(gp, gu, gv, rr.STEP_DT, resample=rs, entry_start=ges, preconditioner=pre, **kw)
            assert len(out) == (6 if alpha is not None else 5) and rs.step == t + 1
            gp, gu, gv, iters, ges = out[0], out[1], out[2], out[3], out[-1]
            total[arm] += int(iters.sum())
            live = s32["total"]
            np.testing.assert_array_equal(_np(ges), s32["entry_start"])
            np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
            _, gcs, _ = ops.particle_cells(gp, shape, entry_start=ges)
            np.testing.assert_array_equal(_np(gcs), s32["cell_start"])
            e32 = [lref.max_err(s32[k], s64[k]) for k in ("vel", "pvel")]
            eg = [lref.max_err(_np(gv), s64["vel"]), lref.max_err(_np(gu)[:live], s64["pvel"])]
            print("%s step %d %s arm: iterations %s  live %d  vel/pvel twin-vs-fp64 %.3e %.3e  gpu-vs-fp64 %.3e %.3e" %
                  ((name, t + 1, arm, _np(iters).tolist(), live) + tuple(e32) + tuple(eg)))
            for k in range(2):
                assert eg[k] <= 3 * e32[k] + 2 * tight * max(shape), (arm, k, eg[k], e32[k])
    assert total["mg"] < total["plain"]


def test_a_generator_with_multigrid_writes_the_same_files(tmp_path):
    from deep_fluids_amd import data, ops
    kw = dict(num_src_x_pos=2, num_src_radius=1, num_frames=3, resolution_x=16, resolution_y=12, device="cuda")
    a, b = str(tmp_path / "plain"), str(tmp_path / "mg")
    na = data.generate_liquid_dataset(a, **kw)
    nb = data.generate_liquid_dataset(b, preconditioner=ops.Multigrid(), **kw)
    assert na == nb == 6
    assert sorted(os.listdir(os.path.join(a, "v"))) == sorted(os.listdir(os.path.join(b, "v")))
    keys = [[line.split(":")[0] for line in open(os.path.join(r, "args.txt"))] for r in (a, b)]
    assert keys[0] == keys[1] and "preconditioner" not in keys[1]
    worst = 0.0
    for f in os.listdir(os.path.join(a, "v")):
        xa, xb = np.load(os.path.join(a, "v", f)), np.load(os.path.join(b, "v", f))
        assert xa["x"].shape == xb["x"].shape and (xa["y"] == xb["y"]).all()
        worst = max(worst, float(np.abs(xa["x"] - xb["x"]).max()))
    print("generator: max difference between the arms' frames %.3e" % worst)
