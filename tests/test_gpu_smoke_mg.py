"""GPU side of the multigrid preconditioner of the smoke pressure solve (multigrid.hip, ops.multigrid_hierarchy / multigrid_apply, the
``preconditioner=`` keyword): against tests/smoke_mg_ref.py -- the hierarchy and the V-cycle bit for bit against the fp32 twin, the
iteration against the fp64 recurrence with tolerances measured from the twin in the same test.  Every parity test prints its figures
before it asserts.

Shapes are SOLVE_SHAPES of test_gpu_smoke_obstacles.py and 33x20x18 (odd at two levels): the smallest where odd extents, a 256-cell
workgroup boundary, bnd 2, split regions, enclosed cells and all-solid entries can go wrong."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import smoke_mg_ref as mg
import smoke_obs_ref as oref
import smoke_open_ref as pref
from gpu_util import assert_bits, dev

pytestmark = pytest.mark.gpu

SHAPES = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((17, 130), 1), ((6, 6, 6), 1), ((7, 8, 6), 1), ((19, 10, 7), 2), ((33, 20, 18), 1)]
ACC = 1e-4


def _np(t):
    return t.cpu().numpy()


def _obs(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _all_obstacles(shape, bnd):
    c = oref.obstacle_cases(shape, bnd)
    names = sorted(c)
    return names, np.stack([c[n] for n in names])


def _one_open(nd):
    return pref.sides("XyY", nd)


# ---- 1. the hierarchy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_hierarchy_is_bitwise_the_restatement(shape, bnd):
    from deep_fluids_amd import ops
    nd = len(shape)
    names, obs = _all_obstacles(shape, bnd)
    for spec, bits in pref.specs(nd):
        h = ops.multigrid_hierarchy(shape, bnd, obstacle=_obs(obs), open_bound=bits, batch=len(names))
        levs = mg.hierarchy(obs, bnd, bits, np.float32)
        assert h.levels == len(levs) and h.level_shape(h.levels - 1) == levs[-1]["diag"].shape[1:] and max(h.level_shape(h.levels - 1)) <= 2
        for l, lev in enumerate(levs):
            w, d, dg = h.weights(l)
            for a in range(nd):
                assert_bits(_np(w[a]), lev["w"][a], "%s open %r level %d w_%d" % (shape, spec, l, a))
            assert_bits(_np(d), lev["dir"], "%s open %r level %d dir" % (shape, spec, l))
            assert_bits(_np(dg), lev["diag"], "%s open %r level %d diag" % (shape, spec, l))
    # no obstacle at all (the index tests instead of the flags byte) gives the weights of an all-zero obstacle
    zero = np.zeros((2,) + shape, np.uint8)
    h0, h1 = ops.multigrid_hierarchy(shape, bnd, batch=2, open_bound=_one_open(nd)), ops.multigrid_hierarchy(shape, bnd, obstacle=_obs(zero), open_bound=_one_open(nd))
    for l in range(h0.levels):
        (w0, d0, g0), (w1, d1, g1) = h0.weights(l), h1.weights(l)
        assert all(torch.equal(a, b) for a, b in zip(w0, w1)) and torch.equal(d0, d1) and torch.equal(g0, g1)


# ---- 2. the bare V-cycle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_apply_is_bitwise_the_fp32_twin(shape, bnd):
    from deep_fluids_amd import ops
    nd = len(shape)
    names, obs = _all_obstacles(shape, bnd)
    rng = np.random.RandomState(7)
    r = rng.standard_normal((len(names),) + shape).astype(np.float32)        # non-zero on solid and band cells too
    for bits in (0, _one_open(nd)):
        for alpha in (ops.DEFAULT_MG_ALPHA, 1.0):
            h = ops.multigrid_hierarchy(shape, bnd, obstacle=_obs(obs), open_bound=bits, batch=len(names), alpha=alpha)
            for l in range(h.levels):                                          # nothing is read before it is written
                for a in (nd + 2, nd + 3, nd + 4):
                    h._array(l, a).fill_(float("nan"))
            z = _np(ops.multigrid_apply(h, dev(r))).copy()
            z32 = mg.vcycle(mg.hierarchy(obs, bnd, bits, np.float32), r, alpha)
            z64 = mg.vcycle(mg.hierarchy(obs, bnd, bits, np.float64), r.astype(np.float64), alpha)
            e32, eg = float(np.abs(z32 - z64).max()), float(np.abs(z - z64).max())
            print("%s bnd %d open %d alpha %.1f: twin - fp64 %.3e  gpu - fp64 %.3e  |z| %.3e" % (shape, bnd, bits, alpha, e32, eg, float(np.abs(z64).max())))
            assert_bits(z, z32, "%s open %d alpha %.1f: z" % (shape, bits, alpha))
            assert eg <= 3 * e32
            fluid = oref.fluid_mask(obs, bnd)
            assert not z[~fluid].any()                                          # 0 off the fluid, the all-solid entry included
            if "enclosed" in names:                                             # an enclosed fluid cell (n_c = 0) is inactive
                e = names.index("enclosed")
                mid = tuple(n // 2 for n in shape)
                assert fluid[e][mid] and z[e][mid] == 0
            assert_bits(_np(ops.multigrid_apply(h, dev(r))), z, "a second cycle on used scratch")


# ---- 3. k iterations against the fp64 preconditioned recurrence ----------------------------------------------------------------------------
@pytest.mark.parametrize("bits_of", [lambda nd: 0, _one_open], ids=["closed", "open"])
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_k_iterations_against_the_fp64_recurrence(shape, bnd, bits_of):
    from deep_fluids_amd import ops
    bits = bits_of(len(shape))
    names, obs = _all_obstacles(shape, bnd)
    w = pref.solve_input(shape, bnd, obs, bits)
    live = np.array([n != "solid" for n in names])
    flags = ops.obstacle_flags(_obs(obs), bnd)
    h = ops.multigrid_hierarchy(dev(w), bnd, obstacle=flags, open_bound=bits)
    for k in (1, 2, 3, 4):
        x64, it64, _, _ = mg.pcg(w, obs, bits, bnd, 0.0, k, np.float64)
        x32, _, _, _ = mg.pcg(w, obs, bits, bnd, 0.0, k, np.float32)
        e32 = float(np.abs(x32 - x64).max())
        v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=0.0, max_iter=k, obstacle=flags, open_bound=bits, preconditioner=h)
        err = float(np.abs(_np(p) - x64).max())
        print("%s bnd %d open %d k %d: e32 %.3e  gpu %.3e (bound %.3e)  |x| %.3e" % (shape, bnd, bits, k, e32, err, 3 * e32 + 1e-7, float(np.abs(x64).max())))
        assert (_np(iters)[live] == k).all() and (it64[live] == k).all() and (_np(iters)[~live] == 0).all()
        assert err <= 3 * e32 + 1e-7


# ---- 4. the full solve -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits_of", [lambda nd: 0, _one_open], ids=["closed", "open"])
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_solve_residual_projection_and_iterations(shape, bnd, bits_of):
    from deep_fluids_amd import ops
    nd = len(shape)
    bits = bits_of(nd)
    names, obs = _all_obstacles(shape, bnd)
    w = pref.solve_input(shape, bnd, obs, bits)
    live = np.array([n != "solid" for n in names])
    max_iter = ops.default_max_iter(shape)
    b64 = pref.rhs(w, obs, bnd, np.float64)
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=ACC, obstacle=_obs(obs), open_bound=bits, preconditioner="mg")
    _, _, plain = ops.solve_pressure(dev(w), bnd=bnd, accuracy=ACC, obstacle=_obs(obs), open_bound=bits, preconditioner=None)
    x32, it32, r32, broke = mg.pcg(w, obs, bits, bnd, ACC, max_iter, np.float32)
    excess = float(np.abs((b64 - pref.apply_A(x32.astype(np.float64), obs, bits, bnd)) - r32).max())
    res = float(np.abs(b64 - pref.apply_A(_np(p).astype(np.float64), obs, bits, bnd)).max())
    it = _np(iters)
    print("%s bnd %d open %d: iterations gpu %s twin %s plain %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
          (shape, bnd, bits, it.tolist(), it32.tolist(), _np(plain).tolist(), res, ACC, excess))
    assert not broke.any()
    assert (it[live] > 0).all() and (it < max_iter).all() and (it[~live] == 0).all()
    assert res <= ACC + excess
    assert (np.abs(it - it32) <= 2).all()
    if shape == (17, 130):
        assert (it * 4 <= _np(plain)).all()
    if int(oref.fluid_mask(obs, bnd).sum(axis=tuple(range(1, obs.ndim))).max()) <= 1200:
        vex, _ = pref.exact_projection(w, obs, bits, bnd)
        v32 = pref.extrapolate(pref.correct(w, x32, obs, bits, bnd, np.float32), bits, bnd)
        d32, dg = float(np.abs(v32 - vex).max()), float(np.abs(_np(v) - vex).max())
        print("%s bnd %d open %d: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (shape, bnd, bits, d32, dg))
        assert dg <= 3 * d32
    fluid = oref.fluid_mask(obs, bnd)
    assert not _np(p)[~fluid].any()


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits_of", [lambda nd: 0, _one_open], ids=["closed", "open"])
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_batch_invariance_determinism_check_every_and_hierarchy_object(shape, bnd, bits_of):
    from deep_fluids_amd import ops
    bits = bits_of(len(shape))
    names, obs = _all_obstacles(shape, bnd)
    w = pref.solve_input(shape, bnd, obs, bits)
    o = _obs(obs)
    flags = ops.obstacle_flags(o, bnd)
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, obstacle=flags, open_bound=bits, preconditioner="mg")
    it = _np(iters).tolist()
    print("%s bnd %d open %d: obstacles %s iterations %s" % (shape, bnd, bits, names, it))
    for e in range(len(names)):
        ve, pe, ie = ops.solve_pressure(dev(w[e:e + 1]), bnd=bnd, obstacle=o[e:e + 1], open_bound=bits, preconditioner="mg")
        assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
        assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
        assert int(ie[0]) == it[e]
    h = ops.multigrid_hierarchy(dev(w), bnd, obstacle=flags, open_bound=bits)
    ws = ops.pressure_workspace(dev(w))
    ws.fill_(float("nan"))                                 # nothing is read before it is written
    for ce in (None, 1, 16, 64):
        v2, p2, i2 = ops.solve_pressure(dev(w), bnd=bnd, check_every=ce, workspace=ws, obstacle=flags, open_bound=bits, preconditioner=h)   # and reused
        assert_bits(_np(p2), _np(p), "check_every %s" % ce)
        assert_bits(_np(v2), _np(v), "check_every %s" % ce)
        assert torch.equal(i2, iters)
    vi = dev(w)
    assert ops.solve_pressure(vi, bnd=bnd, out=vi, obstacle=flags, open_bound=bits, preconditioner=h)[0] is vi and torch.equal(vi, v)     # in place


def test_an_entry_that_converges_early_is_frozen():
    from deep_fluids_amd import ops
    shape, bnd = (17, 130), 1
    obs = np.zeros((2,) + shape, np.uint8)
    w = oref.solve_input(shape, bnd, obs)
    w[1] *= np.float32(1e-2)                                # entry 1 starts nearer the accuracy and stops first
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, preconditioner="mg")
    it = _np(iters)
    assert 0 < it[1] < it[0]
    v1, p1, i1 = ops.solve_pressure(dev(w[1:2]), bnd=bnd, preconditioner="mg")
    assert_bits(_np(p1)[0], _np(p)[1], "the early entry")
    assert int(i1[0]) == it[1]


def test_a_hierarchy_that_does_not_fit_is_refused():
    from deep_fluids_amd import ops
    w = dev(oref.solve_input((12, 10), 1, np.zeros((2, 12, 10), np.uint8)))
    for h in (ops.multigrid_hierarchy((12, 12), 1, batch=2), ops.multigrid_hierarchy((12, 10), 2, batch=2), ops.multigrid_hierarchy((12, 10), 1, batch=3),
              ops.multigrid_hierarchy((12, 10), 1, batch=2, open_bound="Y")):
        with pytest.raises(ValueError):
            ops.solve_pressure(w, bnd=1, preconditioner=h)
    with pytest.raises(ValueError):
        ops.multigrid_apply(ops.multigrid_hierarchy((12, 10), 1, batch=2), torch.zeros((2, 12, 12), device="cuda"))


# ---- 6. the default is untouched; 7. the step --------------------------------------------------------------------------------------------------
def _scene(shape):
    """from rest: a sphere source low in the box, a solid block above it"""
    from deep_fluids_amd import ops
    nd = len(shape)
    ext = shape[::-1]
    centre = tuple(0.5 * ext[a] if a != 1 else 0.2 * ext[1] for a in range(nd))
    mask = (_np(ops.sphere_mask(shape, centre, 0.15 * ext[0])) != 0)[None]
    obs = np.zeros((1,) + shape, np.uint8)
    sl = [slice(n // 2 - 1, n // 2 + 1) for n in shape]
    sl[-2] = slice(shape[-2] // 2, shape[-2] // 2 + 2)
    obs[(0,) + tuple(sl)] = 1
    return mask, obs


@pytest.mark.parametrize("shape", [(32, 24), (12, 16, 12)])
def test_preconditioner_none_is_bitwise_the_call_without_it(shape):
    from deep_fluids_amd import ops
    nd = len(shape)
    mask, obs = _scene(shape)
    d0, v0 = torch.zeros((1,) + shape, device="cuda"), torch.zeros((1,) + shape + (nd,), device="cuda")
    kw = dict(source=_obs(mask), obstacle=_obs(obs), open_bound="XyY")
    d, vels = ops.simulate_smoke(d0, v0, 8, **kw)
    d2, vels2 = ops.simulate_smoke(d0, v0, 8, preconditioner=None, **kw)
    assert torch.equal(d, d2) and torch.equal(vels, vels2) and float(vels.abs().max()) > 0
    a, b = ops.smoke_step(d, vels[-1], 0.5, **kw), ops.smoke_step(d, vels[-1], 0.5, preconditioner=None, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    w = ops.wall_buoyancy(vels[-1], d, ops.default_buoyancy_force(shape, 0.5), obstacle=_obs(obs), open_bound="XyY")
    for x, y in zip(ops.solve_pressure(w, obstacle=_obs(obs), open_bound="XyY"), ops.solve_pressure(w, obstacle=_obs(obs), open_bound="XyY", preconditioner=None)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("shape", [(32, 24), (12, 16, 12)])
def test_simulate_smoke_with_the_preconditioner(shape):
    from deep_fluids_amd import ops
    nd = len(shape)
    bits = pref.sides("XyY", nd)
    mask, obs = _scene(shape)
    d0, v0 = torch.zeros((1,) + shape, device="cuda"), torch.zeros((1,) + shape + (nd,), device="cuda")
    kw = dict(source=_obs(mask), obstacle=_obs(obs), open_bound="XyY")
    stats = []
    dp, vp = ops.simulate_smoke(d0, v0, 8, **kw)
    dm, vm = ops.simulate_smoke(d0, v0, 8, preconditioner="mg", stats=stats, **kw)
    # the twin's two runs
    tw = {}
    for pre in (False, True):
        d, v = np.zeros((1,) + shape, np.float32), np.zeros((1,) + shape + (nd,), np.float32)
        for _ in range(8):
            d, v = mg.step(d, v, 0.5, obs, bits, source=mask, dtype=np.float32, precondition=pre)
        tw[pre] = (d, v)
    bd, bv = 3 * float(np.abs(tw[True][0] - tw[False][0]).max()), 3 * float(np.abs(tw[True][1] - tw[False][1]).max())
    ed, ev = float((dm - dp).abs().max()), float((vm[-1] - vp[-1]).abs().max())
    fluid = oref.fluid_mask(obs, 1)
    divm = np.abs(pref.divergence(_np(vm[-1]), obs, 1))[fluid].max()
    divp = np.abs(pref.divergence(_np(vp[-1]), obs, 1))[fluid].max()
    print("%s: mg - plain: density %.3e (bound %.3e) velocity %.3e (bound %.3e); divergence mg %.3e plain %.3e; iterations %s" %
          (shape, ed, bd, ev, bv, divm, divp, [int(s[0]) for s in stats]))
    assert float(vm.abs().max()) > 0 and all(int(s[0]) > 0 for s in stats[1:])
    assert divm <= divp + ACC
    assert ed <= bd and ev <= bv


# ---- 8. a generator ----------------------------------------------------------------------------------------------------------------------------
def test_generate_smoke_dataset_with_the_preconditioner(tmp_path):
    from deep_fluids_amd.data import BatchManager, generate_smoke_dataset
    X, Y, T = 24, 32, 3
    root, plain = str(tmp_path / "mg"), str(tmp_path / "plain")
    kw = dict(num_src_x_pos=2, num_src_radius=2, num_frames=T, resolution_x=X, resolution_y=Y)
    assert generate_smoke_dataset(root, preconditioner="mg", **kw) == 2 * 2 * T
    generate_smoke_dataset(plain, **kw)
    assert sorted(os.listdir(os.path.join(root, "v"))) == sorted(os.listdir(os.path.join(plain, "v")))
    keys = [[line.split(": ")[0] for line in open(os.path.join(r, "args.txt"))] for r in (root, plain)]
    assert keys[0] == keys[1]
    with np.load(os.path.join(root, "v", "1_1_2.npz")) as f, np.load(os.path.join(plain, "v", "1_1_2.npz")) as g:
        assert np.isfinite(f["x"]).all() and np.abs(f["x"]).max() > 0 and f["x"].shape == g["x"].shape
        np.testing.assert_array_equal(f["y"], g["y"])
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=False, data_type="velocity", arch="de", batch_size=3, res_x=X, res_y=Y, res_z=1,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, _ = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (3, Y, X, 2)
