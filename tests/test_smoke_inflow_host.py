"""CPU-side properties of the restatement in tests/smoke_inflow_ref.py (the noise inflow, the cylinder stamp: this project's own definition
in include/deepfluids_hip.h, its own lattice noise included -- not mantaflow's), of ``ops.cylinder_mask`` and of the scene order of the
smoke3_vel_buo generator.  No GPU."""
import itertools

import numpy as np
import pytest

import smoke_inflow_ref as iref


@pytest.mark.parametrize("D", [2, 3])
def test_noise_is_continuous_across_lattice_planes(D):
    n = iref.noise_params(clamp=False)
    rng = np.random.RandomState(0)
    base = [rng.uniform(-40, 40, 500) for _ in range(D)]
    for k in range(D):
        for plane in (-7.0, 0.0, 1.0, 12.0):
            for dtype, eps in ((np.float64, 1e-9), (np.float32, 2e-6)):
                lo = [b.copy() for b in base]; hi = [b.copy() for b in base]; at = [b.copy() for b in base]
                lo[k][:] = plane - eps; hi[k][:] = plane + eps; at[k][:] = plane
                v_lo, v_hi, v_at = (iref.noise_at(q, n, dtype, raw=True).astype(np.float64) for q in (lo, hi, at))
                # the fade has slope 0 at the planes: a step of eps moves the value by O(eps^2) plus rounding
                tol = 100 * eps * eps + 8 * np.finfo(dtype).eps
                assert np.abs(v_lo - v_at).max() <= tol and np.abs(v_hi - v_at).max() <= tol, (k, plane, dtype)
    # and it is not constant: the test above cannot pass on a flat field
    assert iref.noise_at(base, n, np.float64, raw=True).std() > 0.1


@pytest.mark.parametrize("D", [2, 3])
def test_noise_range_seed_and_negative_coordinates(D):
    rng = np.random.RandomState(1)
    q = [rng.uniform(-300, 300, 20000) for _ in range(D)]
    for dtype in (np.float64, np.float32):
        v = iref.noise_at(q, iref.noise_params(seed=7), dtype, raw=True)
        assert v.dtype == dtype and v.min() >= -1.0 and v.max() < 1.0
        assert np.array_equal(v, iref.noise_at(q, iref.noise_params(seed=7), dtype, raw=True))          # reproducible from the seed
        other = iref.noise_at(q, iref.noise_params(seed=8), dtype, raw=True)
        assert np.abs(other - v).mean() > 0.1                                                            # another seed, another field
    # the lattice values themselves: at integer points the noise is the hashed value, in [-1, 1), on 2^-23 steps
    ints = [np.arange(-50, 50, dtype=np.float64)[:, None] + np.zeros((1, 100))] + [np.arange(-50, 50, dtype=np.float64)[None, :] + np.zeros((100, 1))]
    ints = [a.ravel() for a in ints] + ([np.full(10000, -3.0)] if D == 3 else [])
    lv = iref.noise_at(ints, iref.noise_params(seed=7), np.float64, raw=True)
    assert lv.min() >= -1.0 and lv.max() < 1.0 and np.array_equal(lv * 2.0 ** 23, np.round(lv * 2.0 ** 23))
    assert abs(lv.mean()) < 0.05 and 0.5 < lv.std() < 0.65                                               # uniform on [-1, 1): std 0.577
    # offset, scale and clamp follow the interpolation
    full = iref.noise_at(q, iref.noise_params(seed=7, val_offset=0.75, val_scale=2.0, clamp=True, clamp_neg=0.0, clamp_pos=1.0))
    raw = iref.noise_at(q, iref.noise_params(seed=7), raw=True)
    np.testing.assert_array_equal(full, np.clip((raw + 0.75) * 2.0, 0.0, 1.0))


def test_hash_is_uint32_arithmetic():
    ix = np.array([0, 1, 0xFFFFFFFF, 12345], np.uint32)                 # 0xFFFFFFFF: the lattice coordinate -1
    got = iref.lattice_hash(99, ix, ix[::-1].copy(), np.zeros(4, np.uint32))
    want = []
    for x, y in zip(ix.tolist(), ix[::-1].tolist()):
        h = (99 ^ (x * 0x8DA6B343) ^ (y * 0xD8163841)) & 0xFFFFFFFF
        h ^= h >> 16; h = (h * 0x7FEB352D) & 0xFFFFFFFF
        h ^= h >> 15; h = (h * 0x846CA68B) & 0xFFFFFFFF
        h ^= h >> 16
        want.append(h)
    assert got.dtype == np.uint32 and got.tolist() == want


def test_factor_ramp():
    for sigma in (0.5, 2.0):
        for dtype in (np.float64, np.float32):
            f = iref.inflow_factor(np.array([-3 * sigma, -sigma, 0.0, sigma, 2 * sigma]), sigma, dtype)
            np.testing.assert_array_equal(f, np.array([1.0, 1.0, 0.5, 0.0, 0.0], dtype))


def test_cylinder_sdf_on_and_inside_the_surface():
    shape = (17, 17, 17)
    cyl = np.array([[8, 8, 8, 0, 3, 0, 4]], np.float32)                # along y: caps at j = 5, 11, wall at radius 4
    for dtype in (np.float64, np.float32):
        sdf, valid = iref.cylinder_sdf(shape, cyl, dtype)
        assert valid.all()
        at = lambda i, j, k: float(sdf[0, k, j, i])
        assert at(12, 8, 8) == 0.0 and at(8, 11, 8) == 0.0 and at(8, 5, 8) == 0.0 and at(8, 8, 4) == 0.0        # on the wall, on the caps
        assert at(8, 8, 8) == -3.0                                     # the centre: the caps are nearer than the wall
        assert at(11, 8, 8) == -1.0 and at(8, 10, 8) == -1.0 and at(10, 9, 10) == pytest.approx(-(4 - np.sqrt(8.0)), abs=1e-6)
        assert at(14, 8, 8) == 2.0 and at(8, 14, 8) == 3.0             # outside: beside the wall, above a cap
        assert at(15, 15, 8) == pytest.approx(5.0, abs=1e-6)           # beyond the rim: 3 from the wall and 4 from the cap
    # a tilted axis in 2-D, against a brute-force distance to the rectangle's outline
    cyl2 = np.array([[10.25, 9.5, 3.0, 1.5, 2.5]], np.float32)
    sdf, _ = iref.cylinder_sdf((20, 22), cyl2, np.float64)
    a = np.array([3.0, 1.5]) / np.hypot(3.0, 1.5); n = np.array([-a[1], a[0]])
    zl = np.hypot(3.0, 1.5)
    s = np.linspace(-1, 1, 4001)
    outline = np.concatenate([np.array([10.25, 9.5]) + sh * zl * a + t[:, None] * 2.5 * n for sh in (-1, 1) for t in (s,)] +
                             [np.array([10.25, 9.5]) + t[:, None] * zl * a + sn * 2.5 * n for sn in (-1, 1) for t in (s,)])
    for (j, i) in ((3, 4), (9, 10), (10, 12), (15, 2), (11, 14), (8, 7)):
        dist = np.sqrt(((outline - np.array([i, j])) ** 2).sum(axis=1)).min()
        assert abs(abs(float(sdf[0, j, i])) - dist) < 2e-3, (i, j)
    assert sdf[0, 9, 10] < 0 and sdf[0, 15, 2] > 0
    # entries that stamp nothing: a zero-length axis, a NaN
    bad = np.array([[8, 8, 8, 0, 0, 0, 4], [8, np.nan, 8, 0, 3, 0, 4], [8, 8, 8, 0, 3, 0, np.inf]], np.float32)
    assert not iref.cylinder_sdf(shape, bad)[1].any()
    region, _ = iref.inflow_region(shape, bad, 0.5)
    assert not region.any()
    assert not any(iref.cylinder_inside(shape, bad, [k != a for k in range(3)]).any() for a in range(3))


def test_inflow_touches_only_its_region_and_never_lowers_the_density():
    shape = (12, 16, 20)
    cyl = np.array([[4, 6, 5, 0, 2.5, 0, 3], [30, 6, 5, 0, 2.5, 0, 3]], np.float32)          # the second lies wholly outside
    rng = np.random.RandomState(2)
    d = rng.uniform(0, 0.4, (2,) + shape)
    out, region, target = iref.density_inflow(d, cyl, iref.noise_params(), 1.5, 1.0, 0.5, parts=True)
    assert region[0].sum() > 100 and not region[1].any() and target[0][region[0]].std() > 0.05
    assert np.array_equal(out[~region], d[~region]) and (out >= d).all() and (out[0][region[0]] > d[0][region[0]]).any()
    assert np.array_equal(out[1], d[1])
    high = np.full_like(d, 2.0)                                       # a density already above the target comes back untouched
    assert np.array_equal(iref.density_inflow(high, cyl, iref.noise_params(), 1.5, 1.0, 0.5), high)


@pytest.mark.parametrize("shape,center,z,radius", [((9, 11), (5.25, 4.0), (1.5, 0.0), 2.0), ((9, 11), (5.0, 4.5), (1.0, 2.0), 2.5),
                                                   ((7, 8, 9), (4.0, 4.5, 3.0), (0.0, 1.75, 0.0), 2.5),
                                                   ((7, 8, 9), (4.5, 4.0, 3.5), (1.0, 1.0, 2.0), 2.0), ((7, 8, 9), (-1.0, 4.0, 3.5), (3.0, 0.0, 0.0), 3.0)])
def test_cylinder_mask_agrees_with_a_loop(shape, center, z, radius):
    from deep_fluids_amd import ops
    got = ops.cylinder_mask(shape, center, z, radius).numpy()
    zl = np.sqrt(sum(v * v for v in z))
    want = np.zeros(shape, np.uint8)
    for idx in itertools.product(*[range(n) for n in shape]):
        d = [idx[::-1][a] + 0.5 - center[a] for a in range(len(shape))]
        h = sum(d[a] * z[a] / zl for a in range(len(shape)))
        want[idx] = abs(h) <= zl and max(sum(v * v for v in d) - h * h, 0.0) < radius * radius
    assert got.dtype == np.uint8 and np.array_equal(got, want) and 0 < want.sum() < want.size
    # the restatement's face test at cell centres (all axes shifted by a half) is the same mask
    cyl = np.array([list(center) + list(z) + [radius]], np.float32)
    assert np.array_equal(iref.cylinder_inside(shape, cyl, [True] * len(shape))[0], want.astype(bool))
    with pytest.raises(ValueError):
        ops.cylinder_mask(shape, center, (0.0,) * len(shape), radius)
    with pytest.raises(ValueError):
        ops.CylinderShape(center, (0.0,) * len(shape), radius)


def test_scene_order_is_the_scripts_meshgrid():
    from deep_fluids_amd.data import smoke3_vel_buo_scenes
    lo1, hi1, n1, lo2, hi2, n2 = 1, 5, 5, -2e-4, -10e-4, 3
    p_list, pi_list = smoke3_vel_buo_scenes(lo1, hi1, n1, lo2, hi2, n2)
    p1_space, p2_space = np.linspace(lo1, hi1, n1), np.linspace(lo2, hi2, n2)
    np.testing.assert_array_equal(p_list, np.array(np.meshgrid(p1_space, p2_space)).T.reshape(-1, 2))
    np.testing.assert_array_equal(pi_list, np.array(np.meshgrid(range(n1), range(n2))).T.reshape(-1, 2))
    assert p_list.shape == (15, 2) and pi_list[:4].tolist() == [[0, 0], [0, 1], [0, 2], [1, 0]]          # the buoyancy index runs fastest
    assert p_list[4].tolist() == [p1_space[1], p2_space[1]]


def test_holders_and_forces():
    import torch
    from deep_fluids_amd import ops
    n = ops.NoiseField()
    assert (n.pos_scale, n.val_offset, n.val_scale, n.time_anim, n.clamp, n.clamp_neg, n.clamp_pos, n.pos_offset) == (45, 0.75, 1.0, 0.2, True, 0.0, 1.0, 0)
    q = n.params(3, 112)
    assert list(q.pos_scale) == [45.0] * 3 and q.clamp == 1 and q.inv_extent == float(np.float32(1) / np.float32(112))
    c = ops.CylinderShape([[1, 2, 3], [4, 5, 6]], [0, 2, 0], 1.5)
    assert tuple(c.packed.shape) == (2, 7) and c.packed[1].tolist() == [4, 5, 6, 0, 2, 0, 1.5] and c.dim == 3
    assert c.entry(1).packed.tolist() == [[4, 5, 6, 0, 2, 0, 1.5]]
    inflow = ops.NoiseInflow(c, n, time_step=0.5)
    assert inflow.time(4, 0.25) == 2.0 and ops.NoiseInflow(c, n).time(4, 0.25) == 1.0
    with pytest.raises(ValueError):
        ops.NoiseInflow(c, n, sigma=0.0)
    f = ops.buoyancy_forces((32, 64, 112), 0.5, [-2e-4, -6e-4])
    assert f.dtype == torch.float32 and tuple(f.shape) == (2, 3)
    for b, g in enumerate((-2e-4, -6e-4)):
        assert f[b].tolist() == [float(np.float32(x)) for x in ops.default_buoyancy_force((32, 64, 112), 0.5, g)]
