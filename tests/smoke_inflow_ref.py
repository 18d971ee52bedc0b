"""NumPy restatement of the noise inflow, the cylinder stamp and the per-entry force as declared in include/deepfluids_hip.h
(df_density_noise_inflow*, df_mac_cylinder_stamp*, df_wall_buoyancy*_open_dev), written from that text, and the step of
scene/smoke3_vel_buo.py:222-232 built from them and from the pieces of smoke_open_ref.  Every piece takes ``dtype``: float64 is the
reference of the GPU tests, float32 (the same operations in the same order) the twin whose distance from float64 sets their tolerance.
This restates THIS project's definition -- its own seeded lattice noise included -- and not mantaflow, which cannot be run here.  Plain
helper, no fixtures.

Layout as smoke_open_ref: density [B,(Z,)Y,X], velocity [B,(Z,)Y,X,D], axis a = 0, 1, 2 means x, y, z.  ``cyl`` [B, 2D+1]: centre,
half-axis vector, radius.  ``noise``: a dict with the fields of df_noise_params except inv_extent (taken from the grid)."""
import numpy as np

import advect_ref as aref
import smoke_obs_ref as oref
import smoke_open_ref as pref
import smoke_ref as sref
from advect_ref import interior_mask

NOISE = dict(pos_scale=45.0, pos_offset=0.0, time_anim=0.2, val_offset=0.75, val_scale=1.0, clamp=True, clamp_neg=0.0, clamp_pos=1.0, seed=123)


def noise_params(**kw):
    out = dict(NOISE)
    out.update(kw)
    return out


# ---- the cylinder ------------------------------------------------------------------------------------------------------------------------------
def _ex(nd):
    return (slice(None),) + (None,) * nd


def _cyl(cyl, D, dtype):
    """centre [B,D], unit axis [B,D], |z| [B], radius [B], valid [B] -- from the fp32 record, in ``dtype`` arithmetic"""
    rec = np.asarray(cyl, np.float32)
    with np.errstate(all="ignore"):
        c, z, radius = rec[:, :D].astype(dtype), rec[:, D:2 * D].astype(dtype), rec[:, 2 * D].astype(dtype)
        zl2 = z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1]
        if D == 3:
            zl2 = zl2 + z[:, 2] * z[:, 2]
        zl = np.sqrt(zl2)
        valid = np.isfinite(rec).all(axis=1) & (zl2 > 0) & np.isfinite(zl2)
        a = z / zl[:, None]
    return c, a, zl, radius, valid


def _axial(q, c, a, nd):
    """h and r2 of the header for points q (a list over x, y[, z], each broadcastable to [B,(Z,)Y,X])"""
    ex = _ex(nd)
    d = [q[k] - c[:, k][ex] for k in range(nd)]
    h = d[0] * a[:, 0][ex] + d[1] * a[:, 1][ex]
    d2 = d[0] * d[0] + d[1] * d[1]
    if nd == 3:
        h = h + d[2] * a[:, 2][ex]
        d2 = d2 + d[2] * d[2]
    return h, np.maximum(d2 - h * h, d2.dtype.type(0))


def _points(shape, dtype, half=None):
    """the cell index per axis as ``dtype``; ``half``: a per-axis bool, add 0.5 there"""
    nd = len(shape)
    return [aref._cell_index(shape, k, dtype) + (dtype(0.5) if half is not None and half[k] else dtype(0)) for k in range(nd)]


def cylinder_sdf(shape, cyl, dtype=np.float64):
    """sdf [B,(Z,)Y,X] at the cell INDICES, and valid [B]; entries that are not valid hold garbage"""
    dtype = np.dtype(dtype).type
    nd = len(shape)
    c, a, zl, radius, valid = _cyl(cyl, nd, dtype)
    ex = _ex(nd)
    with np.errstate(all="ignore"):
        h, r2 = _axial(_points(shape, dtype), c, a, nd)
        dh = np.abs(h) - zl[ex]
        dr = np.sqrt(r2) - radius[ex]
        oh, orr = np.maximum(dh, dtype(0)), np.maximum(dr, dtype(0))
        sdf = np.minimum(np.maximum(dh, dr), dtype(0)) + np.sqrt(oh * oh + orr * orr)
    return sdf.astype(dtype), valid


def cylinder_inside(shape, cyl, half, dtype=np.float64):
    """the inside test of the stamp at the points index + 0.5 * half: |h| <= |z| and r2 < radius*radius, False for invalid entries"""
    dtype = np.dtype(dtype).type
    nd = len(shape)
    c, a, zl, radius, valid = _cyl(cyl, nd, dtype)
    ex = _ex(nd)
    with np.errstate(all="ignore"):
        h, r2 = _axial(_points(shape, dtype, half), c, a, nd)
        return valid[ex] & (np.abs(h) <= zl[ex]) & (r2 < (radius * radius)[ex])


# ---- the noise ---------------------------------------------------------------------------------------------------------------------------------
def lattice_hash(seed, ix, iy, iz):
    """uint32 arithmetic mod 2^32 on arrays of uint32"""
    with np.errstate(over="ignore"):
        h = np.uint32(seed) ^ (ix * np.uint32(0x8DA6B343)) ^ (iy * np.uint32(0xD8163841)) ^ (iz * np.uint32(0xCB1AB31F))
        h = h ^ (h >> np.uint32(16)); h = h * np.uint32(0x7FEB352D)
        h = h ^ (h >> np.uint32(15)); h = h * np.uint32(0x846CA68B)
        h = h ^ (h >> np.uint32(16))
    return h.astype(np.uint32)


def lattice_value(seed, ix, iy, iz, dtype):
    return (lattice_hash(seed, ix, iy, iz) >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -23) - dtype(1)


def noise_at(q, noise, dtype=np.float64, raw=False):
    """N at lattice-space points q (a list over the D axes of broadcastable arrays): interpolation, then offset, scale and clamp
    (``raw``: the interpolated lattice value before them)"""
    dtype = np.dtype(dtype).type
    D = len(q)
    lo = []
    w = []
    for k in range(D):
        qk = np.minimum(np.maximum(np.atleast_1d(np.asarray(q[k], dtype)), dtype(-2.0 ** 30)), dtype(2.0 ** 30))
        f = np.floor(qk)
        t = (qk - f).astype(dtype)
        lo.append(f.astype(np.int64).astype(np.int32).view(np.uint32))
        w.append(((t * t) * (dtype(3) - dtype(2) * t)).astype(dtype))
    lo = list(np.broadcast_arrays(*lo))
    one = np.uint32(1)
    seed = noise["seed"]

    def lerp(a, b, ww):
        return (a + ww * (b - a)).astype(dtype)
    planes = []
    for dz in range(2 if D == 3 else 1):
        with np.errstate(over="ignore"):
            iz = lo[2] + np.uint32(dz) if D == 3 else np.zeros_like(lo[0])
            x1, y1 = lo[0] + one, lo[1] + one
        r0 = lerp(lattice_value(seed, lo[0], lo[1], iz, dtype), lattice_value(seed, x1, lo[1], iz, dtype), w[0])
        r1 = lerp(lattice_value(seed, lo[0], y1, iz, dtype), lattice_value(seed, x1, y1, iz, dtype), w[0])
        planes.append(lerp(r0, r1, w[1]))
    v = lerp(planes[0], planes[1], w[2]) if D == 3 else planes[0]
    if raw:
        return v
    v = ((v + dtype(np.float32(noise["val_offset"]))) * dtype(np.float32(noise["val_scale"]))).astype(dtype)
    if noise["clamp"]:
        v = np.minimum(np.maximum(v, dtype(np.float32(noise["clamp_neg"]))), dtype(np.float32(noise["clamp_pos"])))
    return v


def _vec(x, D):
    return np.broadcast_to(np.asarray(x, np.float32).reshape(-1), (D,))


def noise_grid(shape, noise, time, dtype=np.float64):
    """N(c) on every cell of a grid [(Z,)Y,X] -> [1,(Z,)Y,X]"""
    dtype = np.dtype(dtype).type
    D = len(shape)
    inv = dtype(np.float32(1.0) / np.float32(shape[-1]))
    tq = dtype(np.float32(noise["time_anim"])) * dtype(np.float32(time))
    ps, po = _vec(noise["pos_scale"], D), _vec(noise["pos_offset"], D)
    q = [((aref._cell_index(shape, k, dtype) * dtype(ps[k])) * inv + dtype(po[k])) + tq for k in range(D)]
    return noise_at(q, noise, dtype)


# ---- the inflow, the stamp, the force -------------------------------------------------------------------------------------------------------
def inflow_region(shape, cyl, sigma, bnd=1, dtype=np.float64):
    """(region [B,(Z,)Y,X] bool: interior, a valid entry and sdf <= sigma; sdf)"""
    dtype = np.dtype(dtype).type
    sdf, valid = cylinder_sdf(shape, cyl, dtype)
    with np.errstate(invalid="ignore"):
        region = valid[_ex(len(shape))] & (sdf <= dtype(np.float32(sigma))) & interior_mask(shape, bnd)[None]
    return region, sdf


def inflow_factor(sdf, sigma, dtype=np.float64):
    dtype = np.dtype(dtype).type
    s = dtype(np.float32(sigma))
    return np.minimum(np.maximum(dtype(1) - (dtype(0.5) / s) * (np.asarray(sdf, dtype) + s), dtype(0)), dtype(1)).astype(dtype)


def density_inflow(density, cyl, noise, time, scale, sigma, bnd=1, dtype=np.float64, parts=False):
    dtype = np.dtype(dtype).type
    d = density.astype(dtype)
    shape = d.shape[1:]
    region, sdf = inflow_region(shape, cyl, sigma, bnd, dtype)
    with np.errstate(invalid="ignore"):
        target = ((noise_grid(shape, noise, time, dtype) * dtype(np.float32(scale))) * inflow_factor(sdf, sigma, dtype)).astype(dtype)
        out = np.where(region & (target > d), target, d).astype(dtype)
    return (out, region, target) if parts else out


def cylinder_stamp(vel, cyl, values, dtype=np.float64):
    dtype = np.dtype(dtype).type
    out = vel.astype(dtype).copy()
    shape = vel.shape[1:-1]
    D = vel.shape[-1]
    values = np.asarray(values, np.float32).astype(dtype)
    for a in range(D):
        inside = cylinder_inside(shape, cyl, [k != a for k in range(D)], dtype)
        out[..., a] = np.where(inside, values[:, a][_ex(D)], out[..., a])
    return out


def wall_buoyancy_dev(vel, rho, forces, obstacle, bits, bnd=1, dtype=np.float64):
    """smoke_open_ref.wall_buoyancy with the force of entry b = forces[b]"""
    forces = np.asarray(forces, np.float32)
    return np.concatenate([pref.wall_buoyancy(vel[b:b + 1], rho[b:b + 1], forces[b], obstacle[b:b + 1], bits, bnd, dtype)
                           for b in range(vel.shape[0])], axis=0)


# ---- the whole step ----------------------------------------------------------------------------------------------------------------------------
def step(density, vel, dt, cyl, noise, time, values, forces, bits, scale=1.0, sigma=0.5, obstacle=None, order=2, clamp_mode=2, bnd=1,
         accuracy=1e-4, max_iter=None, dtype=np.float64, parts=False):
    """The statements of scene/smoke3_vel_buo.py:222-232: density inflow, velocity stamp, both advections through the STAMPED velocity (the
    density's band is 0 afterwards: resetOutflow), fill, walls and per-entry buoyancy, projection.  Returns (density, vel); with ``parts``
    also a dict of the intermediate fields."""
    dtype = np.dtype(dtype).type
    shape = density.shape[1:]
    if obstacle is None:
        obstacle = np.zeros(density.shape, np.uint8)
    if max_iter is None:
        max_iter = int(10 * max(shape)) * (1 if len(shape) == 3 else 4)
    d_in = density_inflow(density, cyl, noise, time, scale, sigma, bnd, dtype)
    v_in = cylinder_stamp(vel, cyl, values, dtype)
    rd = oref.advect_density(d_in, v_in, dt, obstacle, order=order, clamp_mode=clamp_mode, bnd=bnd, source=None, dtype=dtype)
    rv = pref.mac_advect(v_in, dt, obstacle, bits, order=order, clamp_mode=clamp_mode, bnd=bnd, dtype=dtype)
    v_adv = pref.extrapolate(rv["vel"], bits, bnd)
    v_wall = wall_buoyancy_dev(v_adv, rd["out"], forces, obstacle, bits, bnd, dtype)
    v, p, iters = pref.solve_pressure(v_wall, obstacle, bits, bnd, accuracy, max_iter, dtype)
    if parts:
        return rd["out"], v, dict(d_in=d_in, v_in=v_in, rd=rd, rv=rv, v_adv=v_adv, v_wall=v_wall, p=p, iters=iters)
    return rd["out"], v
