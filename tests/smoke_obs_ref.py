"""NumPy restatement of the smoke solver step AROUND OBSTACLES as declared in include/deepfluids_hip.h (the `_flags` entry points):
smoke_ref.py / advect_ref.py with "interior" read as "fluid" (interior and not an obstacle), parametrised by dtype in the same way --
float64 is the reference of the GPU tests, float32 the twin whose distance from float64 sets their tolerance.  The first-order value
fwd and the source stamp ignore obstacles and are taken from advect_ref / smoke_ref unchanged.  Plain helper, no fixtures.

Layout: obstacle [B,(Z,)Y,X] (nonzero = solid, one per batch entry), otherwise as smoke_ref.  Axis a = 0, 1, 2 means x, y, z."""
import itertools

import numpy as np

import advect_ref as aref
import smoke_ref as sref
from advect_ref import BAND, COR, FWD, NOCORNER, interior_mask  # noqa: F401
from smoke_ref import _ax, _dot, stacked_to_vel, vel_to_stacked  # noqa: F401


def fluid_mask(obstacle, bnd):
    """[B,(Z,)Y,X] bool: interior and not an obstacle"""
    obstacle = np.asarray(obstacle)
    return interior_mask(obstacle.shape[1:], bnd)[None] & (obstacle == 0)


def _shift(m, a, sh):
    """m at c - sh*e_a (sh = +1: the low neighbour), False where that cell is outside the grid"""
    ax = m.ndim - 1 - a
    out = np.roll(m, sh, axis=ax)
    idx = [slice(None)] * m.ndim
    idx[ax] = 0 if sh > 0 else -1
    out[tuple(idx)] = False
    return out


def flags(obstacle, bnd):
    """uint8 [B,(Z,)Y,X]: bit 0 = fluid, bits 1..6 = the x-, x+, y-, y+, z-, z+ neighbour is fluid"""
    fl = fluid_mask(obstacle, bnd)
    out = fl.astype(np.uint8)
    for a in range(fl.ndim - 1):
        out |= (_shift(fl, a, 1).astype(np.uint8) << (1 + 2 * a)) | (_shift(fl, a, -1).astype(np.uint8) << (2 + 2 * a))
    return out


def face_mask(fluid, a):
    """component a of cell c is kept: c and c - e_a are both fluid"""
    return fluid & _shift(fluid, a, 1)


def regions(fluid1):
    """connected fluid regions of ONE grid [(Z,)Y,X]: int labels, -1 outside the fluid; the number of regions"""
    lab = np.full(fluid1.shape, -1, np.int64)
    n = 0
    for start in zip(*np.nonzero(fluid1)):
        if lab[start] >= 0:
            continue
        lab[start] = n
        todo = [start]
        while todo:
            c = todo.pop()
            for ax in range(fluid1.ndim):
                for s in (-1, 1):
                    q = list(c); q[ax] += s; q = tuple(q)
                    if 0 <= q[ax] < fluid1.shape[ax] and fluid1[q] and lab[q] < 0:
                        lab[q] = n
                        todo.append(q)
        n += 1
    return lab, n


# ---- MacCormack with flags ---------------------------------------------------------------------------------------------------------------
def _corner_range(orig, cells, fluid, mn, mx, found):
    d = len(cells)
    B = orig.shape[0]
    b = np.arange(B).reshape([B] + [1] * d)
    for off in itertools.product((0, 1), repeat=d):
        idx = tuple(cells[a] + off[a] for a in reversed(range(d)))
        ok = fluid[(b,) + idx]
        v = orig[(b,) + idx]
        mn = np.where(ok, np.where(found, np.minimum(mn, v), v), mn)
        mx = np.where(ok, np.where(found, np.maximum(mx, v), v), mx)
        found = found | ok
    return mn, mx, found


def _maccormack(orig, fwd, du, where, fluid, inter, clamp_mode, bnd, dtype):
    """the second half of order 2 on one cell-centred grid: corrected and clamped over fluid corners on `where`, fwd elsewhere inside"""
    shape = orig.shape[1:]
    bwd = aref.semi_lagrange(fwd, du, -1, bnd, dtype)
    cor = (fwd + dtype(0.5) * (orig - bwd)).astype(dtype)
    cells = aref._clamp_cells(shape, du, +1, dtype)
    mn = np.zeros(orig.shape, dtype); mx = np.zeros(orig.shape, dtype); found = np.zeros(orig.shape, bool)
    mn, mx, found = _corner_range(orig, cells, fluid, mn, mx, found)
    flat = np.ravel_multi_index(tuple(np.broadcast_to(c, orig.shape) for c in reversed(cells)), shape)
    if clamp_mode == 1:
        cells2 = aref._clamp_cells(shape, du, -1, dtype)
        mn, mx, found = _corner_range(orig, cells2, fluid, mn, mx, found)
        flat = flat * int(np.prod(shape)) + np.ravel_multi_index(tuple(np.broadcast_to(c, orig.shape) for c in reversed(cells2)), shape)
    if clamp_mode == 2:
        revert = (cor < mn) | (cor > mx)
        val = np.where(revert, fwd, cor)
        br = np.where(revert, FWD, COR)
    else:
        val = np.minimum(np.maximum(cor, mn), mx)
        br = np.full(orig.shape, COR)
    val = np.where(found, val, fwd)
    br = np.where(found, br, NOCORNER)
    out = np.where(where, val, fwd).astype(dtype)                    # fwd is 0 on wall cells already
    return dict(out=out, branch=np.where(where, br, np.where(inter, FWD, BAND)), cell=np.where(where, flat, 0), fwd=fwd, cor=cor, orig=orig)


def advect_density(density, vel, dt, obstacle, order=2, clamp_mode=2, bnd=1, vel_scale=1.0, source=None, source_value=1.0, dtype=np.float64):
    """advect_ref.step around obstacles; the same record"""
    dtype = np.dtype(dtype).type
    assert order in (1, 2) and clamp_mode in (1, 2) and bnd >= 1
    shape = density.shape[1:]
    orig = aref.stamp(density, source, source_value, dtype)
    du = aref.displacement(vel, dt, bnd, vel_scale, dtype)
    inter = np.broadcast_to(interior_mask(shape, bnd)[None], orig.shape)
    fwd = aref.semi_lagrange(orig, du, +1, bnd, dtype)
    if order == 1:
        return {"out": fwd, "branch": np.where(inter, FWD, BAND), "cell": np.zeros(orig.shape, np.int64), "fwd": fwd, "cor": fwd, "orig": orig}
    fluid = fluid_mask(obstacle, bnd)
    return _maccormack(orig, fwd, du, fluid, fluid, inter, clamp_mode, bnd, dtype)


def mac_advect(vel, dt, obstacle, order=2, clamp_mode=2, bnd=1, dtype=np.float64):
    """smoke_ref.mac_advect around obstacles; the same record (components stacked along the batch axis)"""
    dtype = np.dtype(dtype).type
    assert order in (1, 2) and clamp_mode in (1, 2) and bnd >= 1
    if order == 1:
        return sref.mac_advect(vel, dt, order=1, clamp_mode=clamp_mode, bnd=bnd, dtype=dtype)
    shape = vel.shape[1:-1]
    D = vel.shape[-1]
    inter = np.broadcast_to(interior_mask(shape, bnd)[None], vel.shape[:-1])
    fluid = fluid_mask(obstacle, bnd)
    keys = ("out", "branch", "cell", "fwd", "cor", "orig")
    rec = {k: [] for k in keys}
    for a in range(D):
        orig = vel[..., a].astype(dtype)
        du = sref.face_displacement(vel, a, dt, dtype)
        fwd = aref.semi_lagrange(orig, du, +1, bnd, dtype)
        vals = _maccormack(orig, fwd, du, face_mask(fluid, a), fluid, inter, clamp_mode, bnd, dtype)
        for k in keys:
            rec[k].append(vals[k])
    rec = {k: np.concatenate(v, axis=0) for k, v in rec.items()}
    rec["vel"] = stacked_to_vel(rec["out"], D)
    rec["D"] = D
    return rec


def _reachable(ijk, du, clamp_mode, ext, near):
    D = len(ijk)
    for sign in ((+1, -1) if clamp_mode == 1 else (+1,)):
        opts = []
        for ax in range(D):
            t = ijk[ax] - sign * du[ax]
            c = {int(t)}
            if abs(t - round(t)) < near:
                c |= {int(round(t)) - 1, int(round(t))}
            opts.append(sorted({min(max(v, 0), ext[ax] - 2) for v in c}))
        for cell in itertools.product(*opts):
            for off in itertools.product((0, 1), repeat=D):
                yield tuple(cell[ax] + off[ax] for ax in reversed(range(D)))


def alternatives(r64, vel, dt, clamp_mode, bnd, obstacle, vel_scale=1.0, near=1e-3):
    """``alt`` of advect_ref.compare for an advect_density record: fwd | cor of the cell and orig at the FLUID corners of every clamp
    cell reachable by moving a trunc() whose argument lies within ``near`` of an integer"""
    shape = r64["out"].shape[1:]
    ext = shape[::-1]
    fluid = fluid_mask(obstacle, bnd)
    dus = aref.displacement(vel, dt, bnd, vel_scale, np.float64)

    def alt(index):
        cand = [float(r64["fwd"][index]), float(r64["cor"][index])]
        for idx in _reachable(index[1:][::-1], [float(x[index]) for x in dus], clamp_mode, ext, near):
            if fluid[(index[0],) + idx]:
                cand.append(float(r64["orig"][(index[0],) + idx]))
        return cand
    return alt


def mac_alternatives(r64, vel, dt, clamp_mode, bnd, obstacle, near=1e-3):
    """the same for a mac_advect record (component-major rows)"""
    D = r64["D"]
    B = r64["out"].shape[0] // D
    shape = r64["out"].shape[1:]
    ext = shape[::-1]
    fluid = fluid_mask(obstacle, bnd)
    dus = [sref.face_displacement(vel, a, dt, np.float64) for a in range(D)]

    def alt(index):
        a, b = divmod(index[0], B)
        vidx = (b,) + tuple(index[1:])
        cand = [float(r64["fwd"][index]), float(r64["cor"][index])]
        for idx in _reachable(index[1:][::-1], [float(dus[a][ax][vidx]) for ax in range(D)], clamp_mode, ext, near):
            if fluid[(b,) + idx]:
                cand.append(float(r64["orig"][(index[0],) + idx]))
        return cand
    return alt


# ---- walls and buoyancy, pressure ----------------------------------------------------------------------------------------------------------
def wall_buoyancy(vel, rho, force, obstacle, bnd=1, dtype=np.float64):
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype); rho = rho.astype(dtype)
    nd = vel.ndim - 2
    fluid = fluid_mask(obstacle, bnd)
    out = np.zeros_like(vel)
    for a in range(vel.shape[-1]):
        val = vel[..., a] + (dtype(0.5) * dtype(np.float32(force[a]))) * (rho + np.roll(rho, 1, axis=_ax(nd, a)))
        out[..., a] = np.where(face_mask(fluid, a), val, dtype(0))
    return out


def rhs(vel, obstacle, bnd=1, dtype=np.float64):
    """b = -div on fluid cells, 0 elsewhere"""
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype)
    nd = vel.ndim - 2
    div = None
    for a in range(vel.shape[-1]):
        t = np.roll(vel[..., a], -1, axis=_ax(nd, a)) - vel[..., a]
        div = t if div is None else div + t
    return np.where(fluid_mask(obstacle, bnd), -div, dtype(0)).astype(dtype)


def apply_A(x, obstacle, bnd=1):
    """(A x)[c] = n_c x[c] - sum over fluid neighbours in the order x-, x+, y-, y+, z-, z+; 0 outside the fluid.  Keeps x's dtype."""
    dtype = x.dtype.type
    nd = x.ndim - 1
    fluid = fluid_mask(obstacle, bnd)
    s = np.zeros_like(x)
    cnt = np.zeros(x.shape, np.int64)
    for a in range(nd):
        for sh in (1, -1):
            ok = fluid & _shift(fluid, a, sh)
            s = s + np.where(ok, np.roll(x, sh, axis=_ax(nd, a)), dtype(0))
            cnt = cnt + ok
    return np.where(fluid, cnt.astype(dtype) * x - s, dtype(0)).astype(dtype)


def neighbour_count(obstacle, bnd=1):
    f = flags(obstacle, bnd)
    n = np.zeros(f.shape, np.int64)
    for bit in range(1, 7):
        n += (f >> bit) & 1
    return np.where(f & 1, n, 0)


def cg(vel, obstacle, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64, dot=None, amax=None):
    """smoke_ref.cg on the fluid cells (``dot`` / ``amax`` as there).  Returns (x, iterations [B], r)."""
    dot = _dot if dot is None else dot
    amax = sref._amax if amax is None else amax
    dtype = np.dtype(dtype).type
    b = rhs(vel, obstacle, bnd, dtype)
    B = b.shape[0]
    ex = (slice(None),) + (None,) * (b.ndim - 1)
    x = np.zeros_like(b); r = b.copy(); p = b.copy()
    rr_old = np.ones(B, dtype)
    active = np.ones(B, bool)
    iters = np.zeros(B, np.int32)
    k = 0
    while True:
        rr = dot(r, r)
        mx = amax(r)
        active = active & (mx > dtype(accuracy)) & (rr > 0) & (iters < max_iter)
        if not active.any():
            break
        with np.errstate(all="ignore"):
            beta = np.zeros(B, dtype) if k == 0 else (rr / rr_old).astype(dtype)
            pn = (r + beta[ex] * p).astype(dtype)
            q = apply_A(pn, obstacle, bnd)
            pq = dot(pn, q)
            alpha = np.where(pq > 0, rr / pq, dtype(0)).astype(dtype)
        a_ = active[ex]
        x = np.where(a_, x + alpha[ex] * pn, x).astype(dtype)
        r = np.where(a_, r - alpha[ex] * q, r).astype(dtype)
        p = np.where(a_, pn, p)
        rr_old = np.where(active, rr, rr_old)
        iters = iters + active
        k += 1
    return x, iters, r


def correct(vel, p, obstacle, bnd=1, dtype=np.float64):
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype); p = p.astype(dtype)
    nd = vel.ndim - 2
    fluid = fluid_mask(obstacle, bnd)
    out = np.zeros_like(vel)
    for a in range(vel.shape[-1]):
        out[..., a] = np.where(face_mask(fluid, a), vel[..., a] - (p - np.roll(p, 1, axis=_ax(nd, a))), dtype(0))
    return out


def solve_pressure(vel, obstacle, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64):
    x, iters, _ = cg(vel, obstacle, bnd, accuracy, max_iter, dtype)
    return correct(vel, x, obstacle, bnd, dtype), x, iters


def dense_A(shape, bnd, obstacle):
    """A over the fluid cells of ONE grid (obstacle [(Z,)Y,X]), fp64 [n, n], and the flat indices of those cells"""
    obstacle = np.asarray(obstacle)[None]
    cells = np.flatnonzero(fluid_mask(obstacle, bnd).ravel())
    n = cells.size
    A = np.zeros((n, n))
    for col in range(n):
        e = np.zeros((1,) + tuple(shape))
        e.reshape(-1)[cells[col]] = 1.0
        A[:, col] = apply_A(e, obstacle, bnd).reshape(-1)[cells]
    return A, cells


def exact_projection(vel, obstacle, bnd=1):
    """fp64: the minimum-norm least-squares solution of A p = b per entry (dense; A is singular once per fluid region, which least
    squares copes with), and the projected velocity.  Small grids only."""
    vel = vel.astype(np.float64)
    shape = vel.shape[1:-1]
    b = rhs(vel, obstacle, bnd, np.float64)
    p = np.zeros_like(b)
    for e in range(b.shape[0]):
        A, cells = dense_A(shape, bnd, obstacle[e])
        assert A.shape[0] <= 1200, "exact_projection is for small grids"
        if cells.size:
            p[e].reshape(-1)[cells] = np.linalg.lstsq(A, b[e].reshape(-1)[cells], rcond=None)[0]
    return correct(vel, p, obstacle, bnd, np.float64), p


def divergence(vel, obstacle, bnd=1):
    return -rhs(vel, obstacle, bnd, np.float64)


def step(density, vel, dt, obstacle, source=None, force=None, order=2, clamp_mode=2, bnd=1, accuracy=1e-4, max_iter=None, dtype=np.float64):
    """The statements of scene/smoke3_obs_buo.py:211-219.  Returns (density, vel, density record, velocity record)."""
    dtype = np.dtype(dtype).type
    shape = density.shape[1:]
    force = sref.default_force(shape, dt) if force is None else force
    if max_iter is None:
        max_iter = int(10 * max(shape)) * (1 if len(shape) == 3 else 4)
    rd = advect_density(density, vel, dt, obstacle, order=order, clamp_mode=clamp_mode, bnd=bnd, source=source, dtype=dtype)
    rv = mac_advect(vel, dt, obstacle, order=order, clamp_mode=clamp_mode, bnd=bnd, dtype=dtype)
    v = wall_buoyancy(rv["vel"], rd["out"], force, obstacle, bnd, dtype)
    v, _, _ = solve_pressure(v, obstacle, bnd, accuracy, max_iter, dtype)
    return rd["out"], v, rd, rv


# ---- fixtures: obstacles at the edges of the rule ---------------------------------------------------------------------------------------------
def obstacle_cases(shape, bnd):
    """name -> obstacle [(Z,)Y,X] uint8 for one grid"""
    nd = len(shape)
    mid = tuple(n // 2 for n in shape)
    out = {"none": np.zeros(shape, np.uint8)}
    o = np.zeros(shape, np.uint8); o[mid] = 1
    out["cell"] = o                                                  # a single solid cell in mid-fluid
    o = np.zeros(shape, np.uint8); o[tuple(slice(bnd, bnd + 2) for _ in shape)] = 1
    out["block"] = o                                                 # 2x2(x2) touching the wall
    o = np.zeros(shape, np.uint8)                                    # a wall of solid cells across x: two fluid regions
    o[(slice(None),) * (nd - 1) + (shape[-1] // 2,)] = 1
    out["split"] = o
    if all(m - 1 >= bnd and m + 1 < n - bnd for m, n in zip(mid, shape)):     # one enclosed fluid cell (n_c = 0): a shell around mid
        o = np.zeros(shape, np.uint8)
        o[tuple(slice(m - 1, m + 2) for m in mid)] = 1
        o[mid] = 0
        out["enclosed"] = o
    out["solid"] = np.ones(shape, np.uint8)                          # solid everywhere
    if shape == (17, 130):                                           # a solid run across the 256-cell workgroup boundary (flat 250..262)
        o = np.zeros(shape, np.uint8); o.reshape(-1)[250:263] = 1
        out["run256"] = o
    if shape == (19, 10, 7):
        out["sphere"] = aref.sphere_mask_loop(shape, (3.5, 5.0, 9.5), 2.2)
    return out


def batch_obstacle(shape, bnd, names):
    c = obstacle_cases(shape, bnd)
    return np.stack([c[n] for n in names])


def mixed_batch(shape, bnd):
    """B = 3, a different obstacle per entry: the shape's special obstacle (or a single cell), the block, the split"""
    c = obstacle_cases(shape, bnd)
    first = "run256" if "run256" in c else "sphere" if "sphere" in c else "cell"
    return np.stack([c[first], c["block"], c["split"]])


# The shapes of the GPU tests are smoke_ref.MAC_SHAPES.  OBS_SEEDS: (shape, bnd, order, mode, kind) -> the seed of make_velocity /
# make_density where the default 0 lets the fp32 twin flip too many branches (tuned on the CPU by the gate of
# tests/test_smoke_obstacles_host.py); kind is "mac" or "density".
OBS_SEEDS = {}
OBS_DT = 1.0


def advect_cases(kind):
    """(name, vel, density | None, obstacle [3,..], kwargs): order 2, clamp modes 1 | 2, B = 3 with a different obstacle per entry"""
    for shape, bnds in sref.MAC_SHAPES:
        for bnd in bnds:
            for mode in (1, 2):
                seed = OBS_SEEDS.get((shape, bnd, 2, mode, kind), 0)
                vmax = min(3.0, 0.4 * min(shape))
                vel = sref.make_velocity(shape, seed=seed, vmax=vmax)
                rho = sref.make_density(shape, seed=seed) if kind == "density" else None
                yield ("%s-%s-m%d-b%d" % (kind, "x".join(map(str, shape)), mode, bnd), vel, rho, mixed_batch(shape, bnd),
                       dict(order=2, clamp_mode=mode, bnd=bnd))


def solve_input(shape, bnd, obstacle, seed=4):
    """a velocity with zero solid faces and some divergence: the input solve_pressure expects"""
    B = obstacle.shape[0]
    rng = np.random.RandomState(seed)
    vel = sref.make_velocity(shape, B=B, seed=seed, vmax=1.0)
    rho = rng.uniform(0, 1, (B,) + tuple(shape)).astype(np.float32)
    return wall_buoyancy(vel, rho, (0.0, 0.25, 0.0)[:len(shape)], obstacle, bnd, np.float32)
