"""NumPy restatement of the smoke solver step WITH OPEN SIDES as declared in include/deepfluids_hip.h (the `_open` entry points,
df_open_extrapolate*, df_density_sphere_source*): smoke_ref.py / smoke_obs_ref.py with the cell classes interior | open | wall and the
"live face" in place of the "kept face", parametrised by dtype in the same way -- float64 is the reference of the GPU tests, float32
(the same operations in the same order, dot products NumPy sums) the twin whose distance from float64 sets their tolerance.  This is a
restatement of THIS project's definition, not of mantaflow, which cannot be run here.  Plain helper, no fixtures.

Layout as smoke_obs_ref: obstacle [B,(Z,)Y,X] (nonzero = solid), axis a = 0, 1, 2 means x, y, z.  ``bits``: the open_sides int, bit
2a = the low side of axis a is open, bit 2a + 1 = its high side."""
import numpy as np

import advect_ref as aref
import smoke_obs_ref as oref
import smoke_ref as sref
from advect_ref import BAND, COR, FWD, NOCORNER, interior_mask  # noqa: F401
from smoke_obs_ref import _shift, fluid_mask
from smoke_ref import _ax, _dot, stacked_to_vel, vel_to_stacked  # noqa: F401

SPECS = ["", "Y", "xX", "XyY", "xXyY", "xXyYzZ"]


def sides(spec, dim):
    """the bits of a string of xXyYzZ (lower case: the low side); a 2-D grid has no z sides, so they are dropped from the spec"""
    bits = 0
    for ch in spec:
        at = "xXyYzZ".index(ch)
        if at < 2 * dim:
            bits |= 1 << at
    return bits


def specs(dim):
    """the open specs that differ on a grid of ``dim`` axes, as (name, bits)"""
    seen, out = set(), []
    for s in SPECS:
        b = sides(s, dim)
        if b not in seen:
            seen.add(b)
            out.append((s, b))
    return out


# ---- cell classes ------------------------------------------------------------------------------------------------------------------------------
def open_mask(shape, bnd, bits):
    """[(Z,)Y,X] bool: a band cell that lies, on every axis where its index is outside [bnd, extent - bnd), on an open side"""
    nd = len(shape)
    band = np.zeros(shape, bool)
    ok = np.ones(shape, bool)
    for a in range(nd):
        ax = nd - 1 - a
        n = shape[ax]
        idx = np.arange(n)
        sh = [1] * nd
        sh[ax] = n
        lo = (idx < bnd).reshape(sh)
        hi = (idx >= n - bnd).reshape(sh)
        band = band | lo | hi
        ok = ok & (~lo | bool(bits >> (2 * a) & 1)) & (~hi | bool(bits >> (2 * a + 1) & 1))
    return band & ok


def wall_mask(shape, bnd, bits):
    return ~interior_mask(shape, bnd) & ~open_mask(shape, bnd, bits)


def _opn(obstacle, bnd, bits):
    obstacle = np.asarray(obstacle)
    return np.broadcast_to(open_mask(obstacle.shape[1:], bnd, bits)[None], obstacle.shape).copy()


def both_mask(fluid, a):
    """component a of cell c lies between two fluid cells"""
    return fluid & _shift(fluid, a, 1)


def live_mask(fluid, opn, a):
    """component a of cell c is live: one of c, c - e_a is fluid and the other is fluid or open"""
    f_lo, o_lo = _shift(fluid, a, 1), _shift(opn, a, 1)
    return (fluid & (f_lo | o_lo)) | (opn & f_lo)


def high_face_mask(shape, bnd, bits, a):
    """[(Z,)Y,X]: an open cell whose c - e_a is interior by its index -- component a sits on the high-side boundary face"""
    return open_mask(shape, bnd, bits) & _shift(interior_mask(shape, bnd), a, 1)


# ---- MAC self-advection ----------------------------------------------------------------------------------------------------------------------
def _trace(g, du, sign, dtype):
    """interp(g, centre - sign*du) on EVERY cell (advect_ref.semi_lagrange without its interior mask)"""
    shape = g.shape[1:]
    pos = []
    for a in range(len(du)):
        c = aref._cell_index(shape, a, dtype) + dtype(0.5)
        pos.append(c - du[a] if sign > 0 else c + du[a])
    return aref.interp(g, pos, dtype).astype(dtype)


def mac_advect(vel, dt, obstacle, bits, order=2, clamp_mode=2, bnd=1, dtype=np.float64):
    """smoke_obs_ref.mac_advect with open sides; the same record (components stacked along the batch axis)"""
    dtype = np.dtype(dtype).type
    assert order in (1, 2) and clamp_mode in (1, 2) and bnd >= 1
    shape = vel.shape[1:-1]
    D = vel.shape[-1]
    inter = np.broadcast_to(interior_mask(shape, bnd)[None], vel.shape[:-1])
    fluid = fluid_mask(obstacle, bnd)
    opn = _opn(obstacle, bnd, bits)
    keys = ("out", "branch", "cell", "fwd", "cor", "orig")
    rec = {k: [] for k in keys}
    for a in range(D):
        orig = vel[..., a].astype(dtype)
        du = sref.face_displacement(vel, a, dt, dtype)
        traced = inter | high_face_mask(shape, bnd, bits, a)[None]
        fwd = np.where(traced, _trace(orig, du, +1, dtype), dtype(0)).astype(dtype)
        if order == 1:
            vals = dict(out=fwd, branch=np.where(traced, FWD, BAND), cell=np.zeros(orig.shape, np.int64), fwd=fwd, cor=fwd, orig=orig)
        else:
            live = live_mask(fluid, opn, a)
            bwd = _trace(fwd, du, -1, dtype)
            cor = (fwd + dtype(0.5) * (orig - bwd)).astype(dtype)
            cells = aref._clamp_cells(shape, du, +1, dtype)
            mn = np.zeros(orig.shape, dtype); mx = np.zeros(orig.shape, dtype); found = np.zeros(orig.shape, bool)
            mn, mx, found = oref._corner_range(orig, cells, fluid, mn, mx, found)
            flat = np.ravel_multi_index(tuple(np.broadcast_to(c, orig.shape) for c in reversed(cells)), shape)
            if clamp_mode == 1:
                cells2 = aref._clamp_cells(shape, du, -1, dtype)
                mn, mx, found = oref._corner_range(orig, cells2, fluid, mn, mx, found)
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
            out = np.where(live, val, fwd).astype(dtype)             # fwd is 0 wherever it was not traced
            vals = dict(out=out, branch=np.where(live, br, np.where(traced, FWD, BAND)), cell=np.where(live, flat, 0), fwd=fwd, cor=cor,
                        orig=orig)
        for k in keys:
            rec[k].append(vals[k])
    rec = {k: np.concatenate(v, axis=0) for k, v in rec.items()}
    rec["vel"] = stacked_to_vel(rec["out"], D)
    rec["D"] = D
    return rec


mac_alternatives = oref.mac_alternatives          # fwd | cor and the fluid corners of the reachable clamp cells: open sides change neither


# ---- walls and buoyancy, pressure ------------------------------------------------------------------------------------------------------------
def wall_buoyancy(vel, rho, force, obstacle, bits, bnd=1, dtype=np.float64):
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype); rho = rho.astype(dtype)
    nd = vel.ndim - 2
    fluid = fluid_mask(obstacle, bnd)
    opn = _opn(obstacle, bnd, bits)
    out = np.zeros_like(vel)
    for a in range(vel.shape[-1]):
        val = vel[..., a] + (dtype(0.5) * dtype(np.float32(force[a]))) * (rho + np.roll(rho, 1, axis=_ax(nd, a)))
        keep = live_mask(fluid, opn, a) | opn                        # live without the term, or an open cell's filled value
        out[..., a] = np.where(both_mask(fluid, a), val, np.where(keep, vel[..., a], dtype(0)))
    return out


rhs = oref.rhs                                    # b is unchanged


def neighbour_count(obstacle, bits, bnd=1):
    """n_c = fluid neighbours + open neighbours, on fluid cells"""
    fluid = fluid_mask(obstacle, bnd)
    opn = _opn(obstacle, bnd, bits)
    cnt = np.zeros(fluid.shape, np.int64)
    for a in range(fluid.ndim - 1):
        for sh in (1, -1):
            cnt = cnt + (fluid & (_shift(fluid, a, sh) | _shift(opn, a, sh)))
    return cnt


def apply_A(x, obstacle, bits, bnd=1):
    """(A x)[c] = n_c x[c] - sum over FLUID neighbours (x-, x+, y-, y+, z-, z+); p = 0 in open cells.  Keeps x's dtype."""
    dtype = x.dtype.type
    nd = x.ndim - 1
    fluid = fluid_mask(obstacle, bnd)
    s = np.zeros_like(x)
    for a in range(nd):
        for sh in (1, -1):
            ok = fluid & _shift(fluid, a, sh)
            s = s + np.where(ok, np.roll(x, sh, axis=_ax(nd, a)), dtype(0))
    return np.where(fluid, neighbour_count(obstacle, bits, bnd).astype(dtype) * x - s, dtype(0)).astype(dtype)


def cg(vel, obstacle, bits, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64, dot=None, amax=None):
    """smoke_obs_ref.cg with the open-side n_c (``dot`` / ``amax`` as in smoke_ref.cg).  Returns (x, iterations [B], r)."""
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
            q = apply_A(pn, obstacle, bits, bnd)
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


def correct(vel, p, obstacle, bits, bnd=1, dtype=np.float64):
    """live faces: vel - (p[c] - p[c - e_a]) with p as the array holds it; open cells keep their other components; the rest 0"""
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype); p = p.astype(dtype)
    nd = vel.ndim - 2
    fluid = fluid_mask(obstacle, bnd)
    opn = _opn(obstacle, bnd, bits)
    out = np.zeros_like(vel)
    for a in range(vel.shape[-1]):
        val = vel[..., a] - (p - np.roll(p, 1, axis=_ax(nd, a)))
        out[..., a] = np.where(live_mask(fluid, opn, a), val, np.where(opn, vel[..., a], dtype(0)))
    return out


def extrapolate(vel, bits, bnd=1):
    """the zero-gradient fill: vel[c][a] = vel[c'][a] on open cells, c' = c clamped to [bnd, extent - bnd] along a and to
    [bnd, extent - bnd - 1] along every other axis.  Keeps vel's dtype; returns a new array."""
    shape = vel.shape[1:-1]
    nd = len(shape)
    opn = open_mask(shape, bnd, bits)[None]
    out = vel.copy()
    for a in range(vel.shape[-1]):
        idx = []
        for ax, n in enumerate(shape):
            b = nd - 1 - ax
            src = np.clip(np.arange(n), bnd, n - bnd - (0 if b == a else 1))
            sh = [1] * nd
            sh[ax] = n
            idx.append(src.reshape(sh))
        moved = vel[..., a][(slice(None),) + tuple(np.broadcast_arrays(*idx))]
        out[..., a] = np.where(opn, moved, vel[..., a])
    return out


def solve_pressure(vel, obstacle, bits, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64):
    x, iters, _ = cg(vel, obstacle, bits, bnd, accuracy, max_iter, dtype)
    return extrapolate(correct(vel, x, obstacle, bits, bnd, dtype), bits, bnd), x, iters


def dense_A(shape, bnd, obstacle, bits):
    """A over the fluid cells of ONE grid (obstacle [(Z,)Y,X]), fp64 [n, n], and the flat indices of those cells"""
    obstacle = np.asarray(obstacle)[None]
    cells = np.flatnonzero(fluid_mask(obstacle, bnd).ravel())
    n = cells.size
    A = np.zeros((n, n))
    for col in range(n):
        e = np.zeros((1,) + tuple(shape))
        e.reshape(-1)[cells[col]] = 1.0
        A[:, col] = apply_A(e, obstacle, bits, bnd).reshape(-1)[cells]
    return A, cells


def exact_projection(vel, obstacle, bits, bnd=1):
    """fp64, dense: the least-squares solution of A p = b per entry (A is singular once per fluid region that touches no open cell,
    which least squares copes with), and the projected, filled velocity.  Small grids only."""
    vel = vel.astype(np.float64)
    shape = vel.shape[1:-1]
    b = rhs(vel, obstacle, bnd, np.float64)
    p = np.zeros_like(b)
    for e in range(b.shape[0]):
        A, cells = dense_A(shape, bnd, obstacle[e], bits)
        assert A.shape[0] <= 1200, "exact_projection is for small grids"
        if cells.size:
            p[e].reshape(-1)[cells] = np.linalg.lstsq(A, b[e].reshape(-1)[cells], rcond=None)[0]
    return extrapolate(correct(vel, p, obstacle, bits, bnd, np.float64), bits, bnd), p


def divergence(vel, obstacle, bnd=1):
    return -rhs(vel, obstacle, bnd, np.float64)


# ---- the sphere stamp ------------------------------------------------------------------------------------------------------------------------
def sphere_source(density, centers, radius, value=1.0, dtype=np.float64):
    """out = value where ((i+.5-cx)^2 + (j+.5-cy)^2) [+ (k+.5-cz)^2] <= radius*radius, else density; centers [B,D]"""
    dtype = np.dtype(dtype).type
    d = density.astype(dtype)
    shape = d.shape[1:]
    nd = len(shape)
    centers = np.asarray(centers).astype(dtype)
    ex = (slice(None),) + (None,) * nd
    s = None
    with np.errstate(invalid="ignore"):
        for a in range(nd):
            t = (aref._cell_index(shape, a, dtype) + dtype(0.5)) - centers[:, a][ex]
            s = t * t if s is None else s + t * t
        hit = s <= dtype(radius) * dtype(radius)                     # a NaN centre compares false
    return np.where(hit, dtype(value), d).astype(dtype)


# ---- the whole step --------------------------------------------------------------------------------------------------------------------------
def step(density, vel, dt, obstacle, bits, source=None, force=None, order=2, clamp_mode=2, bnd=1, accuracy=1e-4, max_iter=None,
         dtype=np.float64):
    """The statements of scene/smoke3_mov.py's loop.  ``source``: a mask, or (centers [B,D], radius).  Returns (density, vel)."""
    dtype = np.dtype(dtype).type
    shape = density.shape[1:]
    force = sref.default_force(shape, dt) if force is None else force
    if max_iter is None:
        max_iter = int(10 * max(shape)) * (1 if len(shape) == 3 else 4)
    mask = source
    if isinstance(source, tuple):
        density, mask = sphere_source(density, source[0], source[1], 1.0, dtype), None
    rd = oref.advect_density(density, vel, dt, obstacle, order=order, clamp_mode=clamp_mode, bnd=bnd, source=mask, dtype=dtype)
    rv = mac_advect(vel, dt, obstacle, bits, order=order, clamp_mode=clamp_mode, bnd=bnd, dtype=dtype)
    v = extrapolate(rv["vel"], bits, bnd)
    v = wall_buoyancy(v, rd["out"], force, obstacle, bits, bnd, dtype)
    v, _, _ = solve_pressure(v, obstacle, bits, bnd, accuracy, max_iter, dtype)
    return rd["out"], v


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------
def obstacle_cases(shape, bnd):
    """smoke_obs_ref.obstacle_cases and two more: ``touch``, a block against the high-x band (it touches the x+ side when that is open),
    and ``chamber``, a closed shell of solid cells around two fluid cells in mid-grid: with any side open the box is split into a region
    that reaches an open side and one (the chamber) that does not."""
    out = dict(oref.obstacle_cases(shape, bnd))
    nd = len(shape)
    mid = tuple(n // 2 for n in shape)
    o = np.zeros(shape, np.uint8)
    sl = [slice(max(m - 1, bnd), m + 1) for m in mid]
    sl[-1] = slice(shape[-1] - bnd - 2, shape[-1] - bnd)
    o[tuple(sl)] = 1
    out["touch"] = o
    long_ax = int(np.argmax(shape))
    region, shell = [], []
    for ax in range(nd):
        lo, hi = (mid[ax] - 1, mid[ax] + 1) if ax == long_ax else (mid[ax], mid[ax] + 1)
        assert lo - 1 >= bnd and hi + 1 <= shape[ax] - bnd, (shape, bnd)
        region.append(slice(lo, hi)); shell.append(slice(lo - 1, hi + 1))
    o = np.zeros(shape, np.uint8)
    o[tuple(shell)] = 1
    o[tuple(region)] = 0
    out["chamber"] = o
    return out


def all_obstacles(shape, bnd):
    c = obstacle_cases(shape, bnd)
    names = sorted(c)
    return names, np.stack([c[n] for n in names])


def mixed_batch(shape, bnd):
    """B = 3, a different obstacle per entry: none, the block against the high-x band, the chamber"""
    c = obstacle_cases(shape, bnd)
    return np.stack([c["none"], c["touch"], c["chamber"]])


def solve_input(shape, bnd, obstacle, bits, seed=4, inflow=0.0):
    """a velocity whose non-live faces are 0, with some divergence: the input solve_pressure expects.  ``inflow`` is added to the y
    component everywhere before the walls: with an open side the b of a region then need not sum to zero (a net inflow)."""
    B = obstacle.shape[0]
    rng = np.random.RandomState(seed)
    vel = sref.make_velocity(shape, B=B, seed=seed, vmax=1.0)
    vel[..., 1] += np.float32(inflow)
    rho = rng.uniform(0, 1, (B,) + tuple(shape)).astype(np.float32)
    return wall_buoyancy(vel, rho, (0.0, 0.25, 0.0)[:len(shape)], obstacle, bits, bnd, np.float32)
