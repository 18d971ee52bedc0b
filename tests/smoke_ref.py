"""NumPy restatement of the smoke solver step declared in include/deepfluids_hip.h (MAC self-advection, walls and buoyancy, conjugate
gradient pressure projection), written from that definition and parametrised by dtype like advect_ref.py: float64 is the reference of
the GPU tests, float32 -- the same operations in the same order, except that dot products are NumPy sums -- is the twin whose distance
from float64 sets their tolerance.  Also an exact fp64 projection for small grids (dense least squares).  Plain helper, no fixtures.

Layout: density / pressure [B,(Z,)Y,X], velocity [B,(Z,)Y,X,D], cell (i,j,k) = [..,k,j,i].  Axis a = 0, 1, 2 below means x, y, z."""
import numpy as np

import advect_ref as aref
from advect_ref import BAND, COR, FWD, NOCORNER, interior_mask  # noqa: F401


def _ax(nd, a):
    """array axis (in [B,(Z,)Y,X]) of grid axis a"""
    return nd - a


def face_mask(shape, bnd, a):
    """[(Z,)Y,X] bool: component a of cell c is kept -- c and c - e_a are both interior"""
    inter = interior_mask(shape, bnd)
    return inter & np.roll(inter, 1, axis=len(shape) - 1 - a)


# ---- 1. MAC self-advection ---------------------------------------------------------------------------------------------------------------
def face_displacement(vel, a, dt, dtype):
    """dt * uface_a per axis (list over x, y[, z]) on every cell; only interior cells are meaningful (neighbours are rolled)."""
    vel = vel.astype(dtype)
    D = vel.shape[-1]
    nd = vel.ndim - 2
    out = []
    for b in range(D):
        v = vel[..., b]
        if b == a:
            u = v
        else:
            lo = np.roll(v, 1, axis=_ax(nd, a))                      # c - e_a
            hi = np.roll(v, -1, axis=_ax(nd, b))                     # c + e_b
            lohi = np.roll(lo, -1, axis=_ax(nd, b))                  # c - e_a + e_b
            u = dtype(0.25) * (((v + lo) + hi) + lohi)
        out.append(dtype(dt) * u)
    return out


def mac_advect(vel, dt, order=2, clamp_mode=2, bnd=1, dtype=np.float64):
    """The velocity carried through itself.  Returns a record like advect_ref.step's with the D components stacked along the batch axis
    (component-major: row a*B + b), so that advect_ref.twin_error / compare apply; ``vel`` of the record is the result [B,..,D]."""
    dtype = np.dtype(dtype).type
    assert order in (1, 2) and clamp_mode in (1, 2) and bnd >= 1
    shape = vel.shape[1:-1]
    D = vel.shape[-1]
    assert D == len(shape) and all(2 * bnd + 2 <= n for n in shape)
    nd = len(shape)
    inter = np.broadcast_to(interior_mask(shape, bnd)[None], vel.shape[:-1])
    keys = ("out", "branch", "cell", "fwd", "cor", "orig")
    rec = {k: [] for k in keys}
    for a in range(D):
        orig = vel[..., a].astype(dtype)
        du = face_displacement(vel, a, dt, dtype)
        fwd = aref.semi_lagrange(orig, du, +1, bnd, dtype)
        if order == 1:
            vals = dict(out=fwd, branch=np.where(inter, FWD, BAND), cell=np.zeros(orig.shape, np.int64), fwd=fwd, cor=fwd, orig=orig)
        else:
            both = np.broadcast_to(face_mask(shape, bnd, a)[None], orig.shape)
            bwd = aref.semi_lagrange(fwd, du, -1, bnd, dtype)
            cor = (fwd + dtype(0.5) * (orig - bwd)).astype(dtype)
            cells = aref._clamp_cells(shape, du, +1, dtype)
            mn = np.zeros(orig.shape, dtype); mx = np.zeros(orig.shape, dtype); found = np.zeros(orig.shape, bool)
            mn, mx, found = aref._corner_range(orig, cells, bnd, mn, mx, found)
            flat = np.ravel_multi_index(tuple(np.broadcast_to(c, orig.shape) for c in reversed(cells)), shape)
            if clamp_mode == 1:
                cells2 = aref._clamp_cells(shape, du, -1, dtype)
                mn, mx, found = aref._corner_range(orig, cells2, bnd, mn, mx, found)
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
            out = np.where(both, val, fwd).astype(dtype)             # fwd is 0 on wall cells already
            vals = dict(out=out, branch=np.where(both, br, np.where(inter, FWD, BAND)), cell=np.where(both, flat, 0), fwd=fwd, cor=cor, orig=orig)
        for k in keys:
            rec[k].append(vals[k])
    rec = {k: np.concatenate(v, axis=0) for k, v in rec.items()}
    rec["vel"] = stacked_to_vel(rec["out"], D)
    rec["D"] = D
    return rec


def stacked_to_vel(x, D):
    """[D*B,..] component-major -> [B,..,D]"""
    B = x.shape[0] // D
    return np.stack([x[a * B:(a + 1) * B] for a in range(D)], axis=-1)


def vel_to_stacked(v):
    return np.concatenate([v[..., a] for a in range(v.shape[-1])], axis=0)


def mac_alternatives(r64, vel, dt, clamp_mode, bnd, near=1e-3):
    """``alt`` of advect_ref.compare for a mac_advect record: fwd | cor of the cell, and the values of the component at the interior
    corners of every clamp cell reachable by moving a trunc() whose argument lies within ``near`` of an integer."""
    import itertools
    D = r64["D"]
    B = r64["out"].shape[0] // D
    shape = r64["out"].shape[1:]
    ext = shape[::-1]
    inter = interior_mask(shape, bnd)
    dus = [face_displacement(vel, a, dt, np.float64) for a in range(D)]

    def alt(index):
        a, b = divmod(index[0], B)
        vidx = (b,) + tuple(index[1:])
        cand = [float(r64["fwd"][index]), float(r64["cor"][index])]
        ijk = index[1:][::-1]
        for sign in ((+1, -1) if clamp_mode == 1 else (+1,)):
            opts = []
            for ax in range(D):
                t = ijk[ax] - sign * float(dus[a][ax][vidx])
                c = {int(t)}
                if abs(t - round(t)) < near:
                    c |= {int(round(t)) - 1, int(round(t))}
                opts.append(sorted({min(max(v, 0), ext[ax] - 2) for v in c}))
            for cell in itertools.product(*opts):
                for off in itertools.product((0, 1), repeat=D):
                    idx = tuple(cell[ax] + off[ax] for ax in reversed(range(D)))
                    if inter[idx]:
                        cand.append(float(r64["orig"][(index[0],) + idx]))
        return cand
    return alt


# ---- 2. walls and buoyancy ------------------------------------------------------------------------------------------------------------------
def wall_buoyancy(vel, rho, force, bnd=1, dtype=np.float64):
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype); rho = rho.astype(dtype)
    shape = vel.shape[1:-1]
    nd = len(shape)
    out = np.zeros_like(vel)
    for a in range(vel.shape[-1]):
        keep = face_mask(shape, bnd, a)[None]
        val = vel[..., a] + (dtype(0.5) * dtype(np.float32(force[a]))) * (rho + np.roll(rho, 1, axis=_ax(nd, a)))
        out[..., a] = np.where(keep, val, dtype(0))
    return out


# ---- 3. pressure projection --------------------------------------------------------------------------------------------------------------------
def rhs(vel, bnd=1, dtype=np.float64):
    """b = -div on interior cells, 0 on wall cells"""
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype)
    shape = vel.shape[1:-1]
    nd = len(shape)
    div = None
    for a in range(vel.shape[-1]):
        t = np.roll(vel[..., a], -1, axis=_ax(nd, a)) - vel[..., a]
        div = t if div is None else div + t
    return np.where(interior_mask(shape, bnd)[None], -div, dtype(0)).astype(dtype)


def apply_A(x, bnd=1):
    """(A x)[c] = n_c x[c] - sum over interior neighbours in the order x-, x+, y-, y+, z-, z+; 0 on wall cells.  Keeps x's dtype."""
    dtype = x.dtype.type
    shape = x.shape[1:]
    nd = len(shape)
    inter = interior_mask(shape, bnd)
    s = np.zeros_like(x)
    cnt = np.zeros(shape, np.int64)
    for a in range(nd):
        for sh in (1, -1):                                           # roll by +1 brings c - e_a
            ok = inter & np.roll(inter, sh, axis=nd - 1 - a)
            s = s + np.where(ok[None], np.roll(x, sh, axis=_ax(nd, a)), dtype(0))
            cnt = cnt + ok
    return np.where(inter[None], cnt[None].astype(dtype) * x - s, dtype(0)).astype(dtype)


def _dot(a, b):
    return (a * b).reshape(a.shape[0], -1).sum(axis=1, dtype=a.dtype)


def _amax(r):
    return np.abs(r).reshape(r.shape[0], -1).max(axis=1)


def cg(vel, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64, dot=None, amax=None):
    """The iteration of the header, every batch entry on its own.  Returns (x, iterations [B], r).
    ``dot`` / ``amax``: the reductions (defaults: NumPy's sum and max); with cg_ref.ordered_dot / ordered_amax and
    float32 the run is the kernels' twin bit for bit."""
    dot = _dot if dot is None else dot
    dtype = np.dtype(dtype).type
    b = rhs(vel, bnd, dtype)
    B = b.shape[0]
    ex = (slice(None),) + (None,) * (b.ndim - 1)
    x = np.zeros_like(b); r = b.copy(); p = b.copy()
    rr_old = np.ones(B, dtype)
    active = np.ones(B, bool)
    iters = np.zeros(B, np.int32)
    k = 0
    while True:
        rr = dot(r, r)
        mx = _amax(r) if amax is None else amax(r)
        active = active & (mx > dtype(accuracy)) & (rr > 0) & (iters < max_iter)
        if not active.any():
            break
        with np.errstate(all="ignore"):
            beta = np.zeros(B, dtype) if k == 0 else (rr / rr_old).astype(dtype)
            pn = (r + beta[ex] * p).astype(dtype)
            q = apply_A(pn, bnd)
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


def correct(vel, p, bnd=1, dtype=np.float64):
    dtype = np.dtype(dtype).type
    vel = vel.astype(dtype); p = p.astype(dtype)
    shape = vel.shape[1:-1]
    nd = len(shape)
    out = np.zeros_like(vel)
    for a in range(vel.shape[-1]):
        keep = face_mask(shape, bnd, a)[None]
        out[..., a] = np.where(keep, vel[..., a] - (p - np.roll(p, 1, axis=_ax(nd, a))), dtype(0))
    return out


def solve_pressure(vel, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64):
    x, iters, _ = cg(vel, bnd, accuracy, max_iter, dtype)
    return correct(vel, x, bnd, dtype), x, iters


def dense_A(shape, bnd=1):
    """A over the interior cells of one grid, fp64 [n, n], and the flat indices of those cells"""
    inter = interior_mask(shape, bnd)
    cells = np.flatnonzero(inter.ravel())
    n = cells.size
    A = np.zeros((n, n))
    for col in range(n):
        e = np.zeros((1,) + tuple(shape))
        e.reshape(-1)[cells[col]] = 1.0
        A[:, col] = apply_A(e, bnd).reshape(-1)[cells]
    return A, cells


def exact_projection(vel, bnd=1):
    """fp64: the minimum-norm least-squares solution of A p = b per entry (dense), and the projected velocity.  Small grids only."""
    vel = vel.astype(np.float64)
    shape = vel.shape[1:-1]
    A, cells = dense_A(shape, bnd)
    assert A.shape[0] <= 1200, "exact_projection is for small grids"
    b = rhs(vel, bnd, np.float64)
    p = np.zeros_like(b)
    pinv = np.linalg.pinv(A)
    for e in range(b.shape[0]):
        p[e].reshape(-1)[cells] = pinv @ b[e].reshape(-1)[cells]
    return correct(vel, p, bnd, np.float64), p


def divergence(vel, bnd=1):
    return -rhs(vel, bnd, np.float64)


# ---- the whole step ----------------------------------------------------------------------------------------------------------------------------
def default_force(shape, dt, gravity=-4e-3):
    f = [0.0] * len(shape)
    f[1] = -gravity * dt * max(shape)
    return tuple(f)


def step(density, vel, dt, source=None, force=None, order=2, clamp_mode=2, bnd=1, accuracy=1e-4, max_iter=None, dtype=np.float64):
    """The seven statements.  Returns (density, vel, record of the density advection, record of the velocity advection)."""
    dtype = np.dtype(dtype).type
    shape = density.shape[1:]
    force = default_force(shape, dt) if force is None else force
    if max_iter is None:
        max_iter = int(10 * max(shape)) * (1 if len(shape) == 3 else 4)
    rd = aref.step(density, vel, dt, order=order, clamp_mode=clamp_mode, bnd=bnd, source=source, dtype=dtype)
    rv = mac_advect(vel, dt, order=order, clamp_mode=clamp_mode, bnd=bnd, dtype=dtype)
    v = wall_buoyancy(rv["vel"], rd["out"], force, bnd, dtype)
    v, _, _ = solve_pressure(v, bnd, accuracy, max_iter, dtype)
    return rd["out"], v, rd, rv


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
def make_velocity(shape, B=3, seed=0, vmax=3.0, noise=0.01):
    """smooth velocities [B,*shape,D] float32, up to ``vmax`` cells per unit time, so that traces reach the wall band"""
    rng = np.random.RandomState(seed)
    D = len(shape)
    v = np.zeros((B,) + tuple(shape) + (D,))
    for b in range(B):
        for a in range(D):
            f = aref._sines(rng, shape, 3, 1.0)
            f = f / np.abs(f).max() * vmax * rng.uniform(0.5, 1.0)
            v[b, ..., a] = f + noise * rng.standard_normal(shape)
    return v.astype(np.float32)


def make_density(shape, B=3, seed=0):
    return aref.make_fixture(shape, B=B, seed=seed)["density"]


# the shapes of the GPU tests: (shape, bnd values).  2-D (17,130): X not a multiple of 4, more than one workgroup per entry.
MAC_SHAPES = [((6, 6), (1,)), ((9, 7), (1,)), ((12, 10), (1, 2)), ((17, 130), (1, 2)), ((6, 6, 6), (1,)), ((7, 8, 6), (1,)), ((19, 10, 7), (1, 2))]
MAC_SEEDS = {}        # (shape, bnd, order, mode) -> seed where the default 0 lets the twin flip a branch (tuned on the CPU by the gate)
MAC_DT = 1.0


def mac_cases():
    """(name, vel, kwargs): orders 1 | 2, clamp modes 1 | 2, B = 3"""
    for shape, bnds in MAC_SHAPES:
        for bnd in bnds:
            for order, mode in ((1, 2), (2, 1), (2, 2)):
                seed = MAC_SEEDS.get((shape, bnd, order, mode), 0)
                vmax = min(3.0, 0.4 * min(shape))
                yield ("%s-o%d-m%d-b%d" % ("x".join(map(str, shape)), order, mode, bnd), make_velocity(shape, seed=seed, vmax=vmax),
                       dict(order=order, clamp_mode=mode, bnd=bnd))


def walled(vel, bnd):
    """a velocity with its wall faces zeroed: the input solve_pressure expects"""
    return wall_buoyancy(vel, np.zeros(vel.shape[:-1]), (0.0,) * vel.shape[-1], bnd, np.float32)
