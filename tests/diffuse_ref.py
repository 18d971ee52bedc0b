"""NumPy restatement of the implicit velocity diffusion declared in include/deepfluids_hip.h (cgSolveDiffusion of the viscous liquid scene),
written from that definition and parametrised by dtype: float64 is the reference of the GPU tests, float32 -- the same operations in the
same order -- is the twin (op for op but for the dot products, which the GPU sums in workgroup order).  Also the system matrix and a dense
fp64 solve for small grids, and the viscous step built on tests/liquid_ref.py.  Plain helper, no fixtures.

Layout: velocity [B,(Z,)Y,X,D]; alpha [B], taken at its fp32 rounding in every dtype (the library holds it in fp32); the (entry, component)
pairs are solved as planar grids [B*D,(Z,)Y,X], pair e*D + a = component a of entry e."""
import numpy as np

import liquid_ref as lref
import particles_ref as pref
from smoke_ref import interior_mask


def _type(dtype):
    return np.dtype(dtype).type


def default_max_iter(shape):
    return int(max(shape)) * (1 if len(shape) == 3 else 4)


def planar(vel):
    """[B,..,D] -> [B*D,..]"""
    v = np.moveaxis(np.asarray(vel), -1, 1)
    return v.reshape((-1,) + v.shape[2:])


def interleaved(x, B):
    """[B*D,..] -> [B,..,D]"""
    x = x.reshape((B, -1) + x.shape[1:])
    return np.ascontiguousarray(np.moveaxis(x, 1, -1))


def pair_alpha(alpha, B, D, dtype):
    a = np.broadcast_to(np.asarray(alpha, np.float64), (B,)).astype(np.float32)
    return np.repeat(a, D).astype(dtype)


def neighbour_sum(x, mask=None):
    """the 2D axis neighbours of every cell in the order x-, x+, y-, y+[, z-, z+], summed from 0; with ``mask`` [..] only the neighbours
    inside it.  (np.roll wraps: only read at the cells of I, whose neighbours all exist.)"""
    nd = x.ndim - 1
    s = np.zeros_like(x)
    for a in range(nd):
        ax = x.ndim - 1 - a
        for sh in (1, -1):                                                 # roll by +1 brings c - e_a
            nb = np.roll(x, sh, axis=ax)
            if mask is not None:
                nb = np.where(np.roll(mask, sh, axis=ax - 1)[None], nb, x.dtype.type(0))
            s = (s + nb).astype(x.dtype)
    return s


def apply_A(x, alpha, bnd=1):
    """(A x)_c = x_c + alpha * (2D * x_c - sum_{nb in I} x_nb) on I, 0 off it; x [P,..], alpha [P]"""
    dtype = x.dtype.type
    nd = x.ndim - 1
    inter = interior_mask(x.shape[1:], bnd)
    al = alpha.reshape((-1,) + (1,) * nd).astype(x.dtype)
    q = x + al * (dtype(2 * nd) * x - neighbour_sum(x, inter))
    return np.where(inter[None], q, dtype(0)).astype(x.dtype)


def rhs(u, alpha, bnd=1):
    """b_c = u_c + alpha * sum_{nb not in I} u_nb on I, 0 off it"""
    dtype = u.dtype.type
    nd = u.ndim - 1
    inter = interior_mask(u.shape[1:], bnd)
    al = alpha.reshape((-1,) + (1,) * nd).astype(u.dtype)
    return np.where(inter[None], u + al * neighbour_sum(u, ~inter), dtype(0)).astype(u.dtype)


def first_residual(u, alpha, bnd=1):
    """r0 = b - A u from x0 = u, in the form the header writes: alpha * (sum of all 2D neighbours - 2D * u) on I, 0 off it"""
    dtype = u.dtype.type
    nd = u.ndim - 1
    inter = interior_mask(u.shape[1:], bnd)
    al = alpha.reshape((-1,) + (1,) * nd).astype(u.dtype)
    return np.where(inter[None], al * (neighbour_sum(u) - dtype(2 * nd) * u), dtype(0)).astype(u.dtype)


def _dot(a, b):
    return (a * b).reshape(a.shape[0], -1).sum(axis=1, dtype=a.dtype)


def cg(vel, alpha, bnd=1, accuracy=1e-4, max_iter=None, dtype=np.float64, dot=None, amax=None):
    """The iteration of the header, every (entry, component) pair on its own.  Returns (vel_out [B,..,D], iterations [B,D], r [B*D,..],
    x [B*D,..]); cells off I keep the input's bits.  ``dot`` / ``amax``: the reductions (defaults: NumPy's sum and max); with
    cg_ref.ordered_dot / ordered_amax and float32 the run is the kernels' twin bit for bit."""
    dot = _dot if dot is None else dot
    amax = lref._amax if amax is None else amax
    dtype = _type(dtype)
    B, D = vel.shape[0], vel.shape[-1]
    max_iter = default_max_iter(vel.shape[1:-1]) if max_iter is None else max_iter
    u = planar(vel).astype(dtype)
    al = pair_alpha(alpha, B, D, dtype)
    inter = interior_mask(u.shape[1:], bnd)[None]
    P = u.shape[0]
    ex = (slice(None),) + (None,) * (u.ndim - 1)
    x = u.copy()
    r = first_residual(u, al, bnd)
    p = r.copy()
    rr_old = np.ones(P, dtype)
    active = np.ones(P, bool)
    iters = np.zeros(P, np.int32)
    k = 0
    while True:
        rr = dot(r, r)
        mx = amax(r)
        with np.errstate(invalid="ignore"):
            active = active & (mx > dtype(accuracy)) & (rr > 0) & (iters < max_iter)
        if not active.any():
            break
        with np.errstate(all="ignore"):
            beta = np.zeros(P, dtype) if k == 0 else (rr / rr_old).astype(dtype)
            pn = (r + beta[ex] * p).astype(dtype)
            q = apply_A(pn, al, bnd)
            pq = dot(pn, q)
            step = np.where(pq > 0, rr / pq, dtype(0)).astype(dtype)
        a_ = active[ex] & inter
        x = np.where(a_, x + step[ex] * pn, x).astype(dtype)
        r = np.where(a_, r - step[ex] * q, r).astype(dtype)
        p = np.where(active[ex], pn, p)
        rr_old = np.where(active, rr, rr_old)
        iters = iters + active
        k += 1
    return interleaved(x, B), iters.reshape(B, D), r, x


def matrices(shape, alpha, bnd=1):
    """fp64, one pair: (A [n,n] on the cells of I, G [n,m] the coupling to the m cells off I so that b = u_I + G u_band, cells of I, cells
    off I), assembled by applying the restatement to unit vectors.  Small grids only."""
    inter = interior_mask(shape, bnd)
    cells, band = np.flatnonzero(inter.ravel()), np.flatnonzero(~inter.ravel())
    n, m = cells.size, band.size
    assert n <= 1500, "matrices is for small grids"
    al = np.array([np.float64(np.float32(alpha))])
    A = np.zeros((n, n))
    for col in range(n):
        e = np.zeros((1,) + tuple(shape))
        e.reshape(-1)[cells[col]] = 1.0
        A[:, col] = apply_A(e, al, bnd).reshape(-1)[cells]
    G = np.zeros((n, m))
    for col in range(m):
        e = np.zeros((1,) + tuple(shape))
        e.reshape(-1)[band[col]] = 1.0
        G[:, col] = rhs(e, al, bnd).reshape(-1)[cells]
    return A, G, cells, band


def dense(vel, alpha, bnd=1):
    """fp64: the exact solution of every pair's system, cells off I copied; [B,..,D]"""
    v = np.asarray(vel).astype(np.float64)
    B, D = v.shape[0], v.shape[-1]
    shape = v.shape[1:-1]
    u = planar(v)
    x = u.copy()
    for e in range(B):
        A, G, cells, band = matrices(shape, np.broadcast_to(np.asarray(alpha, np.float64), (B,))[e], bnd)
        for a in range(D):
            row = u[e * D + a].reshape(-1)
            x[e * D + a].reshape(-1)[cells] = np.linalg.solve(A, row[cells] + G @ row[band])
    return interleaved(x, B)


def residual(x_vel, vel, alpha, bnd=1):
    """fp64 b - A x of a solution [B,..,D] for the input [B,..,D]; [B*D,..]"""
    B, D = vel.shape[0], vel.shape[-1]
    al = pair_alpha(alpha, B, D, np.float64)
    inter = interior_mask(vel.shape[1:-1], bnd)[None]
    xi = np.where(inter, planar(x_vel).astype(np.float64), 0.0)
    return rhs(planar(vel).astype(np.float64), al, bnd) - apply_A(xi, al, bnd)


# ---- the viscous step (scene/liquid3_vis.py:256-296) on tests/liquid_ref.py ---------------------------------------------------------------------
def step(pos, pvel, vel, dt, alpha, force=None, bnd=1, accuracy=1e-4, max_iter=None, flip_ratio=0.97, dtype=np.float64):
    """liquid_ref.step with, after the liquid cells are marked, setWallBcs as a zero-force pass of ``forces`` (wall faces 0, + 0 on the
    faces of liquid cells, the rest copied) and the diffusion at the step's accuracy and its own default iteration cap."""
    dtype = _type(dtype)
    shape = vel.shape[1:-1]
    B = pos.shape[0]
    force = lref.default_force(shape, dt) if force is None else force
    p = pref.trace(pos, vel, dt, bnd, 1.0, dtype)
    p, u, cell_start, _ = lref.sort_particles_any(p, np.asarray(pvel).astype(dtype), shape)
    v, w, known = lref.p2g(p, u, cell_start, shape, dtype)
    v_old = v.copy()
    v, _ = lref.extrapolate(v, known, 2, bnd, dtype)
    liquid = lref.liquid_mask(cell_start, B, shape, bnd)
    _, touch = lref.flags_of(liquid)
    v = lref.forces(v, liquid, (0.0,) * len(shape), bnd, dtype)
    v, diters, _, _ = cg(v, alpha, bnd, accuracy, default_max_iter(shape), dtype)
    v = lref.forces(v, liquid, force, bnd, dtype)
    v, pr, iters = lref.solve_pressure(v, liquid, bnd, accuracy, max_iter, dtype)
    v, _ = lref.extrapolate(v, touch, 4, bnd, dtype)
    u = lref.flip_update(p, u, v, v_old, flip_ratio, dtype)
    return dict(pos=p, pvel=u, vel=v, liquid=liquid, cell_start=cell_start, iters=iters, diters=diters, pressure=pr)
