"""NumPy restatement of the multigrid preconditioner for the liquid systems as declared in include/deepfluids_hip_liquid_mg.h: level 0 of
the free-surface, the ghost-fluid and the diffusion matrix as face weights, the coarser levels, and the preconditioned conjugate gradients
whose rows are level 0 -- parametrised by dtype: float64 is the reference, float32 the op-for-op twin whose bits the kernels of
liquid_mg.hip give.  The V-cycle, ``apply_A`` and the dense forms are smoke_mg_ref's (a level is w, dir, diag whatever system wrote it);
the systems themselves are liquid_ref's, liquid_gf_ref's and diffuse_ref's.  Plain helper, no fixtures.

``coarsen`` here restates mg_coarsen_kernel's order of additions (tot = 0; tot += low + high per axis; diag = tot + dir).
smoke_mg_ref.coarsen adds the same terms in another order, which gives the same bits only while every term is a small integer: the smoke
and the free-surface weights are, 1/theta and alpha are not.

Layout as in smoke_mg_ref: every array [B,(Z,)Y,X], axis a = 0, 1, 2 means x, y, z; a level is a dict ``w``, ``dir``, ``diag``."""
import numpy as np

import diffuse_ref as dref
import liquid_gf_ref as gref
import liquid_ref as lref
import smoke_mg_ref as mg
from liquid_gf_ref import DIRS
from liquid_ref import _shift
from smoke_mg_ref import ALPHA, _children, apply_A, dense_level, dense_M, vcycle  # noqa: F401
from smoke_ref import _amax, _dot, interior_mask


def _type(dtype):
    return np.dtype(dtype).type


# ---- level 0 ---------------------------------------------------------------------------------------------------------------------------------
def _air(liquid, bnd):
    """[2D, B, ..]: the neighbour in direction DIRS[n] of a liquid cell is interior by index and not liquid"""
    nd = liquid.ndim - 1
    inter = np.broadcast_to(interior_mask(liquid.shape[1:], bnd)[None], liquid.shape).copy()
    return np.stack([liquid & ~_shift(liquid, a, sh) & _shift(inter, a, sh) for a, sh in DIRS[:2 * nd]])


def level0_liquid(liquid, bnd=1, dtype=np.float64):
    """free surface: w = 1 between two liquid cells, dir = the air neighbours, diag = liquid neighbours + dir (small integers: exact)"""
    dtype = _type(dtype)
    nd = liquid.ndim - 1
    w = [(liquid & _shift(liquid, a, 1)).astype(dtype) for a in range(nd)]
    return mg._with_diag(w, _air(liquid, bnd).sum(axis=0).astype(dtype))


def level0_gf(liquid, phi, bnd=1, gf_clamp=1e-4, dtype=np.float64):
    """ghost fluid: w as above; dir = the sum from 0 of 1/theta over the air neighbours in the order of DIRS; diag = liquid_gf_ref.diagonal
    on the liquid (the chain of the init kernel, with its "1 if the sum is 0"), 0 off it"""
    dtype = _type(dtype)
    nd = liquid.ndim - 1
    w = [(liquid & _shift(liquid, a, 1)).astype(dtype) for a in range(nd)]
    it, air = gref.inv_theta(phi, liquid, bnd, gf_clamp, dtype)
    d = np.zeros(liquid.shape, dtype)
    for n in range(2 * nd):
        d = np.where(air[n], d + it[n], d).astype(dtype)
    diag = np.where(liquid, gref.diagonal(phi, liquid, bnd, gf_clamp, dtype), dtype(0)).astype(dtype)
    return dict(w=w, dir=d, diag=diag)


def level0_diffusion(shape, alpha, B, bnd=1, dtype=np.float64):
    """(I - alpha L) on I for the B*D pairs: w = alpha between two cells of I, dir = 1 + alpha * float(2D - cnt), diag = float(cnt) * alpha +
    dir, cnt the neighbours in I; 0 off I.  ``alpha``: a number or [B]."""
    dtype = _type(dtype)
    nd = len(shape)
    al = dref.pair_alpha(alpha, B, nd, dtype).reshape((-1,) + (1,) * nd)
    inter = np.broadcast_to(interior_mask(shape, bnd)[None], (B * nd,) + tuple(shape)).copy()
    w = [np.where(inter & _shift(inter, a, 1), al, dtype(0)).astype(dtype) for a in range(nd)]
    cnt = np.zeros(inter.shape, np.int64)
    for a, sh in DIRS[:2 * nd]:
        cnt = cnt + (inter & _shift(inter, a, sh))
    d = np.where(inter, dtype(1) + al * (2 * nd - cnt).astype(dtype), dtype(0)).astype(dtype)
    diag = np.where(inter, cnt.astype(dtype) * al + d, dtype(0)).astype(dtype)
    return dict(w=w, dir=d, diag=diag)


# ---- the coarser levels ----------------------------------------------------------------------------------------------------------------------
def coarsen(lev):
    """mg_coarsen_kernel: the Galerkin product over aggregates of 2^D children, in the kernel's order of additions"""
    nd = len(lev["w"])
    w = [_children(lev["w"][a], skip=a) for a in range(nd)]
    d = _children(lev["dir"])
    tot = np.zeros_like(d)
    for a in range(nd):
        tot = tot + (w[a] + _shift(w[a], a, -1))
    return dict(w=w, dir=d, diag=tot + d)


def hierarchy_from(lev0):
    levs = [lev0]
    while max(levs[-1]["diag"].shape[1:]) > 2:
        levs.append(coarsen(levs[-1]))
    return levs


def hierarchy_liquid(liquid, bnd=1, phi=None, gf_clamp=1e-4, dtype=np.float64):
    return hierarchy_from(level0_liquid(liquid, bnd, dtype) if phi is None else level0_gf(liquid, phi, bnd, gf_clamp, dtype))


def hierarchy_diffusion(shape, alpha, B, bnd=1, dtype=np.float64):
    return hierarchy_from(level0_diffusion(shape, alpha, B, bnd, dtype))


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------------
def pcg(r0, levs, x0=None, accuracy=1e-4, max_iter=100, alpha=ALPHA, precondition=True, dot=None, amax=None, stop_after=None):
    """smoke_mg_ref.pcg with the rows of ``levs[0]``: from x0 (default 0) and its residual r0, z = M r (``precondition=False``: z = r, plain
    conjugate gradients on the same rows), rr holds r.z, p = z + beta p, q = apply_A(levs[0], p); stops on the unscaled max|r|.  Keeps
    r0's dtype.  Returns (x, iterations [B], r, broke [B]); ``broke``: the entry ended on r.z <= 0 with max|r| above the accuracy.
    ``dot`` / ``amax`` as in smoke_ref.cg (cg_ref.ordered_dot / ordered_amax and float32: the kernels' twin).  ``stop_after``: at most
    that many iterations whatever the residual."""
    dot = _dot if dot is None else dot
    amax = _amax if amax is None else amax
    dtype = r0.dtype.type
    max_iter = max_iter if stop_after is None else min(max_iter, stop_after)
    B = r0.shape[0]
    ex = (slice(None),) + (None,) * (r0.ndim - 1)
    x = np.zeros_like(r0) if x0 is None else x0.astype(dtype).copy()
    r = r0.copy(); p = np.zeros_like(r0)
    rz_old = np.ones(B, dtype)
    active = np.ones(B, bool)
    broke = np.zeros(B, bool)
    iters = np.zeros(B, np.int32)
    k = 0
    while True:
        z = vcycle(levs, r, alpha) if precondition else r
        rz = dot(r, z)
        mx = amax(r)
        broke = broke | (active & (mx > dtype(accuracy)) & ~(rz > 0))
        active = active & (mx > dtype(accuracy)) & (rz > 0) & (iters < max_iter)
        if not active.any():
            break
        with np.errstate(all="ignore"):
            beta = np.zeros(B, dtype) if k == 0 else (rz / rz_old).astype(dtype)
            pn = (z + beta[ex] * p).astype(dtype)
            q = apply_A(levs[0], pn)
            pq = dot(pn, q)
            a_cg = np.where(pq > 0, rz / pq, dtype(0)).astype(dtype)
        a_ = active[ex]
        x = np.where(a_, x + a_cg[ex] * pn, x).astype(dtype)
        r = np.where(a_, r - a_cg[ex] * q, r).astype(dtype)
        p = np.where(a_, pn, p)
        rz_old = np.where(active, rz, rz_old)
        iters = iters + active
        k += 1
    return x, iters, r, broke


def solve_liquid(vel, liquid, phi=None, bnd=1, accuracy=1e-4, max_iter=None, gf_clamp=1e-4, dtype=np.float64, alpha=ALPHA, precondition=True,
                 dot=None, amax=None, stop_after=None):
    """the free-surface (``phi`` None) or ghost-fluid pressure solve.  Returns (p, iterations, r, broke)."""
    dtype = _type(dtype)
    max_iter = lref.default_max_iter(vel.shape[1:-1]) if max_iter is None else max_iter
    ph = None if phi is None else np.asarray(phi).astype(dtype)
    levs = hierarchy_liquid(liquid, bnd, ph, gf_clamp, dtype)
    return pcg(lref.rhs(vel, liquid, dtype), levs, None, accuracy, max_iter, alpha, precondition, dot, amax, stop_after)


def solve_diffusion(vel, alpha_v, bnd=1, accuracy=1e-4, max_iter=None, dtype=np.float64, alpha=ALPHA, precondition=True, dot=None, amax=None,
                    stop_after=None):
    """the diffusion of every (entry, component) pair from x = u.  Returns (vel_out [B,..,D], iterations [B,D], r [B*D,..], broke [B*D])."""
    dtype = _type(dtype)
    B, D = vel.shape[0], vel.shape[-1]
    shape = vel.shape[1:-1]
    max_iter = dref.default_max_iter(shape) if max_iter is None else max_iter
    u = dref.planar(vel).astype(dtype)
    levs = hierarchy_diffusion(shape, alpha_v, B, bnd, dtype)
    r0 = dref.first_residual(u, dref.pair_alpha(alpha_v, B, D, dtype), bnd)
    x, iters, r, broke = pcg(r0, levs, u, accuracy, max_iter, alpha, precondition, dot, amax, stop_after)
    return dref.interleaved(x, B), iters.reshape(B, D), r, broke


def viscous_step(pos, pvel, vel, dt, alpha, diffusion_max_iter, force=None, bnd=1, accuracy=1e-4, max_iter=None, flip_ratio=0.97,
                 dtype=np.float64):
    """diffuse_ref.step, statement for statement, with the diffusion's iteration cap as an argument: with a cap the plain recurrence never
    reaches it is the step whose diffusion runs to convergence, the yardstick for a solve that converges by another path"""
    dtype = _type(dtype)
    shape = vel.shape[1:-1]
    B = pos.shape[0]
    force = lref.default_force(shape, dt) if force is None else force
    p = dref.pref.trace(pos, vel, dt, bnd, 1.0, dtype)
    p, u, cell_start, _ = lref.sort_particles_any(p, np.asarray(pvel).astype(dtype), shape)
    v, w, known = lref.p2g(p, u, cell_start, shape, dtype)
    v_old = v.copy()
    v, _ = lref.extrapolate(v, known, 2, bnd, dtype)
    liquid = lref.liquid_mask(cell_start, B, shape, bnd)
    _, touch = lref.flags_of(liquid)
    v = lref.forces(v, liquid, (0.0,) * len(shape), bnd, dtype)
    v, diters, _, _ = dref.cg(v, alpha, bnd, accuracy, diffusion_max_iter, dtype)
    v = lref.forces(v, liquid, force, bnd, dtype)
    v, pr, iters = lref.solve_pressure(v, liquid, bnd, accuracy, max_iter, dtype)
    v, _ = lref.extrapolate(v, touch, 4, bnd, dtype)
    u = lref.flip_update(p, u, v, v_old, flip_ratio, dtype)
    return dict(pos=p, pvel=u, vel=v, liquid=liquid, cell_start=cell_start, iters=iters, diters=diters, pressure=pr)


# ---- the cases of the tests --------------------------------------------------------------------------------------------------------------------
GRIDS = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((34, 66), 1), ((66, 70), 1), ((6, 6, 6), 1), ((7, 8, 6), 1), ((19, 10, 7), 2), ((18, 22, 26), 1)]
RATIO_GRIDS = [((34, 66), 1), ((66, 70), 1), ((18, 22, 26), 1), ((48, 24, 48), 1)]      # host only: the grids of the issue's table
DIFFUSION_ALPHAS = (0.0, 0.23, 23.0, 230.0)
GEOMETRIES = ("pool_drop", "full", "none", "isolated", "batch3")


def pool_drop(shape, bnd=1):
    """[(Z,)Y,X] bool: a pool over the lower third and a drop above it"""
    inter = interior_mask(shape, bnd)
    nd = len(shape)
    idx = np.indices(shape)
    y = idx[nd - 2]
    liq = y < max(bnd + 1, shape[nd - 2] // 3)
    c = [n * f for n, f in zip(shape, ((0.5, 0.7, 0.4) if nd == 3 else (0.7, 0.4)))]
    rad = max(1.0, 0.15 * min(shape))
    d2 = sum((idx[a] - c[a]) ** 2 for a in range(nd))
    return (liq | (d2 <= rad * rad)) & inter


def geometry(name, shape, bnd=1):
    """[B,(Z,)Y,X] bool.  ``isolated``: entry 0 one isolated liquid cell beside a blob, entry 1 every interior cell liquid -- with walls at
    the border only, the one region that touches no air (singular but consistent)."""
    inter = interior_mask(shape, bnd)
    if name == "pool_drop":
        return pool_drop(shape, bnd)[None]
    if name == "full":
        return inter[None].copy()
    if name == "none":
        return np.zeros((1,) + tuple(shape), bool)
    if name == "isolated":
        a = np.zeros(shape, bool)
        a[tuple(bnd for _ in shape)] = True
        blob = tuple(slice(bnd + 2, max(bnd + 3, n - bnd - 1)) for n in shape)
        a[blob] = True
        return np.stack([a & inter, inter])
    if name == "batch3":
        return np.stack([pool_drop(shape, bnd), inter, geometry("isolated", shape, bnd)[0]])
    raise ValueError(name)


def velocity(shape, B, seed, bnd=1, scale=1.0):
    """a random velocity [B,..,D] with the wall faces 0 (what liquid_forces leaves)"""
    rng = np.random.RandomState(seed)
    nd = len(shape)
    v = (scale * rng.standard_normal((B,) + tuple(shape) + (nd,))).astype(np.float32)
    for a in range(nd):
        v[..., a] = np.where(lref.both_interior(shape, bnd, a)[None], v[..., a], np.float32(0))
    return v
