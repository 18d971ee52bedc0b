"""NumPy restatement of the multigrid preconditioner of the smoke pressure solve as declared in include/deepfluids_hip.h ("multigrid
preconditioner"): the hierarchy of face weights, the V-cycle z = M r and the preconditioned conjugate gradients, parametrised by dtype
-- float64 is the reference, float32 the op-for-op twin with the header's summation order, whose bits the kernels of multigrid.hip give
(no reductions across cells, fixed order, no contraction; the dot products of the iteration are NumPy sums as in the other twins).  Built
on smoke_obs_ref / smoke_open_ref for the level-0 matrix, the obstacle cases and ``solve_input``.  Plain helper, no fixtures.

Layout: every array [B,(Z,)Y,X]; axis a = 0, 1, 2 means x, y, z.  A level is a dict: ``w`` (list of D arrays, w[a][c] = the face between
c and c - e_a), ``dir``, ``diag``.  ``bits``: the open_sides int of smoke_open_ref."""
import numpy as np

import smoke_obs_ref as oref
import smoke_open_ref as pref
from smoke_obs_ref import _shift, fluid_mask
from smoke_ref import _amax, _dot

NU = 2
COARSEST_SWEEPS = 8
ALPHA = 1.8           # ops.DEFAULT_MG_ALPHA; chosen from the fp32 twin's iteration counts (profiles/smoke_mg.md)


def omega(dtype):
    return dtype(2) / dtype(3)


# ---- the hierarchy ---------------------------------------------------------------------------------------------------------------------------
def level0(obstacle, bnd, bits, dtype=np.float64):
    """the solve's own matrix as face weights: w_a = both cells fluid, dir = open neighbours of a fluid cell, diag = incident w + dir"""
    dtype = np.dtype(dtype).type
    obstacle = np.asarray(obstacle)
    nd = obstacle.ndim - 1
    fluid = fluid_mask(obstacle, bnd)
    opn = pref._opn(obstacle, bnd, bits)
    w = [(fluid & _shift(fluid, a, 1)).astype(dtype) for a in range(nd)]
    d = np.zeros(fluid.shape, dtype)
    for a in range(nd):
        for sh in (1, -1):
            d = d + (fluid & _shift(opn, a, sh)).astype(dtype)
    return _with_diag(w, d)


def _with_diag(w, d):
    diag = d.copy()
    for a in range(len(w)):
        diag = diag + w[a] + _shift(w[a], a, -1)             # the low face, and the high face (the neighbour's low face)
    return dict(w=w, dir=d, diag=diag)


def _pad_even(f):
    return np.pad(f, [(0, 0)] + [(0, n % 2) for n in f.shape[1:]])


def _children(f, skip=None):
    """the sum over the children of every aggregate, from 0 in ascending x, then y, then z (x innermost); ``skip``: the axis whose
    offset stays 0 (the faces with i_a = 2 I_a)"""
    f = _pad_even(f)
    nd = f.ndim - 1
    s = np.zeros((f.shape[0],) + tuple(n // 2 for n in f.shape[1:]), f.dtype)
    for dz in range(2 if nd == 3 else 1):
        for dy in range(2):
            for dx in range(2):
                d = (dx, dy, dz)[:nd]
                if skip is not None and d[skip] != 0:
                    continue
                idx = (slice(None),) + tuple(slice(d[a], None, 2) for a in reversed(range(nd)))
                s = s + f[idx]
    return s


def coarsen(lev):
    """the Galerkin product with piecewise-constant interpolation over aggregates of 2^D children"""
    w = [_children(lev["w"][a], skip=a) for a in range(len(lev["w"]))]
    return _with_diag(w, _children(lev["dir"]))


def hierarchy(obstacle, bnd, bits=0, dtype=np.float64):
    """the levels, level 0 first, until every extent is <= 2"""
    levs = [level0(obstacle, bnd, bits, dtype)]
    while max(levs[-1]["diag"].shape[1:]) > 2:
        levs.append(coarsen(levs[-1]))
    return levs


# ---- the V-cycle -----------------------------------------------------------------------------------------------------------------------------
def apply_A(lev, x):
    """diag x - sum, the sum from 0 in the order x-, x+, y-, y+[, z-, z+], each term w * x[neighbour] (a neighbour outside the grid adds an
    exact 0 here and is skipped by the kernels: the same bits)"""
    s = np.zeros_like(x)
    for a in range(len(lev["w"])):
        s = s + lev["w"][a] * _shift(x, a, 1)
        s = s + _shift(lev["w"][a], a, -1) * _shift(x, a, -1)
    return lev["diag"] * x - s


def _active(lev):
    return lev["diag"] > 0


def _safe_diag(lev):
    return np.where(_active(lev), lev["diag"], lev["diag"].dtype.type(1))


def first_sweep(lev, r):
    dtype = r.dtype.type
    return np.where(_active(lev), (omega(dtype) * r) / _safe_diag(lev), dtype(0)).astype(dtype)


def sweep(lev, r, x):
    dtype = r.dtype.type
    t = r - apply_A(lev, x)
    return np.where(_active(lev), x + (omega(dtype) * t) / _safe_diag(lev), dtype(0)).astype(dtype)


def residual(lev, r, x):
    return np.where(_active(lev), r - apply_A(lev, x), r.dtype.type(0)).astype(r.dtype)


def prolong(e, shape):
    for ax in range(1, e.ndim):
        e = np.repeat(e, 2, axis=ax)
    return e[(slice(None),) + tuple(slice(0, n) for n in shape)]


def vcycle(levs, r, alpha=ALPHA, l=0):
    """z = M r; keeps r's dtype"""
    dtype = r.dtype.type
    lev = levs[l]
    x = first_sweep(lev, r)
    if l == len(levs) - 1:
        for _ in range(COARSEST_SWEEPS - 1):
            x = sweep(lev, r, x)
        return x
    for _ in range(NU - 1):
        x = sweep(lev, r, x)
    rc = _children(residual(lev, r, x))
    e = vcycle(levs, rc, alpha, l + 1)
    x = np.where(_active(lev), x + dtype(np.float32(alpha)) * prolong(e, x.shape[1:]), dtype(0)).astype(dtype)
    for _ in range(NU):
        x = sweep(lev, r, x)
    return x


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------------
def pcg(vel, obstacle, bits=0, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64, alpha=ALPHA, precondition=True, dot=None, amax=None):
    """smoke_open_ref.cg with z = M r: rr holds r.z, p = z + beta p; stops on the unscaled max|r|.  ``precondition=False``: z = r, the
    plain solve.  Returns (x, iterations [B], r, broke [B]); ``broke``: the entry ended on r.z <= 0 with max|r| above the accuracy.
    ``dot`` / ``amax`` as in smoke_ref.cg."""
    dot = _dot if dot is None else dot
    amax = _amax if amax is None else amax
    dtype = np.dtype(dtype).type
    b = pref.rhs(vel, obstacle, bnd, dtype)
    levs = hierarchy(obstacle, bnd, bits, dtype) if precondition else None
    B = b.shape[0]
    ex = (slice(None),) + (None,) * (b.ndim - 1)
    x = np.zeros_like(b); r = b.copy(); p = np.zeros_like(b)
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
            q = pref.apply_A(pn, obstacle, bits, bnd)
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


def solve_pressure(vel, obstacle, bits=0, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64, alpha=ALPHA):
    x, iters, _, _ = pcg(vel, obstacle, bits, bnd, accuracy, max_iter, dtype, alpha)
    return pref.extrapolate(pref.correct(vel, x, obstacle, bits, bnd, np.dtype(dtype).type), bits, bnd), x, iters


def step(density, vel, dt, obstacle, bits, source=None, force=None, order=2, clamp_mode=2, bnd=1, accuracy=1e-4, max_iter=None,
         dtype=np.float64, precondition=True, alpha=ALPHA):
    """smoke_open_ref.step with the solve of this file (``precondition=False``: the plain solve).  Returns (density, vel)."""
    import smoke_ref as sref
    dtype = np.dtype(dtype).type
    shape = density.shape[1:]
    force = sref.default_force(shape, dt) if force is None else force
    if max_iter is None:
        max_iter = int(10 * max(shape)) * (1 if len(shape) == 3 else 4)
    rd = oref.advect_density(density, vel, dt, obstacle, order=order, clamp_mode=clamp_mode, bnd=bnd, source=source, dtype=dtype)
    rv = pref.mac_advect(vel, dt, obstacle, bits, order=order, clamp_mode=clamp_mode, bnd=bnd, dtype=dtype)
    v = pref.extrapolate(rv["vel"], bits, bnd)
    v = pref.wall_buoyancy(v, rd["out"], force, obstacle, bits, bnd, dtype)
    x, _, _, _ = pcg(v, obstacle, bits, bnd, accuracy, max_iter, dtype, alpha, precondition)
    return rd["out"], pref.extrapolate(pref.correct(v, x, obstacle, bits, bnd, dtype), bits, bnd)


# ---- dense forms, small grids only -------------------------------------------------------------------------------------------------------------
def dense_level(lev, e=0):
    """fp64 [n, n] of entry e of a level, over ALL its cells (inactive ones are zero rows)"""
    one = {k: ([w[e:e + 1].astype(np.float64) for w in v] if k == "w" else v[e:e + 1].astype(np.float64)) for k, v in lev.items()}
    shape = one["diag"].shape
    n = int(np.prod(shape))
    A = np.zeros((n, n))
    for col in range(n):
        x = np.zeros(n); x[col] = 1.0
        A[:, col] = apply_A(one, x.reshape(shape)).reshape(-1)
    return A


def dense_P(fine_shape):
    """piecewise-constant interpolation [n_fine, n_coarse] for one grid [(Z,)Y,X]"""
    coarse = tuple((n + 1) // 2 for n in fine_shape)
    idx = np.arange(int(np.prod(coarse))).reshape((1,) + coarse)
    parent = prolong(idx, fine_shape).reshape(-1)
    P = np.zeros((parent.size, idx.size))
    P[np.arange(parent.size), parent] = 1.0
    return P


def dense_M(levs, alpha=ALPHA, e=0):
    """fp64 [n, n]: the V-cycle of entry e column by column"""
    one = [{k: ([w[e:e + 1].astype(np.float64) for w in v] if k == "w" else v[e:e + 1].astype(np.float64)) for k, v in lev.items()} for lev in levs]
    shape = one[0]["diag"].shape
    n = int(np.prod(shape))
    M = np.zeros((n, n))
    for col in range(n):
        r = np.zeros(n); r[col] = 1.0
        M[:, col] = vcycle(one, r.reshape(shape), alpha).reshape(-1)
    return M
