"""NumPy restatement of the liquid solver's surface as include/deepfluids_hip.h declares it (the averaged particle level set with its
smoothing passes and band, the ghost-fluid system, its Jacobi-preconditioned conjugate gradients, the correction, the step with
``ghost_fluid``), written from that definition and parametrised by dtype: float64 is the reference of the GPU tests, float32 -- the
same operations in the same order -- is the twin.  The twin is op for op, and so bitwise, for the level set; the solve's dot products
are summed in workgroup order on the GPU, so it is bounded through ``accuracy`` as tests/liquid_ref.py's is.  The definitions are this
project's own, restated from memory of mantaflow's averagedParticleLevelset and solvePressure(phi=); parity is with THIS file, NOT with
mantaflow.  Also the dense fp64 solve of the ghost-fluid system for small grids, and the inputs the host and GPU tests share.  Plain
helper, no fixtures.

Layout: pos [B,N,D] (x, y[, z]); velocity [B,(Z,)Y,X,D]; phi, flags, pressure [B,(Z,)Y,X]; cell (i,j,k) = [..,k,j,i]."""
import numpy as np

import liquid_ref as ref
import particles_ref as pref
from smoke_ref import interior_mask

_type = ref._type
_ax = ref._ax
_shift = ref._shift


# ---- the averaged level set ---------------------------------------------------------------------------------------------------------------------
def levelset_raw(pos_sorted, cell_start, shape, radius_factor=1.0, dtype=np.float64, parts=False):
    """phi before the smoothing passes, of SORTED particles; with ``parts`` also (wacc, pacc [..,D])"""
    dtype = _type(dtype)
    B, N, D = pos_sorted.shape
    ncell = int(np.prod(shape))
    sp = np.asarray(pos_sorted).astype(dtype).reshape(-1, D)
    R = pref.radius_of(D, radius_factor, dtype)
    r = int(R) + 1
    r4 = dtype(4) * (R * R)
    Z, Y, X = ((1,) + tuple(shape))[-3:]
    phi = np.full((B, Z, Y, X), R, dtype)
    wacc = np.zeros((B, Z, Y, X), dtype)
    pacc = np.zeros((B, Z, Y, X, D), dtype)
    half, one, zero = dtype(0.5), dtype(1), dtype(0)
    if N > 0:
        cell_start = pref.clamp_ranges(cell_start, B * N)                # the header's last sentence of the particle block
        for b in range(B):
            for k in range(Z):
                for j in range(Y):
                    for i in range(X):
                        c = np.array([dtype(i) + half, dtype(j) + half, dtype(k) + half][:D], dtype)
                        rows = []
                        for z in range(max(k - r, 0), min(k + r, Z - 1) + 1):
                            for y in range(max(j - r, 0), min(j + r, Y - 1) + 1):
                                key = b * ncell + (z * Y + y) * X
                                s, e = cell_start[key + max(i - r, 0)], cell_start[key + min(i + r, X - 1) + 1]
                                if e > s:
                                    rows.append(np.arange(s, e))
                        if not rows:
                            continue
                        q = sp[np.concatenate(rows)]
                        with np.errstate(invalid="ignore", over="ignore"):
                            d = c - q
                            s2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
                            if D == 3:
                                s2 = s2 + d[:, 2] * d[:, 2]
                            w = np.fmax(zero, one - s2 / r4).astype(dtype)
                            wa = np.cumsum(w, dtype=dtype)[-1]             # sequential sums from 0, in the order of the rows
                            pa = np.array([np.cumsum((w * q[:, a]).astype(dtype), dtype=dtype)[-1] for a in range(D)], dtype)
                            wacc[b, k, j, i] = wa
                            pacc[b, k, j, i] = pa
                            if wa > dtype(1e-6):
                                e_ = c - pa / wa
                                t = e_[0] * e_[0] + e_[1] * e_[1]
                                if D == 3:
                                    t = t + e_[2] * e_[2]
                                phi[b, k, j, i] = np.sqrt(t) - R
    sh = (B,) + tuple(shape)
    if parts:
        return phi.reshape(sh), wacc.reshape(sh), pacc.reshape(sh + (D,))
    return phi.reshape(sh)


def levelset_raw_brute(pos, shape, radius_factor=1.0):
    """fp64, independent of the sort and of the cell ranges: every cell looks at ALL particles of its entry and takes those whose own
    cell (of the fp32 position, clamped into the grid) lies within +-r of it on every axis.  The sums are NumPy's, not sequential: it
    agrees with ``levelset_raw`` to rounding, not bitwise."""
    p32 = np.asarray(pos, np.float32)
    B, N, D = p32.shape
    R = float(pref.radius_of(D, radius_factor, np.float64))
    r = int(R) + 1
    ext = tuple(shape)[::-1]
    p = p32.astype(np.float64)
    pc = np.stack([pref._cell_of(p32[..., a], ext[a]) for a in range(D)], axis=-1)       # [B,N,D]
    phi = np.full((B,) + tuple(shape), R)
    for b in range(B):
        for idx in np.ndindex(*shape):
            c = np.array(idx[::-1])
            near = (np.abs(pc[b] - c) <= r).all(axis=-1)
            q = p[b][near]
            if not len(q):
                continue
            x = c + 0.5
            w = np.maximum(0.0, 1.0 - ((x - q) ** 2).sum(axis=-1) / (4.0 * R * R))
            wa = w.sum()
            if wa > 1e-6:
                phi[(b,) + idx] = np.sqrt(((x - (w[:, None] * q).sum(axis=0) / wa) ** 2).sum()) - R
    return phi


def smooth_pass(phi, mode, band=0, bound_value=1.0):
    """one pass: mode 1 the (2D+1)-point average off the outermost layer, mode 2 the same kept where smaller, mode 0 a copy; then the band"""
    dtype = phi.dtype.type
    shape = phi.shape[1:]
    nd = len(shape)
    out = phi.copy()
    if mode:
        t = phi.copy()
        for a in range(nd):
            t = t + np.roll(phi, 1, axis=_ax(nd, a))
            t = t + np.roll(phi, -1, axis=_ax(nd, a))
        t = (t * (dtype(1) / dtype(2 * nd + 1))).astype(dtype)
        inner = interior_mask(shape, 1)[None]
        with np.errstate(invalid="ignore"):
            out = np.where(inner, t if mode == 1 else np.where(t < phi, t, phi), phi).astype(dtype)
    if band > 0:
        out = np.where(interior_mask(shape, band)[None], out, dtype(bound_value)).astype(dtype)
    return out


def levelset_averaged_sorted(pos_sorted, cell_start, shape, radius_factor=1.0, smooth=1, smooth_neg=1, bound_value=1.0, bnd=1,
                             dtype=np.float64):
    phi = levelset_raw(pos_sorted, cell_start, shape, radius_factor, dtype)
    passes = [1] * smooth + [2] * smooth_neg
    for n, mode in enumerate(passes):
        phi = smooth_pass(phi, mode, bnd if n == len(passes) - 1 else 0, bound_value)
    if not passes and bnd > 0:
        phi = smooth_pass(phi, 0, bnd, bound_value)
    return phi


def levelset_averaged(pos, shape, radius_factor=1.0, smooth=1, smooth_neg=1, bound_value=1.0, bnd=1, dtype=np.float64):
    """the keys are taken of the fp32 positions, the arithmetic runs in ``dtype``"""
    p32 = np.asarray(pos, np.float32)
    B, N, D = p32.shape
    order, cell_start = pref.cell_ranges(pref.cell_keys(p32, shape), B * int(np.prod(shape)))
    sp = p32.reshape(-1, D)[order].reshape(B, N, D)
    return levelset_averaged_sorted(sp, cell_start, shape, radius_factor, smooth, smooth_neg, bound_value, bnd, dtype)


# ---- the ghost-fluid system -----------------------------------------------------------------------------------------------------------------------
DIRS = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))           # (axis, roll shift): x-, x+, y-, y+, z-, z+


def inv_theta(phi, liquid, bnd=1, gf_clamp=1e-4, dtype=np.float64):
    """[2D, B, ..]: 1/theta of every liquid cell towards its x-, x+, y-, y+[, z-, z+] neighbour where that one is interior air, else 0;
    and the mask of those pairs"""
    dtype = _type(dtype)
    ph = np.asarray(phi).astype(dtype)
    shape = ph.shape[1:]
    nd = len(shape)
    inter = interior_mask(shape, bnd)[None]
    out, mask = [], []
    for a, sh in DIRS[:2 * nd]:
        pa = np.roll(ph, sh, axis=_ax(nd, a))
        air = liquid & ~_shift(liquid, a, sh) & _shift(np.broadcast_to(inter, liquid.shape).copy(), a, sh)
        with np.errstate(all="ignore"):
            denom = ph - pa
            theta = np.where(denom > dtype(-1e-4), dtype(0.5), np.fmin(np.fmax(ph / denom, dtype(gf_clamp)), dtype(1))).astype(dtype)
            it = (dtype(1) / theta).astype(dtype)
        out.append(np.where(air, it, dtype(0)).astype(dtype))
        mask.append(air)
    return np.stack(out), np.stack(mask)


def diagonal(phi, liquid, bnd=1, gf_clamp=1e-4, dtype=np.float64):
    """diag: from 0, in the order of DIRS, 1 per liquid neighbour and 1/theta per interior air neighbour; 1 where that is 0 or off the liquid"""
    dtype = _type(dtype)
    it, air = inv_theta(phi, liquid, bnd, gf_clamp, dtype)
    nd = liquid.ndim - 1
    dg = np.zeros(liquid.shape, dtype)
    for n, (a, sh) in enumerate(DIRS[:2 * nd]):
        dg = np.where(_shift(liquid, a, sh), dg + dtype(1), np.where(air[n], dg + it[n], dg)).astype(dtype)
    return np.where(liquid & (dg > 0), dg, dtype(1)).astype(dtype)


def apply_A(x, liquid, diag):
    """(A x)[c] = diag_c x[c] - sum over LIQUID neighbours, in the order of DIRS; 0 off the liquid"""
    dtype = x.dtype.type
    nd = x.ndim - 1
    s = np.zeros_like(x)
    for a, sh in DIRS[:2 * nd]:
        s = s + np.where(_shift(liquid, a, sh), np.roll(x, sh, axis=_ax(nd, a)), dtype(0))
    return np.where(liquid, diag * x - s, dtype(0)).astype(dtype)


def pcg(vel, liquid, phi, bnd=1, accuracy=1e-4, max_iter=100, gf_clamp=1e-4, dtype=np.float64, dot=None, amax=None):
    """The Jacobi-preconditioned iteration of the header on the liquid rows, every batch entry on its own (``dot`` / ``amax`` as in
    liquid_ref.cg).  Returns (x, iterations [B], r)."""
    dot = ref._dot if dot is None else dot
    amax = ref._amax if amax is None else amax
    dtype = _type(dtype)
    b = ref.rhs(vel, liquid, dtype)
    dg = diagonal(phi, liquid, bnd, gf_clamp, dtype)
    B = b.shape[0]
    ex = (slice(None),) + (None,) * (b.ndim - 1)
    x = np.zeros_like(b); r = b.copy(); z = (r / dg).astype(dtype); p = z.copy()
    rz_old = np.ones(B, dtype)
    active = np.ones(B, bool)
    iters = np.zeros(B, np.int32)
    k = 0
    while True:
        rz = dot(r, z)
        mx = amax(r)
        active = active & (mx > dtype(accuracy)) & (rz > 0) & (iters < max_iter)
        if not active.any():
            break
        with np.errstate(all="ignore"):
            beta = np.zeros(B, dtype) if k == 0 else (rz / rz_old).astype(dtype)
            pn = (z + beta[ex] * p).astype(dtype)
            q = apply_A(pn, liquid, dg)
            pq = dot(pn, q)
            alpha = np.where(pq > 0, rz / pq, dtype(0)).astype(dtype)
        a_ = active[ex]
        x = np.where(a_, x + alpha[ex] * pn, x).astype(dtype)
        r = np.where(a_, r - alpha[ex] * q, r).astype(dtype)
        z = np.where(a_, r / dg, z).astype(dtype)
        p = np.where(a_, pn, p)
        rz_old = np.where(active, rz, rz_old)
        iters = iters + active
        k += 1
    return x, iters, r


def correct(vel, p, liquid, phi, bnd=1, gf_clamp=1e-4, dtype=np.float64):
    dtype = _type(dtype)
    v = np.asarray(vel).astype(dtype); p = np.asarray(p).astype(dtype)
    shape = v.shape[1:-1]
    nd = len(shape)
    it, _ = inv_theta(phi, liquid, bnd, gf_clamp, dtype)
    out = np.zeros_like(v)
    for a in range(nd):
        kept = ref.both_interior(shape, bnd, a)[None]
        there = _shift(liquid, a, 1)                                   # c - e_a is liquid
        both = v[..., a] - (p - np.roll(p, 1, axis=_ax(nd, a)))
        here = v[..., a] - p * it[2 * a]                               # c liquid, c - e_a air: theta of c towards its low side
        low = v[..., a] + np.roll(p * it[2 * a + 1], 1, axis=_ax(nd, a))   # c - e_a liquid, c air: theta of c - e_a towards its high side
        cor = np.where(liquid & there, both, np.where(liquid, here, np.where(there, low, v[..., a])))
        out[..., a] = np.where(kept, cor, dtype(0))
    return out.astype(dtype)


def solve_pressure(vel, liquid, phi, bnd=1, accuracy=1e-4, max_iter=None, gf_clamp=1e-4, dtype=np.float64):
    max_iter = ref.default_max_iter(vel.shape[1:-1]) if max_iter is None else max_iter
    x, iters, _ = pcg(vel, liquid, phi, bnd, accuracy, max_iter, gf_clamp, dtype)
    return correct(vel, x, liquid, phi, bnd, gf_clamp, dtype), x, iters


def dense_matrix(liquid_e, phi_e, bnd=1, gf_clamp=1e-4):
    """fp64: (A [n,n], cells [n]) of ONE entry's ghost-fluid system"""
    liq = liquid_e[None]
    dg = diagonal(phi_e[None], liq, bnd, gf_clamp, np.float64)
    cells = np.flatnonzero(liquid_e.ravel())
    n = cells.size
    assert n <= 1200, "dense_matrix is for small grids"
    A = np.zeros((n, n))
    for col in range(n):
        u = np.zeros(liq.shape)
        u.reshape(-1)[cells[col]] = 1.0
        A[:, col] = apply_A(u, liq, dg).reshape(-1)[cells]
    return A, cells


def exact_projection(vel, liquid, phi, bnd=1, gf_clamp=1e-4):
    """fp64: the dense solution of the ghost-fluid system per entry (pinv: a region that touches no air is singular but consistent) and
    the projected velocity"""
    v = np.asarray(vel).astype(np.float64)
    b = ref.rhs(v, liquid, np.float64)
    p = np.zeros_like(b)
    for e in range(b.shape[0]):
        A, cells = dense_matrix(liquid[e], np.asarray(phi[e], np.float64), bnd, gf_clamp)
        if cells.size:
            p[e].reshape(-1)[cells] = np.linalg.pinv(A, rcond=1e-13) @ b[e].reshape(-1)[cells]
    return correct(v, p, liquid, phi, bnd, gf_clamp, np.float64), p


def residual(vel, p, liquid, phi, bnd=1, gf_clamp=1e-4):
    """fp64: b - A p"""
    dg = diagonal(phi, liquid, bnd, gf_clamp, np.float64)
    return ref.rhs(vel, liquid, np.float64) - apply_A(np.asarray(p).astype(np.float64), liquid, dg)


# ---- the step with ghost_fluid ------------------------------------------------------------------------------------------------------------------
def step(pos, pvel, vel, dt, force=None, bnd=1, accuracy=1e-4, max_iter=None, flip_ratio=0.97, radius_factor=1.0, gf_clamp=1e-4,
         dtype=np.float64):
    """liquid_ref.step with the averaged level set (smooth 1, smooth_neg 1, the bnd band 1.0) computed right after the liquid cells are
    marked and handed to the solve.  Returns the dict of liquid_ref.step and phi."""
    dtype = _type(dtype)
    shape = vel.shape[1:-1]
    B = pos.shape[0]
    force = ref.default_force(shape, dt) if force is None else force
    p = pref.trace(pos, vel, dt, bnd, 1.0, dtype)
    p, u, cell_start, _ = ref.sort_particles_any(p, np.asarray(pvel).astype(dtype), shape)
    v, w, known = ref.p2g(p, u, cell_start, shape, dtype)
    v_old = v.copy()
    v, _ = ref.extrapolate(v, known, 2, bnd, dtype)
    liquid = ref.liquid_mask(cell_start, B, shape, bnd)
    _, touch = ref.flags_of(liquid)
    phi = levelset_averaged_sorted(p, cell_start, shape, radius_factor, 1, 1, 1.0, bnd, dtype)
    v = ref.forces(v, liquid, force, bnd, dtype)
    v, pr, iters = solve_pressure(v, liquid, phi, bnd, accuracy, max_iter, gf_clamp, dtype)
    v, _ = ref.extrapolate(v, touch, 4, bnd, dtype)
    u = ref.flip_update(p, u, v, v_old, flip_ratio, dtype)
    return dict(pos=p, pvel=u, vel=v, liquid=liquid, cell_start=cell_start, iters=iters, pressure=pr, phi=phi)


# ---- inputs the host and the GPU tests share ------------------------------------------------------------------------------------------------
#               shape        B  bnd
LEVELSET_CASES = [((7, 9), 2, 1), ((16, 12), 1, 2), ((5, 7, 6), 2, 1)]
LEVELSET_N = 400


def levelset_positions(shape, B, bnd, seed):
    """[B,N,D] float32 in the manner of test_gpu_liquid.particle_set: the rows of particles_ref.special_positions (band cells, both clamp
    limits), one particle exactly on a cell centre, the rest in the lower-index 60 % of the grid so that the upper cells are empty; the
    LAST entry has ALL of its particles crowded into a single cell."""
    rng = np.random.RandomState(seed)
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    lo, hi = pref.clamp_bounds(shape, bnd, np.float32)
    p = (lo + rng.uniform(0, 1, size=(B, LEVELSET_N, D)) * (0.6 * (hi - lo))).astype(np.float32)
    sp = pref.special_positions(shape, bnd)
    p[:, :len(sp)] = sp
    p[:, len(sp)] = (np.floor(0.4 * ext) + 0.5).astype(np.float32)       # exactly on a cell centre
    if B > 1:
        p[-1] = (np.floor(0.5 * ext) + rng.uniform(0.01, 0.99, size=(LEVELSET_N, D))).astype(np.float32)
    return p


SOLVE_SHAPES = [(8, 8), (6, 6, 6), (17, 33), (9, 11, 7)]
GF_CLAMPS = (1e-4, 1e-2)


def ragged(shape, B, seed):
    """(liquid, vel) as test_gpu_liquid._ragged makes them"""
    rng = np.random.RandomState(seed)
    liquid = (rng.uniform(size=(B,) + shape) < 0.7) & interior_mask(shape, 1)[None]
    D = len(shape)
    vel = ref.forces(rng.standard_normal((B,) + shape + (D,)), liquid, (0.0, -0.25, 0.0)[:D], 1, np.float32)
    return liquid, vel.astype(np.float32)


def branch_phi(liquid, seed):
    """phi [B,..] float32 that sends the liquid/air pairs of ``liquid`` through every branch of theta: ordinary fractions (liquid in
    [-0.9, -0.1], air in [0.1, 0.9]); liquid cells at -1e-6 (their ratio falls below either gf_clamp); liquid cells at +0.05 (a
    negative ratio: the low clamp again); air cells at 0 or at -0.05, above their liquid neighbours but not positive (ratio >= 1: the
    high clamp); liquid cells at -2e-5 next to air at +3e-5 (denom > -1e-4: the fallback)."""
    rng = np.random.RandomState(seed)
    phi = np.where(liquid, -rng.uniform(0.1, 0.9, liquid.shape), rng.uniform(0.1, 0.9, liquid.shape))
    kind = rng.randint(0, 10, liquid.shape)
    phi = np.where(liquid & (kind == 0), -1e-6, phi)
    phi = np.where(liquid & (kind == 1), 0.05, phi)
    phi = np.where(~liquid & (kind == 2), 0.0, phi)
    phi = np.where(~liquid & (kind == 3), -0.05, phi)
    phi = np.where(liquid & (kind == 4), -2e-5, phi)
    phi = np.where(~liquid & (kind == 5), 3e-5, phi)
    return phi.astype(np.float32)


def theta_branches(phi, liquid, gf_clamp):
    """how many liquid/air pairs take each branch: (fallback, low clamp, high clamp, ordinary)"""
    it, air = inv_theta(phi, liquid, 1, gf_clamp, np.float64)
    nd = liquid.ndim - 1
    ph = np.asarray(phi, np.float64)
    fb = lo = hi = mid = 0
    for n, (a, sh) in enumerate(DIRS[:2 * nd]):
        denom = ph - np.roll(ph, sh, axis=_ax(nd, a))
        m = air[n]
        f = m & (denom > -1e-4)
        with np.errstate(all="ignore"):
            ratio = ph / denom
        fb += int(f.sum())
        lo += int((m & ~f & (ratio <= gf_clamp)).sum())
        hi += int((m & ~f & (ratio >= 1)).sum())
        mid += int((m & ~f & (ratio > gf_clamp) & (ratio < 1)).sum())
    return fb, lo, hi, mid


def solve_cases():
    """(name, liquid, vel, phi, gf_clamp) of every ghost-fluid solve the GPU tests run against the dense solve"""
    for n, shape in enumerate(SOLVE_SHAPES):
        liquid, vel = ragged(shape, 2, 3)
        phi = branch_phi(liquid, 40 + n)
        for c in GF_CLAMPS:
            yield "%s-%g" % ("x".join(str(s) for s in shape), c), liquid, vel, phi, c


def unit_theta_phi(liquid):
    """phi with every theta = 1: -1 in the liquid, 0 in the air"""
    return np.where(liquid, -1.0, 0.0).astype(np.float32)


HYDRO_SHAPES = [(10, 8), (6, 10, 6)]
HYDRO_S = (0.25, 0.5, 0.9)
HYDRO_G = -0.0625


def hydrostatic_case(shape, s, g=HYDRO_G):
    """A closed box whose lower rows are liquid, a flat surface ``s`` above the top liquid cell centres (phi = y_centre - y_surface), the
    velocity after a uniform vertical force g (``liquid_forces`` on zero).  Returns (liquid, vel, phi, depth): depth [1,..] of every
    liquid cell centre below the surface."""
    D = len(shape)
    Y = shape[-2]
    rows = Y // 2                                                       # liquid rows 1 .. rows - 1 (row 0 is wall)
    liquid = np.zeros((1,) + shape, bool)
    liquid[(slice(None),) * (D - 1) + (slice(0, rows),)] = True
    liquid &= interior_mask(shape, 1)[None]
    y_surface = (rows - 1) + 0.5 + s
    yc = pref._centre(shape, 1, np.float64)
    phi = np.broadcast_to(yc - y_surface, shape)[None].astype(np.float32)
    vel = ref.forces(np.zeros((1,) + shape + (D,)), liquid, (0.0, g, 0.0)[:D], 1, np.float32).astype(np.float32)
    depth = np.where(liquid, y_surface - np.broadcast_to(yc, shape)[None], 0.0)
    return liquid, vel, phi, depth


STEP_SHAPES = [(12, 16), (8, 10, 8)]
# seeds of the jitter, checked on the CPU (tests/test_liquid_gf_host.py): on all 4 steps the fp32 twin and the fp64 run sort every
# particle into the same cell and every solve stops below the iteration cap
STEP_SEEDS = {(12, 16): (123, 124), (8, 10, 8): (123, 124)}
