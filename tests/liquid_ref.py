"""NumPy restatement of the liquid solver step declared in include/deepfluids_hip.h (particles to grid, layer extrapolation, liquid
flags, gravity and walls, the free-surface projection, the FLIP update and the chained step), written from that definition and
parametrised by dtype: float64 is the reference of the GPU tests, float32 -- the same operations in the same order -- is the twin.  The
twin is op for op, and so bitwise, for everything but the conjugate-gradient solve, whose dot products the GPU sums in workgroup order.
Also a dense fp64 solve of the free-surface system for small grids.  Plain helper, no fixtures.

Layout: pos, pvel [B,N,D] (x, y[, z]); velocity, weight, marks [B,(Z,)Y,X,D]; flags [B,(Z,)Y,X]; cell (i,j,k) = [..,k,j,i]."""
import numpy as np

import particles_ref as pref
from smoke_ref import interior_mask

FLUID = 1


def _type(dtype):
    return np.dtype(dtype).type


def lo_bit(a):
    return 2 << (2 * a)


def hi_bit(a):
    return 4 << (2 * a)


def _ax(nd, a):
    """array axis of grid axis a (0 = x) in [B,(Z,)Y,X]"""
    return nd - a


# ---- particles: sort, sample ------------------------------------------------------------------------------------------------------------------
def sort_particles(pos, pvel, shape):
    """(pos_sorted, pvel_sorted, cell_start, order): the keys of the fp32 positions, sorted stably"""
    B, N, D = pos.shape
    ncell = int(np.prod(shape))
    order, cell_start = pref.cell_ranges(pref.cell_keys(pos, shape), B * ncell)
    return pos.reshape(-1, D)[order].reshape(B, N, D), pvel.reshape(-1, D)[order].reshape(B, N, D), cell_start, order


def sample(vel, pos, dtype):
    dtype = _type(dtype)
    return pref.mac_sample(np.asarray(vel).astype(dtype), np.asarray(pos).astype(dtype), 1.0, dtype)


def _reach(w, t):
    n, s0, s1 = w
    return np.where(n == t, s0, np.where(n + 1 == t, s1, s0.dtype.type(0)))


def p2g(pos, pvel, cell_start, shape, dtype=np.float64, normalise=True):
    """(vel, weight, known) of SORTED particles; with normalise=False vel is the numerator (the transpose of ``sample``)."""
    dtype = _type(dtype)
    B, N, D = pos.shape
    Z, Y, X = ((1,) + tuple(shape))[-3:]
    ext = (X, Y, Z)
    ncell = Z * Y * X
    p = np.asarray(pos).astype(dtype).reshape(-1, D)
    u = np.asarray(pvel).astype(dtype).reshape(-1, D)
    half = dtype(0.5)
    num = np.zeros((B, Z, Y, X, D), dtype)
    den = np.zeros((B, Z, Y, X, D), dtype)
    if N > 0:
        cell_start = pref.clamp_ranges(cell_start, B * N)                # the header's last sentence of the liquid solver block
        wc = [pref.axis_weights(p[:, b] - half, ext[b], dtype) for b in range(D)]
        wf = [pref.axis_weights(p[:, b], ext[b], dtype) for b in range(D)]
        for e in range(B):
            for k in range(Z):
                for j in range(Y):
                    for i in range(X):
                        own = (i, j, k)
                        rows = []
                        for z in range(max(k - 1, 0), min(k + 1, Z - 1) + 1):
                            for y in range(max(j - 1, 0), min(j + 1, Y - 1) + 1):
                                key = e * ncell + (z * Y + y) * X
                                s, t = cell_start[key + max(i - 1, 0)], cell_start[key + min(i + 1, X - 1) + 1]
                                if t > s:
                                    rows.append(np.arange(s, t))
                        if not rows:
                            continue
                        r = np.concatenate(rows)
                        for a in range(D):
                            w = None
                            for b in range(D):
                                src = wf[b] if b == a else wc[b]
                                wb = _reach((src[0][r], src[1][r], src[2][r]), own[b])
                                w = wb if w is None else (w * wb).astype(dtype)
                            # sequential sums from 0, in the order of the rows
                            num[e, k, j, i, a] = np.cumsum((w * u[r, a]).astype(dtype), dtype=dtype)[-1]
                            den[e, k, j, i, a] = np.cumsum(w, dtype=dtype)[-1]
    sh = (B,) + tuple(shape) + (D,)
    num, den = num.reshape(sh), den.reshape(sh)
    if not normalise:
        return num, den, (den > 0).astype(np.uint8)
    with np.errstate(all="ignore"):
        vel = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0)).astype(dtype)
    return vel, den, (den > 0).astype(np.uint8)


def face_weights(pos, shape, dtype=np.float64):
    """[N, D, 2^D] weights and flat face indices with which ``sample`` reads one entry's grid at pos [N,D] (for the host tests)"""
    dtype = _type(dtype)
    N, D = pos.shape
    ext = tuple(shape)[::-1]
    p = pos.astype(dtype)
    W = np.zeros((N, D, 2 ** D), dtype)
    I = np.zeros((N, D, 2 ** D), np.int64)
    for a in range(D):
        ws = [pref.axis_weights(p[:, b] - (dtype(0) if b == a else dtype(0.5)), ext[b], dtype) for b in range(D)]
        for c in range(2 ** D):
            w = np.ones(N, dtype)
            idx = np.zeros(N, np.int64)
            for b in reversed(range(D)):
                o = (c >> b) & 1
                w = w * (ws[b][2] if o else ws[b][1])
                idx = idx * ext[b] + ws[b][0] + o
            W[:, a, c] = w
            I[:, a, c] = idx * D + a
    return W, I


# ---- extrapolation ------------------------------------------------------------------------------------------------------------------------------
def both_interior(shape, bnd, a):
    """component a of cell c lies between two interior cells"""
    nd = len(shape)
    inter = interior_mask(shape, bnd)
    return inter & np.roll(inter, 1, axis=nd - 1 - a)


def extrapolate_layer(v, m, layer, bnd, dtype):
    """ONE layer of df_mac_extrapolate* from (v, m) of ``dtype`` / uint8; returns new arrays"""
    shape = v.shape[1:-1]
    nd = len(shape)
    vn, mn = v.copy(), m.copy()
    for a in range(nd):
        s = np.zeros(v.shape[:-1], dtype)
        cnt = np.zeros(v.shape[:-1], np.int64)
        for b in range(nd):
            for sh in (1, -1):                                       # roll by +1 brings c - e_b
                mk = np.roll(m[..., a], sh, axis=_ax(nd, b))
                ok = (mk >= 1) & (mk <= layer)
                with np.errstate(invalid="ignore"):
                    s = np.where(ok, s + np.roll(v[..., a], sh, axis=_ax(nd, b)), s).astype(dtype)
                cnt = cnt + ok
        fill = (m[..., a] == 0) & both_interior(shape, bnd, a)[None] & (cnt > 0)
        with np.errstate(all="ignore"):
            vn[..., a] = np.where(fill, s / np.maximum(cnt, 1).astype(dtype), v[..., a])
        mn[..., a] = np.where(fill, layer + 1, m[..., a])
    return vn, mn


def extrapolate(vel, mark, distance, bnd=1, dtype=np.float64):
    """``distance`` layers; returns (vel, marks)"""
    dtype = _type(dtype)
    v = np.asarray(vel).astype(dtype).copy()
    m = np.asarray(mark).astype(np.uint8).copy()
    for layer in range(1, int(distance) + 1):
        v, m = extrapolate_layer(v, m, layer, bnd, dtype)
    return v, m


# ---- flags, forces --------------------------------------------------------------------------------------------------------------------------------
def liquid_mask(cell_start, B, shape, bnd):
    n = (cell_start[1:] > cell_start[:-1]).reshape((B,) + tuple(shape))
    return n & interior_mask(shape, bnd)[None]


def _shift(m, a, sh):
    """m at c - sh*e_a, False outside the grid"""
    nd = m.ndim - 1
    out = np.roll(m, sh, axis=_ax(nd, a))
    idx = [slice(None)] * m.ndim
    idx[_ax(nd, a)] = 0 if sh == 1 else -1
    out[tuple(idx)] = False
    return out


def flags_of(liquid):
    """(flags [B,..] uint8, touch [B,..,D] uint8) of a liquid mask (interior cells only)"""
    nd = liquid.ndim - 1
    f = liquid.astype(np.uint8) * FLUID
    for a in range(nd):
        f = f | (_shift(liquid, a, 1).astype(np.uint8) * lo_bit(a)) | (_shift(liquid, a, -1).astype(np.uint8) * hi_bit(a))
    touch = np.stack([liquid | _shift(liquid, a, 1) for a in range(nd)], axis=-1).astype(np.uint8)
    return f.astype(np.uint8), touch


def live_face(liquid, bnd, a):
    """component a lies between two interior cells of which at least one is liquid"""
    return both_interior(liquid.shape[1:], bnd, a)[None] & (liquid | _shift(liquid, a, 1))


def forces(vel, liquid, force, bnd=1, dtype=np.float64):
    dtype = _type(dtype)
    v = np.asarray(vel).astype(dtype)
    out = np.zeros_like(v)
    shape = v.shape[1:-1]
    for a in range(len(shape)):
        kept = both_interior(shape, bnd, a)[None]
        out[..., a] = np.where(kept, np.where(live_face(liquid, bnd, a), v[..., a] + dtype(force[a]), v[..., a]), dtype(0))
    return out


# ---- free-surface projection --------------------------------------------------------------------------------------------------------------------
def rhs(vel, liquid, dtype=np.float64):
    dtype = _type(dtype)
    v = np.asarray(vel).astype(dtype)
    nd = v.ndim - 2
    div = None
    for a in range(nd):
        t = np.roll(v[..., a], -1, axis=_ax(nd, a)) - v[..., a]
        div = t if div is None else div + t
    return np.where(liquid, -div, dtype(0)).astype(dtype)


def apply_A(x, liquid, bnd=1):
    """(A x)[c] = n_c x[c] - sum over LIQUID neighbours (x-, x+, y-, y+, z-, z+), n_c = neighbours interior by index; 0 outside the liquid"""
    dtype = x.dtype.type
    shape = x.shape[1:]
    nd = len(shape)
    inter = interior_mask(shape, bnd)
    s = np.zeros_like(x)
    cnt = np.zeros(shape, np.int64)
    for a in range(nd):
        for sh in (1, -1):
            cnt = cnt + (inter & np.roll(inter, sh, axis=nd - 1 - a))
            s = s + np.where(_shift(liquid, a, sh), np.roll(x, sh, axis=_ax(nd, a)), dtype(0))
    return np.where(liquid, cnt[None].astype(dtype) * x - s, dtype(0)).astype(dtype)


def _dot(a, b):
    return (a * b).reshape(a.shape[0], -1).sum(axis=1, dtype=a.dtype)


def _amax(r):
    return np.abs(r).reshape(r.shape[0], -1).max(axis=1)


def cg(vel, liquid, bnd=1, accuracy=1e-4, max_iter=100, dtype=np.float64, dot=None, amax=None):
    """The iteration of the header on the liquid rows, every batch entry on its own.  Returns (x, iterations [B], r).
    ``dot`` / ``amax``: the reductions (defaults: NumPy's sum and max); with cg_ref.ordered_dot / ordered_amax and float32 the run is the
    kernels' twin bit for bit."""
    dot = _dot if dot is None else dot
    amax = _amax if amax is None else amax
    dtype = _type(dtype)
    b = rhs(vel, liquid, dtype)
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
            q = apply_A(pn, liquid, bnd)
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


def correct(vel, p, liquid, bnd=1, dtype=np.float64):
    dtype = _type(dtype)
    v = np.asarray(vel).astype(dtype); p = np.asarray(p).astype(dtype)
    shape = v.shape[1:-1]
    nd = len(shape)
    out = np.zeros_like(v)
    for a in range(nd):
        kept = both_interior(shape, bnd, a)[None]
        cor = v[..., a] - (p - np.roll(p, 1, axis=_ax(nd, a)))
        out[..., a] = np.where(kept, np.where(live_face(liquid, bnd, a), cor, v[..., a]), dtype(0))
    return out


def default_max_iter(shape):
    return int(10 * max(shape)) * (1 if len(shape) == 3 else 4)


def solve_pressure(vel, liquid, bnd=1, accuracy=1e-4, max_iter=None, dtype=np.float64):
    max_iter = default_max_iter(vel.shape[1:-1]) if max_iter is None else max_iter
    x, iters, _ = cg(vel, liquid, bnd, accuracy, max_iter, dtype)
    return correct(vel, x, liquid, bnd, dtype), x, iters


def exact_projection(vel, liquid, bnd=1):
    """fp64: the dense (minimum-norm least-squares, for a region that touches no air) solution of the free-surface system per entry, and
    the projected velocity.  Small grids only."""
    v = np.asarray(vel).astype(np.float64)
    b = rhs(v, liquid, np.float64)
    p = np.zeros_like(b)
    for e in range(b.shape[0]):
        cells = np.flatnonzero(liquid[e].ravel())
        n = cells.size
        assert n <= 1200, "exact_projection is for small grids"
        if n == 0:
            continue
        A = np.zeros((n, n))
        for col in range(n):
            u = np.zeros((1,) + liquid.shape[1:])
            u.reshape(-1)[cells[col]] = 1.0
            A[:, col] = apply_A(u, liquid[e:e + 1], bnd).reshape(-1)[cells]
        p[e].reshape(-1)[cells] = np.linalg.pinv(A) @ b[e].reshape(-1)[cells]
    return correct(v, p, liquid, bnd, np.float64), p


def divergence(vel, liquid):
    return -rhs(vel, liquid, np.float64)


# ---- FLIP update, the step ---------------------------------------------------------------------------------------------------------------------
def flip_update(pos, pvel, vel, vel_old, flip_ratio=0.97, dtype=np.float64):
    dtype = _type(dtype)
    flip = dtype(np.float32(flip_ratio))
    pic = dtype(np.float32(1.0) - np.float32(flip_ratio))          # rounded to fp32 once, as the host of the library does
    un = sample(vel, pos, dtype)
    d = un - sample(vel_old, pos, dtype)
    return (flip * (np.asarray(pvel).astype(dtype) + d) + pic * un).astype(dtype)


def default_force(shape, dt, gravity=-1e-3):
    f = [0.0] * len(shape)
    f[1] = float(gravity) * float(dt) * max(shape)
    return tuple(f)


def step(pos, pvel, vel, dt, force=None, bnd=1, accuracy=1e-4, max_iter=None, flip_ratio=0.97, dtype=np.float64):
    """One step.  The positions are traced in ``dtype`` and the keys are taken of their fp32 rounding.  Returns a dict: pos, pvel (sorted),
    vel, liquid, cell_start, iters."""
    dtype = _type(dtype)
    shape = vel.shape[1:-1]
    B = pos.shape[0]
    force = default_force(shape, dt) if force is None else force
    p = pref.trace(pos, vel, dt, bnd, 1.0, dtype)
    p, u, cell_start, _ = sort_particles_any(p, np.asarray(pvel).astype(dtype), shape)
    v, w, known = p2g(p, u, cell_start, shape, dtype)
    v_old = v.copy()
    v, _ = extrapolate(v, known, 2, bnd, dtype)
    liquid = liquid_mask(cell_start, B, shape, bnd)
    _, touch = flags_of(liquid)
    v = forces(v, liquid, force, bnd, dtype)
    v, pr, iters = solve_pressure(v, liquid, bnd, accuracy, max_iter, dtype)
    v, _ = extrapolate(v, touch, 4, bnd, dtype)
    u = flip_update(p, u, v, v_old, flip_ratio, dtype)
    return dict(pos=p, pvel=u, vel=v, liquid=liquid, cell_start=cell_start, iters=iters, pressure=pr)


def sort_particles_any(pos, pvel, shape):
    """sort_particles for positions of any dtype: keys of the fp32 rounding, the arrays keep their dtype"""
    B, N, D = pos.shape
    ncell = int(np.prod(shape))
    order, cell_start = pref.cell_ranges(pref.cell_keys(pos.astype(np.float32), shape), B * ncell)
    return pos.reshape(-1, D)[order].reshape(B, N, D), pvel.reshape(-1, D)[order].reshape(B, N, D), cell_start, order


def initial_velocity(shape, spheres, dtype=np.float32):
    """[*shape, D]: the y component is -1 on the faces whose centre lies inside one of the spheres (centre, radius), everything else 0"""
    D = len(shape)
    v = np.zeros(tuple(shape) + (D,), dtype)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")       # (z,) y, x indices
    for c, r in spheres:
        d2 = 0.0
        for a in range(D):
            g = grids[D - 1 - a] + (0.0 if a == 1 else 0.5)                                        # the y face: (i+.5, j[, k+.5])
            d2 = d2 + (g - float(c[a])) ** 2
        v[..., 1] = np.where(d2 <= float(r) ** 2, -1.0, v[..., 1])
    return v


def max_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.asarray(a).size else 0.0
