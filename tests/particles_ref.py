"""NumPy restatement of the liquid step declared in include/deepfluids_hip.h (MAC sample, RK4 trace with clamp, cell keys and ranges,
union level set, l_adv image), written from that definition and parametrised by dtype: float64 is the reference of the GPU tests,
float32 -- the same operations in the same order -- is the twin whose distance from float64 sets their tolerance.  Plain helper, no
fixtures.

Layout: pos [B,N,D] in cell units (x, y[, z]); velocity [B,(Z,)Y,X,D]; phi [B,(Z,)Y,X]; cell (i,j,k) = [..,k,j,i].  Axis a = 0, 1, 2
below means x, y, z."""
import numpy as np


def _type(dtype):
    return np.dtype(dtype).type


def axis_weights(q, ext, dtype):
    """q < 0 or NaN -> (0; 1, 0); trunc(q) >= ext - 1 -> (ext - 2; 0, 1); else n = (int)q, s1 = q - n, s0 = 1 - s1."""
    with np.errstate(invalid="ignore"):
        low = ~(q >= 0)
        high = ~low & (q >= dtype(ext - 1))
        n = np.where(low | high, 0, q).astype(np.int64)
    s1 = q - n.astype(dtype)
    s0 = dtype(1) - s1
    n = np.where(low, 0, np.where(high, ext - 2, n))
    s0 = np.where(low, dtype(1), np.where(high, dtype(0), s0)).astype(dtype)
    s1 = np.where(low, dtype(0), np.where(high, dtype(1), s1)).astype(dtype)
    return n, s0, s1


def mac_sample(vel, p, vel_scale, dtype):
    """u(p): vel [B,(Z,)Y,X,D] (already of ``dtype``), p [B,N,D] -> [B,N,D]."""
    D = p.shape[-1]
    ext = vel.shape[1:-1][::-1]                                  # (X, Y[, Z])
    B = p.shape[0]
    b = np.arange(B).reshape(B, 1)
    half = dtype(0.5)
    cen = [axis_weights(p[..., a] - half, ext[a], dtype) for a in range(D)]
    face = [axis_weights(p[..., a], ext[a], dtype) for a in range(D)]
    out = np.empty(p.shape, dtype)
    for a in range(D):
        w = [face[c] if c == a else cen[c] for c in range(D)]

        def at(off):                                             # off per axis (x, y[, z]) in {0, 1}
            idx = tuple(w[c][0] + off[c] for c in reversed(range(D)))
            return vel[(b,) + idx + (a,)]

        def along_x(rest):
            return w[0][1] * at((0,) + rest) + w[0][2] * at((1,) + rest)

        if D == 2:
            r = w[1][1] * along_x((0,)) + w[1][2] * along_x((1,))
        else:
            r0 = w[1][1] * along_x((0, 0)) + w[1][2] * along_x((1, 0))
            r1 = w[1][1] * along_x((0, 1)) + w[1][2] * along_x((1, 1))
            r = w[2][1] * r0 + w[2][2] * r1
        out[..., a] = r * dtype(vel_scale)
    return out


def clamp_bounds(shape, bnd, dtype):
    """(lo, hi [D]): hi_a = (extent_a - bnd) - 2^-10"""
    ext = shape[::-1]
    return dtype(bnd), np.array([dtype(e - bnd) - dtype(2.0 ** -10) for e in ext], dtype)


def trace(pos, vel, dt, bnd=1, vel_scale=1.0, dtype=np.float64):
    """One RK4 trace and clamp; pos [B,N,D] -> [B,N,D] of ``dtype``."""
    dtype = _type(dtype)
    p = np.asarray(pos).astype(dtype)
    v = np.asarray(vel).astype(dtype)
    assert v.ndim == p.shape[-1] + 2 and v.shape[-1] == p.shape[-1] and v.shape[0] == p.shape[0]
    shape = v.shape[1:-1]
    assert bnd >= 0 and all(n >= 2 * bnd + 2 for n in shape), (shape, bnd)
    dt = dtype(dt)
    hdt = dtype(0.5) * dt
    two = dtype(2)
    with np.errstate(invalid="ignore", over="ignore"):
        k1 = mac_sample(v, p, vel_scale, dtype)
        k2 = mac_sample(v, p + hdt * k1, vel_scale, dtype)
        k3 = mac_sample(v, p + hdt * k2, vel_scale, dtype)
        k4 = mac_sample(v, p + dt * k3, vel_scale, dtype)
        s = ((k1 + two * k2) + two * k3) + k4
        moved = p + (dt * s) / dtype(6)
        lo, hi = clamp_bounds(shape, bnd, dtype)
        return np.fmin(np.fmax(moved, lo), hi).astype(dtype)             # fmax / fmin: a NaN becomes lo


def _cell_of(p, ext):
    with np.errstate(invalid="ignore"):
        low = ~(p >= 0)
        high = ~low & (p >= ext)
        i = np.where(low | high, 0, p).astype(np.int64)
    return np.where(low, 0, np.where(high, ext - 1, np.minimum(i, ext - 1)))


def cell_keys(pos, shape):
    """int32 [B*N]: key = b*ncell + ((k*Y + j)*X + i) of the fp32 positions."""
    p = np.asarray(pos, np.float32)
    B, N, D = p.shape
    ext = shape[::-1]
    ncell = int(np.prod(shape))
    cell = np.zeros((B, N), np.int64)
    for a in reversed(range(D)):
        cell = cell * ext[a] + _cell_of(p[..., a], ext[a])
    keys = np.arange(B).reshape(B, 1) * ncell + cell
    assert B * ncell < 2 ** 31
    return keys.reshape(-1).astype(np.int32)


def cell_ranges(keys, nkeys):
    """(order [B*N] -- the stable argsort --, cell_start [nkeys + 1] int32: the number of keys < c)"""
    order = np.argsort(keys, kind="stable")
    cell_start = np.searchsorted(keys[order], np.arange(nkeys + 1), side="left").astype(np.int32)
    return order, cell_start


def radius_of(D, radius_factor, dtype):
    dtype = _type(dtype)
    return (dtype(0.5) * np.sqrt(dtype(D))) * (dtype(radius_factor) + dtype(0.01))


def window_of(radius_factor):
    return int(radius_factor) + 1


def _centre(shape, a, dtype):
    """centre coordinate along axis a (0 = x), broadcastable against [(Z,)Y,X]"""
    ax = len(shape) - 1 - a
    sh = [1] * len(shape)
    sh[ax] = shape[ax]
    return (np.arange(shape[ax]).astype(dtype) + dtype(0.5)).reshape(sh)


def levelset_brute(pos, shape, radius_factor=1.0, dtype=np.float64):
    """phi [B,(Z,)Y,X] as the minimum over ALL particles of a batch entry (equal to the window form whenever 2*radius <= w + 0.5)."""
    dtype = _type(dtype)
    p = np.asarray(pos).astype(dtype)
    B, N, D = p.shape
    radius = radius_of(D, radius_factor, dtype)
    phi = np.full((B,) + tuple(shape), radius, dtype)
    for b in range(B):
        for lo in range(0, N, 256):
            q = p[b, lo:lo + 256]
            s2 = None
            for a in range(D):
                d = _centre(shape, a, dtype)[..., None] - q[:, a]
                s2 = d * d if s2 is None else s2 + d * d
            phi[b] = np.fmin(phi[b], (np.sqrt(s2) - radius).min(axis=-1))
    return phi


def clamp_ranges(cell_start, total):
    """min(max(cell_start, 0), total): the header's "out-of-range entries of order / cell_start select edge cells or edge particles, never
    memory outside the arrays" (the last sentences of the particle and of the liquid solver blocks), as the kernels apply it to every
    range end they read.  A pair with start > end is an empty range."""
    return np.minimum(np.maximum(np.asarray(cell_start, np.int64), 0), int(total))


def gather(pos, order):
    """pos_sorted[r] = pos[order[r]], an order entry outside 0..n-1 taken as the nearest edge row (the same sentence of the header)"""
    p = np.asarray(pos)
    return p[np.clip(np.asarray(order, np.int64), 0, len(p) - 1)]


def levelset_union_sorted(pos_sorted, cell_start, shape, B, radius_factor=1.0, dtype=np.float64):
    """phi as the header defines it, of SORTED particles [B*N,D] and their ranges: the particles of the cells within +-w of each cell.
    The header's level-set row writes `min` and does not say what a NaN distance does; here the minimum is C's fmin (IEEE minNum), the
    reading the same block states for the trace's clamp ("a NaN becomes bnd"): a NaN distance is skipped and never wins.  Before, a
    range that held one NaN position was dropped as a whole, finite particles included (ndarray.min() gave NaN and Python's
    min(r, NaN) kept r); on finite positions nothing changes."""
    dtype = _type(dtype)
    sp = np.asarray(pos_sorted).astype(dtype)
    D = sp.shape[-1]
    ncell = int(np.prod(shape))
    radius = radius_of(D, radius_factor, dtype)
    w = window_of(radius_factor)
    Z, Y, X = ((1,) + tuple(shape))[-3:]
    phi = np.full((B, Z, Y, X), radius, dtype)
    half = dtype(0.5)
    if len(sp):
        cell_start = clamp_ranges(cell_start, len(sp))
        for b in range(B):
            for k in range(Z):
                for j in range(Y):
                    for i in range(X):
                        c = np.array([dtype(i) + half, dtype(j) + half, dtype(k) + half][:D], dtype)
                        r = radius
                        for z in range(max(k - w, 0), min(k + w, Z - 1) + 1):
                            for y in range(max(j - w, 0), min(j + w, Y - 1) + 1):
                                key = b * ncell + (z * Y + y) * X
                                s, e = cell_start[key + max(i - w, 0)], cell_start[key + min(i + w, X - 1) + 1]
                                if e > s:
                                    with np.errstate(invalid="ignore", over="ignore"):
                                        d = c - sp[s:e]
                                        s2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
                                        if D == 3:
                                            s2 = s2 + d[:, 2] * d[:, 2]
                                        r = np.fmin(r, np.fmin.reduce(np.sqrt(s2) - radius))
                        phi[b, k, j, i] = r
    return phi.reshape((B,) + tuple(shape))


def levelset_window(pos, shape, radius_factor=1.0, dtype=np.float64):
    """phi as the header defines it: over a cell index of the fp32 positions, the particles of the cells within +-w of each cell."""
    p32 = np.asarray(pos, np.float32)
    B, N, D = p32.shape
    order, cell_start = cell_ranges(cell_keys(p32, shape), B * int(np.prod(shape)))
    return levelset_union_sorted(p32.reshape(-1, D)[order], cell_start, shape, B, radius_factor, dtype)


def sequence(pos0, vels, dt, bnd=1, vel_scale=1.0, radius_factor=1.0, dtype=np.float64):
    """The frame loop: per frame the level set of the current particles, then the trace.  Returns (final positions, list of the T phis)."""
    dtype = _type(dtype)
    p = np.asarray(pos0).astype(dtype)
    phis = []
    for v in vels:
        phis.append(levelset_brute(p, v.shape[1:-1], radius_factor, dtype))
        p = trace(p, v, dt, bnd, vel_scale, dtype)
    return p, phis


def density_image(phi):
    """The l_adv frame on the host, as the image kernel computes it: uint8(clip(255 * phi, 0, 255)), rows flipped in y; 3-D: of the z
    mean taken as a sequential ascending fp32 sum divided by Z.  [B,Y,X]."""
    d = np.asarray(phi, np.float32)
    if d.ndim == 4:
        s = d[:, 0].copy()
        for z in range(1, d.shape[1]):
            s = s + d[:, z]
        d = s / np.float32(d.shape[1]) if d.shape[1] > 1 else s
    return np.clip(d[:, ::-1] * np.float32(255), 0, 255).astype(np.uint8)


def max_err(a32, a64):
    return float(np.abs(np.asarray(a32, np.float64) - a64).max())


# ---- fixtures: seeded; velocities of several cells per step so that particles leave through every face ------------------------------
def _smooth(rng, shape, amp):
    grids = np.meshgrid(*[np.arange(n) / float(n) for n in shape], indexing="ij")
    f = np.zeros(shape)
    for _ in range(3):
        k = rng.randint(1, 3, size=len(shape))
        ph = rng.uniform(0, 2 * np.pi, size=len(shape))
        term = rng.uniform(0.4, 1.0)
        for g, kk, p in zip(grids, k, ph):
            term = term * np.sin(2 * np.pi * kk * g + p)
        f += term
    return amp * f / np.abs(f).max()


def make_velocity(shape, B, seed, T=None, vmax=6.0, vel_scale=2.5, noise=0.05):
    """[B,*shape,D] (or [T,B,*shape,D]) float32, in units of vel_scale"""
    rng = np.random.RandomState(seed)
    D = len(shape)
    v = np.zeros((T or 1, B) + tuple(shape) + (D,))
    for t in range(v.shape[0]):
        for b in range(B):
            for a in range(D):
                v[t, b, ..., a] = _smooth(rng, shape, vmax * rng.uniform(0.6, 1.0)) + noise * rng.standard_normal(shape)
    v = (v / vel_scale).astype(np.float32)
    return v if T else v[0]


def special_positions(shape, bnd):
    """The positions the clamp and the edge weights exist for: exact bnd and exact upper-clamp values, the first and last cell on every
    axis (inside the band too).  [M,D] float32."""
    D = len(shape)
    ext = shape[::-1]
    lo, hi = clamp_bounds(shape, bnd, np.float32)
    mid = np.array([0.5 * e + 0.125 for e in ext], np.float32)
    out = [np.full(D, lo, np.float32), hi.copy()]
    for a in range(D):
        for val in (lo, hi[a], np.float32(0.25), np.float32(ext[a] - 0.25), np.float32(0.0), np.float32(bnd + 0.5), np.float32(ext[a] - bnd - 0.5)):
            p = mid.copy()
            p[a] = val
            out.append(p)
    return np.stack(out)


def make_positions(shape, B, N, bnd, seed):
    """[B,N,D] float32: uniform inside the clamp, the first rows of every batch entry replaced by ``special_positions`` (N = 1: by the
    exact-bnd corner in entry 0, by the exact upper corner in the others)."""
    rng = np.random.RandomState(seed)
    D = len(shape)
    lo, hi = clamp_bounds(shape, bnd, np.float32)
    p = (lo + rng.uniform(0, 1, size=(B, N, D)) * (hi - lo)).astype(np.float32)
    sp = special_positions(shape, bnd)
    for b in range(B):
        if N == 1:
            p[b, 0] = sp[min(b, 1)]
        else:
            m = min(N, len(sp))
            p[b, :m] = sp[:m]
    return p


#            name            shape         B  N     bnd
TRACE_CASES = [("2d-b1-n1", (12, 9), 1, 1, 1),
               ("2d-b1-n255", (12, 9), 3, 255, 1),
               ("2d-b2-n257", (12, 9), 3, 257, 2),
               ("2d-b2-n1000", (12, 9), 1, 1000, 2),
               ("3d-b1-n257", (7, 8, 6), 3, 257, 1),
               ("3d-b1-n1000", (7, 8, 6), 1, 1000, 1),
               ("3d-b2-n1", (7, 8, 6), 1, 1, 2),
               ("3d-b2-n255", (7, 8, 6), 3, 255, 2),
               ("3d-16x24x16", (16, 24, 16), 3, 1000, 1)]
VEL_SCALE = 2.5


def trace_cases():
    """(name, positions, velocity, kwargs) of every single-step case"""
    for n, (name, shape, B, N, bnd) in enumerate(TRACE_CASES):
        yield name, make_positions(shape, B, N, bnd, 100 + n), make_velocity(shape, B, 200 + n), dict(dt=1.0, bnd=bnd, vel_scale=VEL_SCALE)


SEQ_CASES = [("2d-T8", (12, 9), 3, 257, 1), ("3d-T8", (7, 8, 6), 3, 257, 1)]


def sequence_cases():
    """(name, positions, velocities [8,...], kwargs) of the 8-frame cases"""
    for n, (name, shape, B, N, bnd) in enumerate(SEQ_CASES):
        yield (name, make_positions(shape, B, N, bnd, 300 + n), make_velocity(shape, B, 400 + n, T=8, vmax=3.0),
               dict(dt=0.5, bnd=bnd, vel_scale=VEL_SCALE, radius_factor=1.0))


def levelset_positions(shape, B, N, seed, crowd=0):
    """[B,N,D] float32 with empty cells: the particles fill the lower-index half of the grid, and ``crowd`` of them share one cell."""
    rng = np.random.RandomState(seed)
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    p = rng.uniform(0, 1, size=(B, N, D)) * (0.55 * ext)
    if crowd:
        cell = np.floor(0.7 * ext)
        p[-1, :crowd] = cell + rng.uniform(0.01, 0.99, size=(min(crowd, N), D))
    return p.astype(np.float32)


#              name         shape      B  N     crowd
LEVELSET_CASES = [("2d-n1", (12, 9), 1, 1, 0),
                  ("2d-n1000", (12, 9), 3, 1000, 300),
                  ("3d-n255", (7, 8, 6), 3, 255, 0),
                  ("3d-n1000", (7, 8, 6), 1, 1000, 300),
                  ("3d-16x24x16", (16, 24, 16), 3, 257, 0)]
RADIUS_FACTORS = (0.5, 1.0, 2.0)


def levelset_cases():
    for n, (name, shape, B, N, crowd) in enumerate(LEVELSET_CASES):
        yield name, shape, levelset_positions(shape, B, N, 500 + n, crowd)
