"""NumPy restatement of the density-advection step declared in include/deepfluids_hip.h (semi-Lagrangian / MacCormack with clamp,
source stamp, d_adv image), written from that definition and parametrised by dtype: float64 is the reference of the GPU tests, float32
-- the same operations in the same order -- is the twin whose distance from float64 sets their tolerance.  Plain helper, no fixtures.

Layout: density [B,(Z,)Y,X], velocity [B,(Z,)Y,X,C], C = 2 | 3, cell (i,j,k) = [..,k,j,i].  Axis a = 0, 1, 2 below means x, y, z."""
import itertools

import numpy as np

BAND, FWD, COR, NOCORNER = 0, 1, 2, 3      # which branch a cell took: band / fwd (order 1, or the MacCormack revert) / corrected / no interior corner


def _ext(density):
    return density.shape[1:][::-1]             # (X, Y[, Z])


def interior_mask(shape, bnd):
    """[(Z,)Y,X] bool: bnd <= index < extent - bnd on every axis."""
    m = np.ones(shape, bool)
    for ax, n in enumerate(shape):
        idx = np.arange(n)
        sh = [1] * len(shape)
        sh[ax] = n
        m &= ((idx >= bnd) & (idx < n - bnd)).reshape(sh)
    return m


def _cell_index(shape, a, dtype):
    """index along axis a (0 = x) of every cell, broadcastable against [B,(Z,)Y,X]"""
    nd = len(shape)
    sh = [1] * (nd + 1)
    sh[nd - a] = shape[nd - 1 - a]
    return np.arange(shape[nd - 1 - a]).astype(dtype).reshape(sh)


def displacement(vel, dt, bnd, vel_scale, dtype):
    """dt * uc per axis (list over x, y[, z]) on every cell; only interior cells are meaningful (the +1 neighbour is rolled)."""
    vel = vel.astype(dtype)
    d = vel.shape[-1]
    nd = vel.ndim - 2
    out = []
    half, vs, dt = dtype(0.5), dtype(vel_scale), dtype(dt)
    for a in range(d):
        own = vel[..., a]
        nb = np.roll(own, -1, axis=nd - a)      # axis of x is the last spatial one
        out.append(dt * ((half * (own + nb)) * vs))
    return out


def _axis_weights(p, ext, dtype):
    q = p - dtype(0.5)
    with np.errstate(invalid="ignore"):
        n = q.astype(np.int64)                  # truncation
    s1 = q - n.astype(dtype)
    s0 = dtype(1) - s1
    neg = q < 0
    n = np.where(neg, 0, n); s0 = np.where(neg, dtype(1), s0); s1 = np.where(neg, dtype(0), s1)
    hi = n >= ext - 1
    n = np.where(hi, ext - 2, n); s0 = np.where(hi, dtype(0), s0); s1 = np.where(hi, dtype(1), s1)
    return n, s0.astype(dtype), s1.astype(dtype)


def interp(g, pos, dtype):
    """g [B,(Z,)Y,X]; pos list over axes (x, y[, z]) of arrays broadcastable to g.shape -> interpolated values, g.shape."""
    g = g.astype(dtype)
    d = len(pos)
    ext = _ext(g)
    B = g.shape[0]
    w = [_axis_weights(np.broadcast_to(pos[a], g.shape).astype(dtype), ext[a], dtype) for a in range(d)]
    b = np.arange(B).reshape([B] + [1] * d)

    def at(off):                                 # off per axis (x, y[, z]) in {0, 1}
        idx = tuple(w[a][0] + off[a] for a in reversed(range(d)))
        return g[(b,) + idx]

    def along_x(rest):
        return w[0][1] * at((0,) + rest) + w[0][2] * at((1,) + rest)

    if d == 2:
        return w[1][1] * along_x((0,)) + w[1][2] * along_x((1,))
    r0 = w[1][1] * along_x((0, 0)) + w[1][2] * along_x((1, 0))
    r1 = w[1][1] * along_x((0, 1)) + w[1][2] * along_x((1, 1))
    return w[2][1] * r0 + w[2][2] * r1


def semi_lagrange(g, du, sign, bnd, dtype):
    """SL(g, sign*dt): interp(g, centre - sign*dt*uc) on interior cells, 0 on the band."""
    shape = g.shape[1:]
    pos = []
    for a in range(len(du)):
        c = _cell_index(shape, a, dtype) + dtype(0.5)
        pos.append(c - du[a] if sign > 0 else c + du[a])
    r = interp(g, pos, dtype)
    return np.where(interior_mask(shape, bnd)[None], r, dtype(0)).astype(dtype)


def _clamp_cells(shape, du, sign, dtype):
    """c = clamp(trunc((i,j,k) - sign*dt*uc), 0, extent - 2) per axis; list over (x, y[, z])."""
    ext = shape[::-1]
    out = []
    for a in range(len(du)):
        i = _cell_index(shape, a, dtype)
        t = i - du[a] if sign > 0 else i + du[a]
        with np.errstate(invalid="ignore"):
            c = t.astype(np.int64)
        out.append(np.clip(c, 0, ext[a] - 2))
    return out


def _corner_range(orig, cells, bnd, mn, mx, found):
    d = len(cells)
    B = orig.shape[0]
    shape = orig.shape[1:]
    inter = interior_mask(shape, bnd)
    b = np.arange(B).reshape([B] + [1] * d)
    for off in itertools.product((0, 1), repeat=d):            # off over (x, y[, z])
        idx = tuple(cells[a] + off[a] for a in reversed(range(d)))
        ok = inter[idx]
        v = orig[(b,) + idx]
        mn = np.where(ok, np.where(found, np.minimum(mn, v), v), mn)
        mx = np.where(ok, np.where(found, np.maximum(mx, v), v), mx)
        found = found | ok
    return mn, mx, found


def stamp(density, source, value, dtype):
    d = density.astype(dtype)
    if source is None:
        return d
    return np.where(np.broadcast_to(np.asarray(source).astype(bool), d.shape), dtype(value), d).astype(dtype)


def step(density, vel, dt, order=2, clamp_mode=2, bnd=1, vel_scale=1.0, source=None, source_value=1.0, dtype=np.float64):
    """One step.  Returns a dict: ``out``; ``branch`` (BAND / FWD / COR / NOCORNER per cell); ``cell`` (the flattened clamp cells the
    min / max were taken around -- a trunc() flipped by rounding shows here); ``fwd``, ``cor`` (the two values a MacCormack cell
    chooses between), ``orig`` (after the source stamp)."""
    dtype = np.dtype(dtype).type
    assert order in (1, 2) and clamp_mode in (1, 2) and bnd >= 1
    shape = density.shape[1:]
    assert all(2 * bnd + 2 <= n for n in shape), (shape, bnd)
    assert vel.shape[:-1] == density.shape and vel.shape[-1] == len(shape)
    orig = stamp(density, source, source_value, dtype)
    du = displacement(vel, dt, bnd, vel_scale, dtype)
    inter = np.broadcast_to(interior_mask(shape, bnd)[None], orig.shape)
    fwd = semi_lagrange(orig, du, +1, bnd, dtype)
    if order == 1:
        return {"out": fwd, "branch": np.where(inter, FWD, BAND), "cell": np.zeros(orig.shape, np.int64), "fwd": fwd, "cor": fwd, "orig": orig}
    bwd = semi_lagrange(fwd, du, -1, bnd, dtype)
    cor = (fwd + dtype(0.5) * (orig - bwd)).astype(dtype)
    cells = _clamp_cells(shape, du, +1, dtype)
    mn = np.zeros(orig.shape, dtype); mx = np.zeros(orig.shape, dtype); found = np.zeros(orig.shape, bool)
    mn, mx, found = _corner_range(orig, cells, bnd, mn, mx, found)
    flat = np.ravel_multi_index(tuple(np.broadcast_to(c, orig.shape) for c in reversed(cells)), shape)
    if clamp_mode == 1:
        cells2 = _clamp_cells(shape, du, -1, dtype)
        mn, mx, found = _corner_range(orig, cells2, bnd, mn, mx, found)
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
    out = np.where(inter, val, dtype(0)).astype(dtype)
    return {"out": out, "branch": np.where(inter, br, BAND), "cell": np.where(inter, flat, 0), "fwd": fwd, "cor": cor, "orig": orig}


def sequence(density0, vels, dt, dtype=np.float64, **kw):
    """T chained steps over vels[T]; returns the list of step records (the last one's ``out`` is the final density)."""
    d = density0
    recs = []
    for v in vels:
        r = step(d, v, dt, dtype=dtype, **kw)
        recs.append(r)
        d = r["out"]
    return recs


def same_branch(a, b):
    return (a["branch"] == b["branch"]) & (a["cell"] == b["cell"])


def twin_error(r64, r32, bnd):
    """(e32, share): the largest |fp32 twin - fp64| over cells where both took the same branch, and the share of interior cells where
    they did not."""
    same = same_branch(r64, r32)
    diff = np.abs(r32["out"].astype(np.float64) - r64["out"])
    e32 = float(diff[same].max())
    n_int = int(interior_mask(r64["out"].shape[1:], bnd).sum()) * r64["out"].shape[0]
    return e32, float((~same).sum()) / n_int


def alternatives_of(r64, vel, dt, clamp_mode, bnd, vel_scale):
    """``alt`` argument of ``compare`` for one step record"""
    return lambda index: alternatives(r64, r64["out"].shape, index, vel, dt, clamp_mode, bnd, vel_scale)


def alternatives(r64, density_shape, index, vel, dt, clamp_mode, bnd, vel_scale, near=1e-3):
    """The fp64 values a cell may take when a decision flips by rounding: the other side of the revert (fwd | cor) and, in clamp mode 1
    (and for the no-corner test), orig at the interior corners of every clamp cell reachable by moving a trunc() whose argument lies
    within ``near`` of an integer."""
    b = index[0]
    cand = [float(r64["fwd"][index]), float(r64["cor"][index])]
    shape = density_shape[1:]
    d = len(shape)
    ext = shape[::-1]
    du = [float(x[index]) for x in displacement(vel, dt, bnd, vel_scale, np.float64)]
    ijk = index[1:][::-1]
    inter = interior_mask(shape, bnd)
    for sign in ((+1, -1) if clamp_mode == 1 else (+1,)):
        opts = []
        for a in range(d):
            t = ijk[a] - sign * du[a]
            c = {int(t)}
            if abs(t - round(t)) < near:
                c |= {int(round(t)) - 1, int(round(t))}
            opts.append(sorted({min(max(v, 0), ext[a] - 2) for v in c}))
        for cell in itertools.product(*opts):
            for off in itertools.product((0, 1), repeat=d):
                idx = tuple(cell[a] + off[a] for a in reversed(range(d)))
                if inter[idx]:
                    cand.append(float(r64["orig"][(b,) + idx]))
    return cand


def compare(got, r64, e32, bnd, alt=None):
    """The GPU-vs-fp64 rule: |got - fp64| <= 3*e32 + 1e-7 on every cell, except cells that took another branch than fp64 -- at most
    0.1 % of the interior cells, each equal within the same bound to an fp64 value of the other branch (``alt(index) -> candidates``).
    Returns (largest error over the agreeing cells, share left out); raises AssertionError otherwise."""
    tol = 3.0 * e32 + 1e-7
    diff = np.abs(np.asarray(got, np.float64) - r64["out"])
    bad = diff > tol
    n_int = int(interior_mask(r64["out"].shape[1:], bnd).sum()) * r64["out"].shape[0]
    share = float(bad.sum()) / n_int
    err = float(diff[~bad].max())
    assert share <= 1e-3, "%d of %d interior cells differ from fp64 by more than %.3e" % (int(bad.sum()), n_int, tol)
    for index in zip(*np.nonzero(bad)):
        assert alt is not None, (index, float(diff[index]))
        cand = alt(index)
        gap = min(abs(float(got[index]) - c) for c in cand)
        assert gap <= tol, "cell %s: %.9g is neither fp64's %.9g nor another branch's %s" % (index, float(got[index]), float(r64["out"][index]), cand)
    return err, share


def density_image(d):
    """The d_adv frame on the host: uint8(clip(255 * d[::-1], 0, 255)), 3-D of the fp32 z mean; [B,Y,X]."""
    d = np.asarray(d, np.float32)
    if d.ndim == 4:
        d = d.mean(axis=1, dtype=np.float32)
    return np.clip(d[:, ::-1] * np.float32(255), 0, 255).astype(np.uint8)


def sphere_mask_loop(shape, center, radius):
    """Brute force: cell (i,j,k) is marked when its centre (i+.5, j+.5, k+.5) lies within ``radius`` of ``center`` (xyz order)."""
    m = np.zeros(shape, np.uint8)
    d = len(shape)
    for idx in itertools.product(*[range(n) for n in shape]):
        p = idx[::-1]
        r2 = sum((p[a] + 0.5 - center[a]) ** 2 for a in range(d))
        m[idx] = r2 <= radius * radius
    return m


def exact_shift_inputs(shape, B=2, seed=3):
    """dt = 0.5, velocities even integers, density on a dyadic grid: every intermediate is exact in fp32."""
    rng = np.random.RandomState(seed)
    d = (rng.randint(0, 257, (B,) + shape) / 256.0).astype(np.float32)
    shift = [2, -1, 1][:len(shape)]                       # cells per step along x, y[, z]
    v = np.zeros((B,) + shape + (len(shape),), np.float32)
    for a, s in enumerate(shift):
        v[..., a] = 2.0 * s                               # dt * u = s
    return d, v, shift


def shifted(d, shift, bnd):
    """out(i,j,k) = d(i - sx, j - sy, k - sz) with the source index clamped to the grid, on interior cells; 0 on the band."""
    shape = d.shape[1:]
    idx = []
    for ax, n in enumerate(shape):
        a = len(shape) - 1 - ax
        src = np.clip(np.arange(n) - shift[a], 0, n - 1)
        sh = [1] * len(shape)
        sh[ax] = n
        idx.append(src.reshape(sh))
    out = d[(slice(None),) + tuple(np.broadcast_arrays(*idx))]
    return np.where(interior_mask(shape, bnd)[None], out, 0).astype(d.dtype)


# ---- fixtures: seeded, smooth, velocities of 0-6 cells per step so that traces reach the band -----------------------------------------
def _sines(rng, shape, n_modes, amp):
    grids = np.meshgrid(*[np.arange(n) / float(n) for n in shape], indexing="ij")
    f = np.zeros(shape)
    for _ in range(n_modes):
        k = rng.randint(1, 3, size=len(shape))
        ph = rng.uniform(0, 2 * np.pi, size=len(shape))
        term = rng.uniform(0.4, 1.0)
        for g, kk, p in zip(grids, k, ph):
            term = term * np.sin(2 * np.pi * kk * g + p)
        f += term
    return amp * f / n_modes


def make_fixture(shape, B=3, seed=0, vmax=6.0, noise=0.02, vel_scale=2.5, with_source=False, T=1):
    """density [B,*shape] (blurred blobs in [0,1]), vels [T,B,*shape,C] (in units of vel_scale), optional source mask; all float32."""
    rng = np.random.RandomState(seed)
    d = len(shape)
    grids = np.meshgrid(*[np.arange(n) + 0.5 for n in shape], indexing="ij")
    dens = np.zeros((B,) + tuple(shape))
    for b in range(B):
        for _ in range(2):
            c = [rng.uniform(0.3, 0.7) * n for n in shape]
            s = [rng.uniform(0.12, 0.22) * n for n in shape]
            dens[b] += 0.5 * np.exp(-sum(((g - cc) / ss) ** 2 for g, cc, ss in zip(grids, c, s)))
    dens = np.clip(dens, 0, 1)
    vels = np.zeros((T, B) + tuple(shape) + (d,))
    for t in range(T):
        for b in range(B):
            for a in range(d):
                f = _sines(rng, shape, 3, 1.0)
                f = f / np.abs(f).max() * vmax * (1.0 if a == 0 and b == 0 else rng.uniform(0.5, 1.0))
                vels[t, b, ..., a] = f + noise * rng.standard_normal(shape)
    vels = vels / vel_scale
    src = None
    if with_source:
        c = [0.5 * n for n in shape[::-1]]
        c[1] = 0.2 * shape[-2]
        src = sphere_mask_loop(tuple(shape), c, 0.15 * shape[-1])[None].repeat(B, axis=0)
    return {"density": dens.astype(np.float32), "vels": vels.astype(np.float32), "source": src, "vel_scale": vel_scale, "dt": 0.5 if T > 1 else 1.0}


SHAPES = {"2d_128x96": (128, 96), "3d_16x24x16": (16, 24, 16), "3d_19x10x7": (19, 10, 7)}
# seeds tuned on the CPU (tests/test_advect_host.py, the fixture gate) so that the fp32 twin takes fp64's branch in all but a few cells
SEEDS = {("2d_128x96", False): 2, ("2d_128x96", True): 100, ("3d_16x24x16", False): 0, ("3d_16x24x16", True): 100,
         ("3d_19x10x7", False): 0, ("3d_19x10x7", True): 100}
SEQ_SEEDS = {"2d_128x96": 11, "3d_16x24x16": 10}


def single_step_cases():
    """(name, fixture, kwargs) of every single-step parity case: orders 1 | 2, clamp modes 1 | 2, bnd 1 | 2, with and without a source."""
    for tag, shape in SHAPES.items():
        for src in (False, True):
            fx = make_fixture(shape, seed=SEEDS[(tag, src)], with_source=src)
            for order, mode in ((1, 2), (2, 1), (2, 2)):
                for bnd in (1, 2):
                    if 2 * bnd + 2 > min(shape):
                        continue
                    yield "%s-o%d-m%d-b%d-%s" % (tag, order, mode, bnd, "src" if src else "nosrc"), fx, dict(order=order, clamp_mode=mode, bnd=bnd)


def sequence_cases():
    for tag, seed in SEQ_SEEDS.items():
        yield "%s-T8" % tag, make_fixture(SHAPES[tag], seed=seed, with_source=True, T=8, vmax=4.0), dict(order=2, clamp_mode=2, bnd=1)
