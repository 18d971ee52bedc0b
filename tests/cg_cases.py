"""The table of tests/test_gpu_cg_edges.py: one row per (variant of the conjugate-gradient solve, grid) with the inputs, the fp32 twin
(the variant's cg() / pcg() restatement run with the reductions of tests/cg_ref.py) and the entry points of the raw C ABI with their
argument lists.  tests/test_cg_cases_host.py keeps the conditions on the rows without a GPU.  NumPy only.

A row: ``variant`` (VARIANTS), ``shape`` [(Z,)Y,X], ``bnd``, ``B`` = 3, ``ks`` (the iteration counts K at which the device state is
compared; direction(k) / update(k) run for k < max(ks) with accuracy 0 and max_iter = max(ks)), ``s2`` (entry 2 is scaled by 2**-s2),
``seed`` (of the inputs: a row that could not tell a wrong summation order apart got another one) and ``reaches`` (why the row is there).

Entries: 0 iterates until max_iter; 1 is at rest (r = 0: frozen by direction(0), 0 iterations); 2 holds the faces of a dozen cells
only, scaled by 2**-s2: its residual spreads and shrinks with every iteration, and once every |r| is below 2**-75 every product r*r
rounds to 0, r.r is 0 and direction freezes the entry on ``rr > 0`` although accuracy is 0.  s2 was chosen per row from the twin so that
this happens after ``it2`` iterations, 0 < it2 < max(ks) (a diffusion states one count per component); tests/test_cg_cases_host.py
asserts the counts the row states.  The products and sums near the end of that run are subnormal: float32 arithmetic is IEEE on
both sides (no flush to zero, correctly rounded quotients).  For the solve to the default accuracy (``solve`` rows) entry 2 is the
full field scaled by 2**-10 instead and stops early on max|r|."""
import functools

import numpy as np

import cg_ref
import diffuse_ref as dref
import liquid_gf_ref as gref
import liquid_ref as lref
import smoke_mg_ref as mg
import smoke_obs_ref as oref
import smoke_open_ref as pref
import smoke_ref as sref

F32 = np.float32
K_THREADS = cg_ref.K_THREADS
VARIANTS = ("closed", "obstacle", "open", "obsopen", "liquid", "gf", "diffuse", "mg", "mg-obs", "mg-open")
GF_CLAMP = 1e-4
ACCURACY = 1e-4
SOLVE_S2 = 10


def _row(variant, shape, bnd, ks, s2, it2, reaches, solve=False, seed=0):
    name = "%s-%s-b%d" % (variant, "x".join(map(str, shape)), bnd)
    return dict(name=name, variant=variant, shape=tuple(shape), bnd=bnd, B=3, ks=tuple(ks), s2=s2, it2=it2, reaches=reaches, solve=solve, seed=seed)


# workgroups per entry: 7x9 1, 17x19 2 (the second holds 67 cells), 255x257 256, 259x259 263, 363x365 518; 6x6x7 1, 7x7x9 2 (185),
# 39x40x42 256, 41x41x41 270, 41x41x43 283 (bnd 2: plane z = 38 is interior and lies past cell 65536), 51x51x51 519.  X is odd or X % 4 == 2 throughout.
ROWS = [
    _row("closed", (7, 9), 2, (1, 3), 75, 1, "one workgroup, bnd 2", solve=False),
    _row("closed", (17, 19), 1, (2, 4), 74, 3, "two workgroups, the second ragged", solve=True),
    _row("closed", (255, 257), 1, (2,), 75, 1, "exactly 256 workgroups: one full trip of entry_reduce, none beyond"),
    _row("closed", (259, 259), 2, (2, 4), 74, 1, "263 workgroups: a second trip for threads 0..6; bnd 2", seed=5),
    _row("closed", (363, 365), 1, (2, 4), 74, 2, "518 workgroups: three trips"),
    _row("closed", (6, 6, 7), 2, (1, 3), 74, 2, "3-D, one workgroup, bnd 2"),
    _row("closed", (7, 7, 9), 1, (2, 4), 72, 2, "3-D, two workgroups, the second ragged", solve=True),
    _row("closed", (39, 40, 42), 1, (2,), 74, 1, "3-D, exactly 256 workgroups"),
    _row("closed", (41, 41, 43), 2, (3, 4), 74, 1, "3-D, 283 workgroups; bnd 2", seed=1),
    _row("closed", (51, 51, 51), 1, (2, 4), 74, 1, "3-D, 519 workgroups: three trips", seed=1),
    _row("obstacle", (17, 19), 1, (2, 4), 74, 3, "flags byte, popcount n_c", solve=True),
    _row("obstacle", (259, 259), 1, (3, 4), 74, 1, "flags, 263 workgroups", seed=4),
    _row("obstacle", (7, 7, 9), 2, (2, 3), 72, 2, "3-D flags, bnd 2"),
    _row("obstacle", (41, 41, 41), 1, (2, 4), 74, 2, "3-D flags, 270 workgroups", seed=2),
    _row("open", (17, 19), 2, (2, 4), 74, 2, "open sides XyY by the index, bnd 2", solve=True),
    _row("open", (363, 365), 2, (2, 4), 75, 1, "open sides, 518 workgroups, bnd 2"),
    _row("open", (7, 7, 9), 1, (2, 3), 74, 2, "3-D open sides xYZ"),
    _row("open", (41, 41, 41), 1, (3, 4), 75, 1, "3-D open sides, 270 workgroups"),
    _row("obsopen", (7, 9), 1, (1, 3), 74, 2, "flags and open sides, one workgroup"),
    _row("obsopen", (17, 19), 1, (2, 4), 74, 2, "flags and open sides", solve=True),
    _row("obsopen", (259, 259), 1, (2, 4), 74, 1, "flags and open sides, 263 workgroups", seed=3),
    _row("obsopen", (51, 51, 51), 2, (2,), 76, 1, "3-D flags and open sides, 519 workgroups, bnd 2"),
    _row("liquid", (17, 19), 1, (2, 4), 74, 2, "liquid rows: n_c by the index, sums by the flags", solve=True),
    _row("liquid", (259, 259), 2, (3,), 73, 2, "liquid, 263 workgroups, bnd 2"),
    _row("liquid", (7, 7, 9), 1, (2, 4), 72, 2, "3-D liquid"),
    _row("liquid", (41, 41, 41), 1, (2,), 74, 1, "3-D liquid, 270 workgroups"),
    _row("gf", (17, 19), 1, (2, 4), 73, 2, "ghost fluid: kRowDiag, kLeaveJacobi", solve=True),
    _row("gf", (363, 365), 1, (2,), 74, 1, "ghost fluid, 518 workgroups"),
    _row("gf", (7, 7, 9), 1, (2, 4), 73, 1, "3-D ghost fluid", seed=1),
    _row("gf", (41, 41, 43), 2, (2, 4), 74, 1, "3-D ghost fluid, 283 workgroups, bnd 2", seed=3),
    _row("diffuse", (17, 19), 1, (2, 4), 75, (2, 2), "diffusion: B*D pairs, kRowDiffuse", solve=True),
    _row("diffuse", (259, 259), 1, (2,), 76, (1, 1), "diffusion, 6 pairs of 263 workgroups"),
    _row("diffuse", (7, 7, 9), 2, (2, 3), 76, (1, 1, 2), "3-D diffusion, bnd 2"),
    _row("diffuse", (41, 41, 41), 1, (2,), 78, (1, 1, 1), "3-D diffusion, 9 pairs of 270 workgroups"),
    _row("mg", (17, 19), 1, (2, 4), 71, 2, "multigrid: kLeaveMg, r.z from the V-cycle's last sweep", solve=True),
    _row("mg", (41, 41, 41), 1, (2, 4), 74, 1, "3-D multigrid, 270 workgroups", seed=4),
    _row("mg-obs", (7, 7, 9), 1, (2, 3), 73, 1, "3-D multigrid with flags"),
    _row("mg-obs", (259, 259), 2, (2,), 73, 1, "multigrid with flags, 263 workgroups, bnd 2"),
    _row("mg-open", (17, 19), 2, (2, 4), 73, 1, "multigrid with open sides, bnd 2"),
    _row("mg-open", (7, 7, 9), 1, (2, 3), 73, 1, "3-D multigrid with open sides xYZ"),
    _row("mg-open", (259, 259), 1, (2,), 73, 1, "multigrid with open sides, 263 workgroups"),
]
BY_NAME = dict((r["name"], r) for r in ROWS)
assert len(BY_NAME) == len(ROWS)


def names(large=None, solve=None):
    return [r["name"] for r in ROWS if (large is None or (nblk(r) > K_THREADS) == large) and (solve is None or r["solve"] == solve)]


def nblk(r):
    return -(-int(np.prod(r["shape"])) // K_THREADS)


def systems(r):
    """the entries of the solve's grid: batch entries, or the (entry, component) pairs of a diffusion"""
    return r["B"] * (len(r["shape"]) if r["variant"] == "diffuse" else 1)


def open_bits(r):
    if r["variant"] not in ("open", "obsopen", "mg-open"):
        return 0
    return pref.sides("XyY" if len(r["shape"]) == 2 else "xYZ", len(r["shape"]))


def has_flags(r):
    return r["variant"] in ("obstacle", "obsopen", "liquid", "gf", "mg-obs")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _field(rng, shape, B, D):
    """white noise in [-1, 1) on a slow wave: divergence at every scale, cheap at 135 000 cells"""
    grids = np.meshgrid(*[np.arange(n) / float(n) for n in shape], indexing="ij")
    v = rng.uniform(-1.0, 1.0, (B,) + tuple(shape) + (D,))
    for a in range(D):
        v[..., a] += np.sin(2 * np.pi * (grids[a % len(shape)] + 0.1 * a))[None]
    return v.astype(F32)


def _obstacle(shape):
    """a block in the middle and a plate near the far end of the slowest axis, so that the last workgroups hold solid and fluid cells"""
    o = np.zeros(shape, np.uint8)
    o[tuple(slice(n // 2 - max(1, n // 8), n // 2 + max(1, n // 8)) for n in shape)] = 1
    plate = [slice(n // 4, n // 2) for n in shape]
    plate[0] = slice(shape[0] - 4, shape[0] - 3)
    if shape[0] >= 12:
        o[tuple(plate)] = 1
    return o


def _phi(shape):
    """a tilted plane with a ripple: negative (liquid) on the low-x side of every row and plane, the last ones included"""
    idx = np.meshgrid(*[np.arange(n) + 0.5 for n in shape], indexing="ij")
    x = idx[-1]
    phi = (x - 0.55 * shape[-1]) + 0.2 * (idx[-2] - 0.5 * shape[-2]) + 1.5 * np.sin(idx[0] * 0.7)
    return phi.astype(F32)


@functools.lru_cache(maxsize=4)
def inputs(name, solve=False):
    """the operands of a row as NumPy arrays: vel [B,..,D] float32 and, by variant, obstacle / liquid / flags / phi / alpha / bits"""
    r = BY_NAME[name]
    shape, bnd, B, var = r["shape"], r["bnd"], r["B"], r["variant"]
    D = len(shape)
    rng = np.random.RandomState(sum(map(ord, name)) + 1000 * r["seed"])
    vel = _field(rng, shape, B, D)
    vel[1] = 0
    i = dict(bits=open_bits(r))
    full = (B,) + shape
    if var in ("obstacle", "obsopen", "mg-obs"):
        i["obstacle"] = np.broadcast_to(_obstacle(shape)[None], full).copy()
    elif var in ("open", "mg", "mg-open", "closed"):
        i["obstacle"] = np.zeros(full, np.uint8)
    if var == "closed":
        vel = sref.walled(vel, bnd)
    elif var in ("obstacle", "obsopen", "open", "mg", "mg-obs", "mg-open"):
        zero = (0.0,) * D
        vel = pref.wall_buoyancy(vel, np.zeros(full, F32), zero, i["obstacle"], i["bits"], bnd, F32)
        if has_flags(r):
            i["flags"] = oref.flags(i["obstacle"], bnd)
    elif var in ("liquid", "gf"):
        i["phi"] = np.broadcast_to(_phi(shape)[None], full).copy()
        i["liquid"] = (i["phi"] < 0) & sref.interior_mask(shape, bnd)[None]
        i["flags"] = lref.flags_of(i["liquid"])[0]
        vel = lref.forces(vel, i["liquid"], (0.0,) * D, bnd, F32)
    elif var == "diffuse":
        i["alpha"] = np.array([0.75, 1.5, 2.25], F32)
    vel = np.ascontiguousarray(vel, F32)
    if not solve:                                                    # entry 2 for the accuracy-0 run: a dozen cells' faces, see above
        keep = np.zeros(int(np.prod(shape)), bool)
        keep[rng.permutation(keep.size)[:12]] = True
        vel[2] = np.where(keep.reshape(shape + (1,)), vel[2], F32(0))
    vel[2] = vel[2] * F32(2.0) ** F32(-(SOLVE_S2 if solve else r["s2"]))
    i["vel"] = vel
    return i


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------
def run(name, max_iter, accuracy=0.0, dtype=F32, dot=None, amax=None, entries=None, solve=False):
    """the row's restatement for at most ``max_iter`` iterations -> dict(x, iters, out): the pressure (diffusion: the planar x), the
    iteration counts (diffusion: [B, D]) and the corrected (diffusion: finished) velocity.  ``dot`` / ``amax`` default to the header's
    order; ``entries`` (a slice) runs a part of the batch."""
    r = BY_NAME[name]
    i = inputs(name, solve)
    bnd, var = r["bnd"], r["variant"]
    sl = slice(None) if entries is None else entries
    dot = cg_ref.ordered_dot if dot is None else dot
    amax = cg_ref.ordered_amax if amax is None else amax
    kw = dict(dtype=dtype, dot=dot, amax=amax)
    vel = i["vel"][sl]
    if var == "closed":
        x, it, _ = sref.cg(vel, bnd, accuracy, max_iter, **kw)
        out = sref.correct(vel, x, bnd, dtype)
    elif var == "obstacle":
        x, it, _ = oref.cg(vel, i["obstacle"][sl], bnd, accuracy, max_iter, **kw)
        out = oref.correct(vel, x, i["obstacle"][sl], bnd, dtype)
    elif var in ("open", "obsopen"):
        x, it, _ = pref.cg(vel, i["obstacle"][sl], i["bits"], bnd, accuracy, max_iter, **kw)
        out = pref.correct(vel, x, i["obstacle"][sl], i["bits"], bnd, dtype)
    elif var == "liquid":
        x, it, _ = lref.cg(vel, i["liquid"][sl], bnd, accuracy, max_iter, **kw)
        out = lref.correct(vel, x, i["liquid"][sl], bnd, dtype)
    elif var == "gf":
        x, it, _ = gref.pcg(vel, i["liquid"][sl], i["phi"][sl], bnd, accuracy, max_iter, GF_CLAMP, **kw)
        out = gref.correct(vel, x, i["liquid"][sl], i["phi"][sl], bnd, GF_CLAMP, dtype)
    elif var == "diffuse":
        out, it, _, x = dref.cg(vel, i["alpha"][sl], bnd, accuracy, max_iter, **kw)
    else:
        x, it, _, _ = mg.pcg(vel, i["obstacle"][sl], i["bits"], bnd, accuracy, max_iter, dtype, mg.ALPHA, True, dot, amax)
        out = pref.correct(vel, x, i["obstacle"][sl], i["bits"], bnd, dtype)
    return dict(x=x, iters=np.asarray(it), out=out)


_TWIN = {}


def twin(name, K, solve=False):
    """the fp32 twin, computed once and shared (read only)"""
    key = (name, K, solve)
    if key not in _TWIN:
        if solve:
            t = run(name, 100000 if K is None else K, ACCURACY, solve=True)
        else:
            t = run(name, K)
        for v in t.values():
            v.setflags(write=False)
        _TWIN[key] = t
    return _TWIN[key]


def expected_iters(r, K):
    """what the row states for accuracy 0 and max_iter K: entry 0 runs K, entry 1 none, entry 2 min(it2, K)"""
    if r["variant"] != "diffuse":
        return np.array([K, 0, min(r["it2"], K)], np.int32)
    D = len(r["shape"])
    return np.array([[K] * D, [0] * D, [min(i, K) for i in r["it2"]]], np.int32)


def residual_by_workgroup(name):
    """[systems, nblk] bool: the workgroup holds a cell with a non-zero first residual (max|r| partial of the init kernel), from the twin's
    arithmetic alone"""
    r = BY_NAME[name]
    i = inputs(name)
    var, bnd = r["variant"], r["bnd"]
    if var == "closed":
        b = sref.rhs(i["vel"], bnd, F32)
    elif var in ("liquid", "gf"):
        b = lref.rhs(i["vel"], i["liquid"], F32)
    elif var == "diffuse":
        b = dref.first_residual(dref.planar(i["vel"]).astype(F32), dref.pair_alpha(i["alpha"], r["B"], len(r["shape"]), F32), bnd)
    else:
        b = pref.rhs(i["vel"], i["obstacle"], bnd, F32)
    v = np.abs(b).reshape(b.shape[0], -1)
    return cg_ref.block_partials(v, F32, np.maximum) > 0


# ---- wrong orders a row must tell apart (tests/test_cg_cases_host.py; nothing of this runs on a GPU) -----------------------------------------
def _first_trip_only(partials, dtype):
    return cg_ref.entry_sum(partials[:, :K_THREADS], dtype)


def _shifted_trips(partials, dtype):
    """partial t + 256 goes to thread t + 1 (thread 255's to thread 0)"""
    E, n = partials.shape
    trips = -(-n // K_THREADS)
    p = np.zeros((E, trips * K_THREADS), dtype)
    p[:, :n] = partials
    p = p.reshape(E, trips, K_THREADS)
    p[:, 1:] = np.roll(p[:, 1:], 1, axis=2)
    return cg_ref.entry_sum(p.reshape(E, -1), dtype)


def _lane_order(v, op):
    """[..., 256]: the 64 lanes of a wave added in ascending order instead of the butterfly"""
    w = v.reshape(v.shape[:-1] + (K_THREADS // cg_ref.WAVE, cg_ref.WAVE))
    acc = w[..., 0].copy()
    for l in range(1, cg_ref.WAVE):
        acc = op(acc, w[..., l])
    out = acc[..., 0]
    for k in range(1, acc.shape[-1]):
        out = op(out, acc[..., k])
    return out


MUTANTS = {
    "lost-partials": lambda a, b: cg_ref.ordered_dot(a, b, combine=_first_trip_only),
    "shifted-trip": lambda a, b: cg_ref.ordered_dot(a, b, combine=_shifted_trips),
    "numpy-order": cg_ref.numpy_dot,
    "lane-order": lambda a, b: cg_ref.ordered_dot(a, b, partials=lambda v, dt: cg_ref.block_partials(v, dt, waves=_lane_order)),
}
LARGE_ONLY = ("lost-partials", "shifted-trip")       # the same sum by construction up to 256 workgroups


# ---- the entry points of the raw C ABI: variant -> kind -> (name pattern, argument names) ------------------------------------------------------
# Pointers: vel pressure ws flags phi alpha out hier count iters.  Scalars: ws_bytes hier_bytes dim B Z Y X bnd os k acc max_iter gf_clamp
# mg_alpha stream.  ``S`` reads "B systems" (B, or B*D for a diffusion's status), ``dims`` is B[, Z], Y, X, ``dims4`` B, Z, Y, X (Z = 1 in 2-D).
def entry_points(r):
    """kind -> (entry point, [argument names]) for the row; kinds: bytes, init, direction, update, status, correct and, by variant, finish,
    hier_bytes, build, precondition"""
    nd = len(r["shape"])
    var = r["variant"]
    d = "%dd" % nd
    dims = ["B"] + (["Z"] if nd == 3 else []) + ["Y", "X"]
    fl = ["flags"] if has_flags(r) else []
    sfx = d + ("_flags" if fl else "")
    e = {"status": ("df_pressure_status", ["ws", "ws_bytes", "S", "Z", "Y", "X", "k", "count", "iters", "stream"])}
    plain = {
        "bytes": ("df_pressure_workspace_bytes", ["B", "Z", "Y", "X"]),
        "init": ("df_pressure_init" + sfx, ["vel", "pressure", "ws", "ws_bytes"] + fl + dims + ["bnd", "stream"]),
        "direction": ("df_pressure_cg_direction" + sfx, ["ws", "ws_bytes"] + fl + dims + ["bnd", "k", "acc", "max_iter", "stream"]),
        "update": ("df_pressure_cg_update" + sfx, ["pressure", "ws", "ws_bytes"] + fl + dims + ["bnd", "k", "stream"]),
        "correct": ("df_pressure_correct" + sfx, ["vel", "pressure", "out"] + fl + dims + ["bnd", "stream"]),
    }
    if var in ("closed", "obstacle"):
        e.update(plain)
    elif var in ("open", "obsopen"):
        e.update(plain)
        e["direction"] = ("df_pressure_cg_direction%s_open" % d, ["ws", "ws_bytes", "flags"] + dims + ["bnd", "os", "k", "acc", "max_iter", "stream"])
        e["correct"] = ("df_pressure_correct%s_open" % d, ["vel", "pressure", "out", "flags"] + dims + ["bnd", "os", "stream"])
    elif var == "liquid":
        e.update(plain)
        e["direction"] = ("df_pressure_cg_direction%s_liquid" % d, ["ws", "ws_bytes", "flags"] + dims + ["bnd", "k", "acc", "max_iter", "stream"])
        e["correct"] = ("df_pressure_correct%s_liquid" % d, ["vel", "pressure", "out", "flags"] + dims + ["bnd", "stream"])
    elif var == "gf":
        e["bytes"] = ("df_pressure_workspace_bytes_gf", ["B", "Z", "Y", "X"])
        e["init"] = ("df_pressure_init%s_gf" % d, ["vel", "pressure", "ws", "ws_bytes", "flags", "phi"] + dims + ["bnd", "gf_clamp", "stream"])
        e["direction"] = ("df_pressure_cg_direction%s_gf" % d, ["ws", "ws_bytes", "flags"] + dims + ["bnd", "k", "acc", "max_iter", "stream"])
        e["update"] = ("df_pressure_cg_update%s_gf" % d, ["pressure", "ws", "ws_bytes", "flags"] + dims + ["bnd", "k", "stream"])
        e["correct"] = ("df_pressure_correct%s_gf" % d, ["vel", "pressure", "out", "flags", "phi"] + dims + ["bnd", "gf_clamp", "stream"])
    elif var == "diffuse":
        e["bytes"] = ("df_diffuse_workspace_bytes", ["B", "Z", "Y", "X", "dim"])
        e["init"] = ("df_diffuse_init" + d, ["vel", "alpha", "ws", "ws_bytes"] + dims + ["bnd", "stream"])
        e["direction"] = ("df_diffuse_cg_direction" + d, ["alpha", "ws", "ws_bytes"] + dims + ["bnd", "k", "acc", "max_iter", "stream"])
        e["update"] = ("df_diffuse_cg_update" + d, ["ws", "ws_bytes"] + dims + ["bnd", "k", "stream"])
        e["finish"] = ("df_diffuse_finish" + d, ["ws", "ws_bytes", "out"] + dims + ["bnd", "stream"])
    else:
        dims4 = ["dim", "B", "Z", "Y", "X"]
        e.update(plain)
        e["hier_bytes"] = ("df_mg_hierarchy_bytes", dims4)
        e["build"] = ("df_mg_build", ["hier", "hier_bytes", "flags"] + dims4 + ["bnd", "os", "stream"])
        e["precondition"] = ("df_pressure_mg_precondition", ["hier", "hier_bytes", "ws", "ws_bytes"] + dims4 + ["mg_alpha", "k", "stream"])
        e["direction"] = ("df_pressure_cg_direction_mg", ["ws", "ws_bytes", "hier", "hier_bytes", "flags"] + dims4 + ["bnd", "os", "k", "acc", "max_iter", "stream"])
        e["update"] = ("df_pressure_cg_update_mg", ["pressure", "ws", "ws_bytes", "flags"] + dims4 + ["bnd", "k", "stream"])
        if open_bits(r):
            e["correct"] = ("df_pressure_correct%s_open" % d, ["vel", "pressure", "out", "flags"] + dims + ["bnd", "os", "stream"])
    return e


POINTERS = ("vel", "pressure", "ws", "flags", "phi", "alpha", "out", "hier", "count", "iters")
