"""The table of tests/test_gpu_particle_edges.py and tests/test_particle_cases_host.py: one row per branch of the host code and the kernels
of csrc/particles.hip and csrc/liquid.hip (the particle, FLIP, ghost-fluid level-set and resampling blocks of include/deepfluids_hip.h),
the seeded inputs of a row, and its result by the NumPy restatements (particles_ref, liquid_ref, liquid_gf_ref, liquid_resample_ref) in
fp64 or in their fp32 twin.  Plain data and NumPy; no torch import.

A row: name, op (a key of OPS), shape [(Z,)Y,X], B, N (the capacity per entry: P = B*N rows), bnd, off (payload offset of every float /
int32 operand in elements and of every byte operand in bytes: 0 = aligned, 1 = loose), twin (the aligned row a loose row must give the
bits of), axes (which axes of the issue's list the row sets), and per op:
  place    'std' specials first (both clamp limits of every axis, integer and half-integer coordinates, cell 0 and the last cell), then
           uniform over the whole grid;  ('crowd', n) n particles in one cell;  'low' the lower 45 % in y only
  fill     'even' N rows per entry;  'first' every row in entry 0, the other entries empty;  unused = rows behind entry_start[B]
  ragged   None (dense entry point) | 'dense' (entry_start[b] = b*N) | 'empty_first' | 'empty_last' | 'unused' | 'nonmono'
  hostile  a tuple of 'pos', 'vel', 'order', 'cell_start', 'entry_start', 'flags', 'new_start', 'seeds', 'overflow'
  rf, mode, band, layer, inside, minp, maxp, null (outputs passed as NULL), inplace
Hostile index values are off by at most 5 elements (the guard zones of gpu_util are 64 floats = 21 records wide)."""
import zlib

import numpy as np

import liquid_gf_ref as gref
import liquid_ref as lref
import liquid_resample_ref as rref
import particles_ref as pref
from smoke_ref import interior_mask

THREADS = 256                       # dfst::kThreads: cells or particles per workgroup
DT, VEL_SCALE = 1.0, 2.5            # the trace rows
FLIP = 0.97
FORCE = (0.25, -0.5, 0.125)
BOUND_VALUE = 0.5
SEED, STEP = 123, 7                 # the scatter rows

# op -> (entry point pattern, inputs, outputs); an operand is (name, kind), kind f32 | i32 | i64 | u8.  `d` is the dimensionality, `r`
# is '_ragged' for a ragged row.  In-place entry points list their arrays as inputs AND outputs.
OPS = {
    "trace": ("df_particles_advect%(d)dd%(r)s", [("pos", "f32"), ("vel", "f32"), ("es", "i32")], [("pos_out", "f32")]),
    "keys": ("df_particles_cell_keys%(d)dd%(r)s", [("pos", "f32"), ("es", "i32")], [("keys", "i32")]),
    "gather": ("df_particles_gather", [("pos", "f32"), ("order", "i64")], [("pos_sorted", "f32")]),
    "union": ("df_particle_levelset_union%(d)dd", [("sp", "f32"), ("cs", "i32")], [("phi", "f32")]),
    "averaged": ("df_particle_levelset_averaged%(d)dd", [("sp", "f32"), ("cs", "i32")], [("phi", "f32")]),
    "smooth": ("df_levelset_smooth%(d)dd", [("phi_in", "f32")], [("phi", "f32")]),
    "p2g": ("df_liquid_p2g%(d)dd", [("sp", "f32"), ("spvel", "f32"), ("cs", "i32")], [("vel", "f32"), ("weight", "f32"), ("known", "u8")]),
    "extrap": ("df_mac_extrapolate%(d)dd", [("vel", "f32"), ("mark", "u8")], [("vel_out", "f32"), ("mark_out", "u8")]),
    "flags": ("df_liquid_flags%(d)dd", [("cs", "i32")], [("flags", "u8"), ("touch", "u8")]),
    "forces": ("df_liquid_forces%(d)dd", [("vel", "f32"), ("flags", "u8")], [("out", "f32")]),
    "flip": ("df_flip_update%(d)dd%(r)s", [("pos", "f32"), ("pvel", "f32"), ("vel", "f32"), ("vel_old", "f32"), ("es", "i32")],
             [("pvel_out", "f32")]),
    "marks": ("df_levelset_extrapolate_marks%(d)dd", [("phi", "f32")], [("mark", "u8")]),
    "layer": ("df_levelset_extrapolate_layer%(d)dd", [("phi", "f32"), ("mark", "u8")], [("phi", "f32"), ("mark", "u8")]),
    "count": ("df_resample_count%(d)dd", [("sp", "f32"), ("cs", "i32"), ("phi", "f32"), ("flags", "u8")],
              [("keep", "u8"), ("kept", "i32"), ("seeds", "i32")]),
    "scatter": ("df_resample_scatter%(d)dd", [("sp", "f32"), ("spvel", "f32"), ("cs", "i32"), ("keep", "u8"), ("seeds", "i32"),
                                               ("new_start", "i32"), ("vel", "f32")], [("pos_out", "f32"), ("pvel_out", "f32")]),
}
# what one element of an operand belongs to: a particle row [P(,D)], a batch entry [B,...], an (entry, cell) [B*ncell] or a range end
# [B*ncell + 1]; None: neither (entry_start; the sort order)
EXTENT = dict(pos="row", pvel="row", sp="row", spvel="row", keep="row", pos_out="row", pvel_out="row", keys="row", pos_sorted="row",
              vel="entry", vel_old="entry", phi="entry", phi_in="entry", mark="entry", flags="entry", vel_out="entry", mark_out="entry",
              weight="entry", known="entry", touch="entry", out="entry", kept="cell", seeds="cell", cs="range", new_start="range", es=None,
              order=None)
assert all(n in EXTENT for _, ins, outs in OPS.values() for n, _ in ins + outs)
# compared with the fp64 restatement under the suite's standing rule (distance <= 3 * e32 + 1e-7); everything else bit for bit with the twin
TOLERANCE_OPS = ("trace", "union", "averaged")
# kernels that take their block from xcd_block(bid, nblk, 0)
REMAPPED_OPS = ("union", "averaged", "p2g", "extrap", "count", "scatter")
PARTICLE_THREAD_OPS = ("trace", "keys", "flip", "gather")
RADIUS_FACTORS = pref.RADIUS_FACTORS

# cell-per-thread grids by block count ceil(B*Z*Y*X / 256): (B, shape).  8 has B = 2; 17 is 3-D with odd extents and B = 2
GRIDS = {1: (1, (5, 7)), 7: (1, (41, 43)), 8: (2, (23, 44)), 9: (1, (47, 47)), 17: (2, (9, 11, 21))}
# particle counts B*N: (B, N)
COUNTS = {1: (1, 1), 255: (1, 255), 256: (2, 128), 257: (1, 257), 771: (3, 257)}
MID = {2: (9, 13), 3: (5, 7, 9)}    # odd on every axis


def entry_point(r):
    return OPS[r["op"]][0] % dict(d=len(r["shape"]), r="_ragged" if r.get("ragged") else "")


def _row(name, op, shape, B, N, axes, **kw):
    r = dict(name=name, op=op, shape=tuple(shape), B=B, N=N, bnd=1, off=0, twin=None, axes=axes, place="std", fill="even", unused=0,
             ragged=None, hostile=(), rf=1.0, mode=1, band=0, layer=2 if op == "layer" else 1, inside=1, minp=2, maxp=4, null=(), inplace=False)
    assert set(kw) <= set(r), kw
    r.update(kw)
    return r


def _rows():
    out = []

    def add(*a, **kw):
        out.append(_row(*a, **kw))

    # ---- geometry: block counts of the cell-per-thread kernels (the xcd_block remainder: rem = 1, 7, 0, 1 and q = 0, 0, 1, 1, 2) ----
    for op in REMAPPED_OPS + ("smooth", "flags", "forces", "marks", "layer"):
        for nblk, (B, shape) in sorted(GRIDS.items()):
            if op not in REMAPPED_OPS and nblk in (7, 9):
                continue
            kw = dict(rf=0.5) if nblk == 17 else {}
            N = 300
            if op in ("count", "scatter"):                  # 300 live rows and room for two seeds in every cell
                N = 300 + 2 * int(np.prod(shape))
                kw.update(unused=B * N - 300)
            add("%s-blk%d" % (op, nblk), op, shape, B, N, "blocks", **kw)
    # ---- geometry: particle counts of the particle-per-thread kernels, odd extents, B = 2 and 3 ----
    for op in PARTICLE_THREAD_OPS:
        for n, (B, N) in sorted(COUNTS.items()):
            for d in (2, 3):
                add("%s-%dd-n%d" % (op, d, n), op, MID[d], B, N, "counts")
    # ---- geometry: minimum extents ----
    for d in (2, 3):
        for op in ("keys", "union", "averaged", "smooth", "marks", "layer"):
            add("%s-%dd-min" % (op, d), op, (2,) * d, 2, 40, "min", rf=2.0 if op in ("union", "averaged") else 1.0)
        for bnd in (1, 2):
            for op in ("trace", "p2g", "extrap", "flags", "forces", "flip", "count", "scatter"):
                kw = dict(unused=40) if op in ("count", "scatter") else {}
                if op == "scatter" and bnd == 2:
                    continue                                # the scatter takes no bnd
                add("%s-%dd-min-b%d" % (op, d, bnd), op, (2 * bnd + 2,) * d, 2, 40, "min", bnd=bnd, **kw)
    # ---- the mid rows of every op (odd extents, B = 2: the last workgroup of entry 0 holds cells / particles of entry 1), their loose twins ----
    for d in (2, 3):
        for op in sorted(OPS):
            kw = dict(unused=300) if op in ("count", "scatter") else {}
            if op in ("trace", "keys", "flip"):
                add("%s-%dd-ragged-dense" % (op, d), op, MID[d], 2, 300, "ragged", ragged="dense")
                add("%s-%dd-ragged-dense-loose" % (op, d), op, MID[d], 2, 300, "align", ragged="dense", off=1, twin="%s-%dd-ragged-dense" % (op, d))
            add("%s-%dd-mid" % (op, d), op, MID[d], 2, 300, "odd,B2", **kw)
            add("%s-%dd-mid-loose" % (op, d), op, MID[d], 2, 300, "align", off=1, twin="%s-%dd-mid" % (op, d), **kw)
    # ---- placement ----
    for d in (2, 3):
        for op in ("keys", "union", "averaged", "p2g", "count", "scatter"):
            kw = dict(unused=300, maxp=8) if op in ("count", "scatter") else {}
            add("%s-%dd-crowd" % (op, d), op, MID[d], 2, 500 if kw else 400, "crowd", place=("crowd", 320), **kw)
        for op in ("union", "averaged", "p2g", "flags", "count", "scatter"):
            kw = dict(unused=150) if op in ("count", "scatter") else {}
            add("%s-%dd-empty-entry" % (op, d), op, MID[d], 2, 150, "empty entry", fill="first", **kw)
        for op in ("union", "averaged", "p2g", "flags"):
            add("%s-%dd-n0" % (op, d), op, MID[d], 2, 0, "N=0")
        for op in ("trace", "keys", "flip"):
            add("%s-%dd-n0" % (op, d), op, MID[d], 2, 0, "N=0")
    add("p2g-2d-no-known", "p2g", MID[2], 2, 300, "null", null=("known",))
    add("p2g-3d-no-known", "p2g", MID[3], 2, 300, "null", null=("known",))
    add("flags-2d-no-touch", "flags", MID[2], 2, 300, "null", null=("touch",))
    add("flags-3d-no-touch", "flags", MID[3], 2, 300, "null", null=("touch",))
    # ---- windows ----
    for d in (2, 3):
        for op in ("union", "averaged"):
            for ext in (2, 3, 4):
                add("%s-%dd-wide%d" % (op, d, ext), op, (ext,) * d, 2, 30, "window", rf=2.0)
            for rf in RADIUS_FACTORS:
                add("%s-%dd-rf%g" % (op, d, rf), op, MID[d], 2, 200, "window", rf=rf)
        for mode in (0, 1, 2):
            for band in (0, 1, 7):                          # 7 >= half of every extent of MID: every cell is banded
                add("smooth-%dd-m%d-band%d" % (d, mode, band), "smooth", MID[d], 2, 0, "window", mode=mode, band=band)
        add("smooth-%dd-m0-inplace" % d, "smooth", MID[d], 2, 0, "in place", mode=0, band=1, inplace=True)
        for layer in (1, 2, 254):
            add("extrap-%dd-layer%d" % (d, layer), "extrap", MID[d], 2, 0, "window", layer=layer)
            if layer >= 2:
                add("layer-%dd-layer%d" % (d, layer), "layer", MID[d], 2, 0, "window", layer=layer, inside=layer % 2)
        add("marks-%dd-outside" % d, "marks", MID[d], 2, 0, "window", inside=0)
    # ---- ragged forms, in place ----
    for d in (2, 3):
        for op in ("trace", "keys", "flip"):
            for form in ("empty_first", "empty_last", "unused"):
                add("%s-%dd-ragged-%s" % (op, d, form), op, MID[d], 3, 100, "ragged", ragged=form)
            add("%s-%dd-ragged-b2-257" % (op, d), op, MID[d], 2, 257, "ragged", ragged="unused")
        add("trace-%dd-inplace" % d, "trace", MID[d], 2, 300, "in place", inplace=True)
        add("flip-%dd-inplace" % d, "flip", MID[d], 2, 300, "in place", inplace=True)
        add("forces-%dd-inplace" % d, "forces", MID[d], 2, 0, "in place", inplace=True)
    # ---- documented hostile inputs ----
    for d in (2, 3):
        for op in ("trace", "keys", "p2g", "flip", "union", "averaged"):
            add("%s-%dd-hostile-pos" % (op, d), op, MID[d], 2, 300, "hostile", hostile=("pos",))
        add("count-%dd-hostile-pos" % d, "count", MID[d], 1, 300, "hostile", hostile=("pos",), unused=100)
        for op in ("trace", "flip"):
            add("%s-%dd-hostile-vel" % (op, d), op, MID[d], 2, 300, "hostile", hostile=("vel",))
            add("%s-%dd-hostile-entry-start" % (op, d), op, MID[d], 3, 100, "hostile", ragged="nonmono", hostile=("entry_start",))
        add("keys-%dd-hostile-entry-start" % d, "keys", MID[d], 3, 100, "hostile", ragged="nonmono", hostile=("entry_start",))
        add("gather-%dd-hostile-order" % d, "gather", MID[d], 1, 300, "hostile", hostile=("order",))
        for op in ("union", "averaged", "p2g", "flags"):
            add("%s-%dd-hostile-cell-start" % (op, d), op, MID[d], 2, 300, "hostile", hostile=("cell_start",))
        # B = 1 and max_particles = 8192: overlapping ranges then write the same byte from every cell that holds a row
        add("count-%dd-hostile-cell-start" % d, "count", MID[d], 1, 300, "hostile", hostile=("cell_start", "flags"), unused=100, maxp=8192)
        add("forces-%dd-hostile-flags" % d, "forces", MID[d], 2, 0, "hostile", hostile=("flags",))
        # every row live: cell_start[B*ncell] is then the capacity itself and the values planted at both ends clamp back to what they were
        add("scatter-%dd-hostile-cell-start" % d, "scatter", MID[d], 1, 300, "hostile", hostile=("cell_start",), maxp=8192)
        add("scatter-%dd-hostile-starts" % d, "scatter", MID[d], 1, 300, "hostile", hostile=("new_start", "seeds"), unused=200, place="low")
    # N is the wanted total minus 3: the last three rows of the result do not fit (inputs() asserts that)
    add("scatter-2d-overflow", "scatter", MID[2], 1, OVERFLOW_N[2], "hostile", hostile=("overflow",), unused=OVERFLOW_N[2] - 60, place="low")
    add("scatter-3d-overflow", "scatter", MID[3], 1, OVERFLOW_N[3], "hostile", hostile=("overflow",), unused=OVERFLOW_N[3] - 60, place="low")
    names = [r["name"] for r in out]
    assert len(set(names)) == len(names)
    return out


OVERFLOW_LIVE = 60
OVERFLOW_N = {2: 92, 3: 100}
ROWS = _rows()
BY_NAME = {r["name"]: r for r in ROWS}


def rows(op=None, **match):
    return [r for r in ROWS if (op is None or r["op"] == op) and all(r[k] == v for k, v in match.items())]


def names(op=None, **match):
    return [r["name"] for r in rows(op, **match)]


def block_count(r):
    """workgroups of the row's launch: cells for the cell-per-thread kernels, rows for the particle-per-thread ones"""
    n = r["B"] * r["N"] if r["op"] in PARTICLE_THREAD_OPS else r["B"] * int(np.prod(r["shape"]))
    return -(-n // THREADS)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _rng(r, salt=0):
    # a loose row draws what its aligned twin draws
    return np.random.RandomState((zlib.crc32((r["twin"] or r["name"]).encode()) + salt) % (2 ** 31))


def special_positions(shape, bnd):
    """[M,D] float32: exactly on both clamp limits of every axis, on integer and on half-integer coordinates (the s1 == 0 ties of both
    frames), in cell 0 and in the last cell"""
    D = len(shape)
    ext = shape[::-1]
    lo, hi = pref.clamp_bounds(shape, bnd, np.float32)
    top = np.array(ext, np.float32)
    out = [np.full(D, lo, np.float32), hi.copy(), np.full(D, 0.25, np.float32), top - np.float32(0.25), np.full(D, 1.0, np.float32),
           np.full(D, 0.5, np.float32), np.full(D, 1.5, np.float32), top - np.float32(0.5), top - np.float32(1.0), np.zeros(D, np.float32)]
    mid = np.array([0.5 * e + 0.125 for e in ext], np.float32)
    for a in range(D):
        for val in (lo, hi[a], 0.0, 1.0, 0.5, 1.5, ext[a] - 1.0, ext[a] - 0.5, ext[a] - 1.5):
            p = mid.copy()
            p[a] = val
            out.append(p)
    return np.stack(out).astype(np.float32)


def hostile_positions(shape):
    """[M,D] float32: NaN, +inf, -inf, -1, exactly the extent and 1e30, alone on an axis and on all of them"""
    D = len(shape)
    ext = shape[::-1]
    mid = np.array([0.5 * e + 0.125 for e in ext], np.float32)
    out = []
    for val in (np.nan, np.inf, -np.inf, -1.0, None, 1e30):
        out.append(np.array([ext[a] if val is None else val for a in range(D)], np.float32))
        for a in range(D):
            p = mid.copy()
            p[a] = ext[a] if val is None else val
            out.append(p)
    return np.stack(out)


def _particles(r):
    """(pos [P,D] float32 with NaN in the unused rows, entry_start [B+1] int32)"""
    rng = _rng(r)
    shape, B, N = r["shape"], r["B"], r["N"]
    D, P = len(shape), B * N
    ext = np.array(shape[::-1], np.float64)
    live = P - r["unused"]
    assert live >= 0
    if r["ragged"] in ("empty_first", "nonmono"):
        counts = [0, N + 7] + [N - 7] * (B - 2) if B > 2 else [0, P]
    elif r["ragged"] == "empty_last":
        counts = [N + 5] + [N - 5] * (B - 2) + [0]
    elif r["ragged"] == "unused":
        counts = [N - 9] + [N + 2] * (B - 1)                 # 9 - 2*(B-1) > 0 rows stay unused
    elif r["fill"] == "first":
        counts = [live] + [0] * (B - 1)
    else:
        counts = [live // B + (1 if b < live % B else 0) for b in range(B)]
    assert sum(counts) <= P and min(counts) >= 0, counts
    parts = []
    for b, n in enumerate(counts):
        span = ext.copy()
        if r["place"] == "low":
            span[1] = 0.45 * ext[1]
        p = (rng.uniform(0, 1, size=(n, D)) * span).astype(np.float32)
        if r["place"] == "std":
            sp = special_positions(shape, r["bnd"])
            m = min(n, len(sp))
            p[:m] = sp[:m]
            if "pos" in r["hostile"]:
                hp = hostile_positions(shape)
                at = np.linspace(m, n - 1, len(hp)).astype(int) if n >= m + len(hp) else np.arange(0)
                p[at] = hp[:len(at)]
        elif isinstance(r["place"], tuple) and b == B - 1:
            cell = np.floor(0.25 * ext)                      # below the surface of _phi: deep for the resampling
            k = min(r["place"][1], n)
            p[:k] = (cell + rng.uniform(0.01, 0.99, size=(k, D))).astype(np.float32)
        parts.append(p)
    pos = np.full((P, D), np.nan, np.float32)
    if sum(counts):
        pos[:sum(counts)] = np.concatenate(parts)
    es = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    if r["ragged"] == "nonmono":
        es[1], es[2] = es[2], es[1] + 3                      # not monotone: 0, N+7, 3, ... -- the bisection still ends in [-1, B-1]
    return pos, es


def _velocity(r, salt, scale=0.8):
    D = len(r["shape"])
    v = (scale * _rng(r, salt).standard_normal((r["B"],) + r["shape"] + (D,))).astype(np.float32)
    if "vel" in r["hostile"]:
        flat = v.reshape(r["B"], -1, D)
        n = flat.shape[1]
        for b in range(r["B"]):
            for k, val in enumerate((np.nan, np.inf, -np.inf)):
                flat[b, (n // 7) * (k + 1) + b, k % D] = val
                flat[b, (n // 5) * (k + 1) + b, :] = val
    return v


def _hostile_ranges(cs, X, total):
    """-3, total + 1 .. total + 5, and a pair with start > end, in the cells around cell (0, 0[, 0]) of entry 0 (which the threads of its
    first two rows read); every value within 5 elements of the array"""
    cs = cs.copy()
    cs[0] = -3
    cs[2:7] = total + np.arange(1, 6)
    cs[X + 1], cs[X + 2] = min(total, 9), min(total, 4)      # start > end: an empty range
    cs[X + 3] = total + 2
    return cs


def _hostile_ends(cs, total):
    """the scatter's: -3 in front of the first range and total + 5 behind the last one, which clamp back to 0 and total (every row is
    live), and a pair with start > end: that cell is empty and the cell in front of it also walks its rows.  With kept and new_start
    taken from the clamped ranges no two cells write one row."""
    cs = cs.copy()
    assert cs[0] == 0 and cs[-1] == total
    c = int(np.flatnonzero(np.diff(cs[1:-1]) > 0)[0]) + 1
    cs[c] = cs[c + 1] + 2
    cs[0], cs[-1] = -3, total + 5
    return cs


DECOYS = (3, 5)                     # finite records in front of and behind the rows of the union's hostile cell_start rows


def decoy_position(D):
    """the centre of cell (1, 0[, 0]): its thread reads cell_start[0] as a start and cell_start[4] as an end"""
    return np.array([1.5, 0.5, 0.5][:D], np.float32)


def _sorted_state(r):
    pos, es = _particles(r)
    shape, B = r["shape"], r["B"]
    ncell = int(np.prod(shape))
    rng = _rng(r, 1)
    pvel = np.where(np.arange(len(pos))[:, None] >= es[-1], np.nan, rng.standard_normal(pos.shape)).astype(np.float32)
    sp, spvel, cs, order = rref.sort(pos, pvel, es, shape)
    out = dict(sp=sp, spvel=spvel, es=es, live=int(es[-1]), ncell=ncell)
    if "cell_start" in r["hostile"]:
        cs = _hostile_ends(cs, len(pos)) if r["op"] == "scatter" else _hostile_ranges(cs, shape[-1], len(pos))
        if r["op"] == "union":
            # fminf drops a NaN, so a read of the NaN-filled guard would not show: the hostile ends land on finite decoy records that
            # lie in the payload, outside the B*N rows the call is told about, at a cell centre no particle sits on
            assert not (sp == decoy_position(sp.shape[1])).all(axis=1).any()
            lead, tail = (np.tile(decoy_position(sp.shape[1]), (n, 1)) for n in DECOYS)
            out["padded"] = dict(sp=(np.concatenate([lead, sp, tail]).astype(np.float32), DECOYS[0] * sp.shape[1]))
        if r["op"] == "scatter":
            # the records behind row B*N that cell_start[B*ncell] = B*N + 5 lands on: finite decoys inside the payload, not the guard,
            # whose NaN pattern is also the fill of the outputs (copying it into a row that must keep the fill would not show)
            tail = np.tile(decoy_position(sp.shape[1]), (DECOYS[1], 1))
            out["padded"] = dict(sp=(np.concatenate([sp, tail]).astype(np.float32), 0),
                                 spvel=(np.concatenate([spvel, -tail]).astype(np.float32), 0))
    out["cs"] = cs.astype(np.int32)
    return out


def _phi(r, salt=3):
    """a surface at 0.6 of the height with noise, exact zeros, and planted NaN / +-inf on the hostile rows"""
    shape, B = r["shape"], r["B"]
    rng = _rng(r, salt)
    yc = pref._centre(shape, 1, np.float64)
    phi = np.stack([np.broadcast_to(yc - 0.6 * shape[-2], shape) + 0.3 * rng.standard_normal(shape) for _ in range(B)]).astype(np.float32)
    flat = phi.reshape(-1)
    flat[rng.choice(flat.size, size=max(flat.size // 16, 1), replace=False)] = 0.0
    return phi


_INPUTS = {}


def inputs(r):
    """the operands of a row by name (float32 / int32 / int64 / uint8 NumPy arrays, None = passed as NULL); computed once, read-only"""
    if r["name"] not in _INPUTS:
        _INPUTS[r["name"]] = _build(r)
    return _INPUTS[r["name"]]


def _build(r):
    op, shape, B, N, bnd = r["op"], r["shape"], r["B"], r["N"], r["bnd"]
    D, P = len(shape), B * N
    grid = (B,) + shape
    rng = _rng(r, 11)
    if op in ("trace", "keys", "flip"):
        pos, es = _particles(r)
        if not r["ragged"]:
            assert (es == np.arange(B + 1) * N).all()
        i = dict(pos=pos if P else None, es=es if r["ragged"] else None)
        if op == "trace":
            i["vel"] = _velocity(r, 5)
        if op == "flip":
            i["vel"], i["vel_old"] = _velocity(r, 5), _velocity(r, 6)
            pv = rng.standard_normal((P, D)).astype(np.float32)
            if "vel" in r["hostile"] and P:
                pv[[3, P // 2, P - 2], [0, 1, D - 1]] = (np.nan, np.inf, -np.inf)
            i["pvel"] = pv if P else None
        return i
    if op == "gather":
        pos = (rng.uniform(0, 1, size=(P, D)) * 9).astype(np.float32)
        order = rng.permutation(P).astype(np.int64)
        if "order" in r["hostile"]:
            order[[0, P // 3, P // 2, P - 1]] = (-1, P, P + 3, -1)
        return dict(pos=pos, order=order)
    if op in ("union", "averaged", "p2g", "flags"):
        if P == 0:
            return dict(sp=None, spvel=None, cs=None, live=0)
        return _sorted_state(r)
    if op == "smooth":
        return dict(phi_in=_phi(r))
    if op in ("marks", "layer"):
        phi = _phi(r)
        flat = phi.reshape(-1)
        flat[rng.choice(flat.size, size=3, replace=False)] = (np.nan, np.inf, -np.inf)        # non-finite phi changes numbers, never addresses
        i = dict(phi=phi)
        if op == "layer":
            L = r["layer"]
            # the marks of the marks call and the layers before it, and, to reach every layer number, arbitrary bytes: a launch writes
            # cells marked 0 only and reads cells marked `layer` only, so any marks give a deterministic result
            m = rref.extrapolate_marks(phi, bool(r["inside"]))
            if L > 2:
                m = rng.choice(np.array([0, 0, 0, 1, 2, L - 1, L, L, L + 1 if L < 255 else 0], np.uint8), size=phi.shape)
            i["mark"] = m.astype(np.uint8)
        return i
    if op in ("extrap", "forces"):
        i = dict(vel=_velocity(r, 5))
        if op == "extrap":
            L = r["layer"]
            i["mark"] = rng.choice(np.array([0, 0, 0, 1, 2, L, min(L + 1, 255), 255], np.uint8), size=grid + (D,)).astype(np.uint8)
        else:
            liquid = (rng.uniform(size=grid) < 0.4) & interior_mask(shape, bnd)[None]
            f, _ = lref.flags_of(liquid)
            if "flags" in r["hostile"]:
                f = np.where(interior_mask(shape, bnd)[None], f, 0xFF).astype(np.uint8)     # believed only where interior by index
            i["flags"], i["liquid"] = f, liquid
        return i
    if op in ("count", "scatter"):
        s = _sorted_state(r)
        phi = _phi(r)
        inter = interior_mask(shape, bnd)[None]
        with np.errstate(invalid="ignore"):
            liquid = (lref.liquid_mask(s["cs"], B, shape, bnd) | (phi <= 0)) & inter
        f, _ = lref.flags_of(liquid)
        if "flags" in r["hostile"]:
            f = np.where(inter, f, 0xFF).astype(np.uint8)
        i = dict(sp=s["sp"], cs=s["cs"], phi=phi, flags=f, live=s["live"])
        if "padded" in s:
            i["padded"] = s["padded"]
        if op == "scatter":
            keep, kept, seeds = rref.resample_count(s["sp"], s["cs"], phi, f, bnd, r["minp"], r["maxp"], r["rf"], np.float32)
            keep = np.where(keep == 255, 0, keep).astype(np.uint8)
            seeds = seeds.copy()
            if "seeds" in r["hostile"]:
                # beyond min_particles on the last cell that holds anything (nothing behind it to collide with), negative on an empty one
                last = int(np.flatnonzero(kept + seeds)[-1])
                seeds[last] = r["minp"] + 3
                seeds[int(np.flatnonzero(kept + seeds == 0)[0])] = -2
            new_start = np.concatenate([[0], np.cumsum(kept.astype(np.int64) + pref.clamp_ranges(seeds, r["minp"]))])
            wanted = int(new_start[-1])
            if "overflow" in r["hostile"]:
                assert wanted - 3 == P, (r["name"], "OVERFLOW_N must be", wanted - 3)
            else:
                assert wanted + (5 if "cell_start" in r["hostile"] else 0) <= P, (r["name"], wanted, P)
            if "new_start" in r["hostile"]:
                # below 0 on the cell that legitimately starts at row 0, beyond the capacity on cells that hold nothing
                first = int(np.flatnonzero(kept + pref.clamp_ranges(seeds, r["minp"]))[0])
                new_start[:first + 1] = -3
                empty = np.flatnonzero(kept + pref.clamp_ranges(seeds, r["minp"]) == 0)
                empty = empty[empty > first][:5]
                new_start[empty] = P + 1 + np.arange(len(empty))
            i.update(spvel=s["spvel"], keep=keep, seeds=seeds.astype(np.int32), new_start=new_start.astype(np.int32), vel=_velocity(r, 5),
                     wanted=wanted)
        return i
    raise KeyError(op)


def scalars(r):
    """the scalar arguments between the extents and the stream, in the header's order"""
    D = len(r["shape"])
    op = r["op"]
    return {"trace": (DT, VEL_SCALE, r["bnd"]), "keys": (), "union": (r["rf"],), "averaged": (r["rf"],),
            "smooth": (r["mode"], r["band"], BOUND_VALUE), "p2g": (), "extrap": (r["bnd"], r["layer"]), "flags": (r["bnd"],),
            "forces": FORCE[:D] + (r["bnd"],), "flip": (FLIP,), "marks": (r["inside"],), "layer": (r["inside"], r["layer"]),
            "count": (r["bnd"], r["minp"], r["maxp"], r["rf"]), "scatter": (r["minp"], SEED, STEP), "gather": ()}[op]


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(r, dtype):
    """{output: (array, written)}: the row's result in ``dtype`` arithmetic; ``written`` is None (every element is written) or a bool
    mask of the elements the header says are written -- the others keep what they held.  Computed once, read-only."""
    key = (r["name"], np.dtype(dtype).name)
    if key not in _EXPECTED:
        _EXPECTED[key] = _restate(r, np.dtype(dtype).type)
    return _EXPECTED[key]


def _restate(r, dtype):
    op, shape, B, N, bnd = r["op"], r["shape"], r["B"], r["N"], r["bnd"]
    D, P = len(shape), B * N
    i = inputs(r)
    if op in ("trace", "keys", "flip"):
        if P == 0:
            return {OPS[op][2][0][0]: (np.zeros((0, D) if op != "keys" else (0,), np.int32 if op == "keys" else dtype), None)}
        es = i["es"] if r["ragged"] else (np.arange(B + 1) * N).astype(np.int32)
        live = rref.entries(es, P) >= 0
        rows = np.broadcast_to(live[:, None], (P, D))
        if op == "trace":
            return dict(pos_out=(rref.trace(i["pos"], i["vel"], es, DT, bnd, VEL_SCALE, dtype), rows))
        if op == "keys":
            return dict(keys=(rref.keys(i["pos"], es, shape), None))
        with np.errstate(invalid="ignore", over="ignore"):
            return dict(pvel_out=(rref.flip_update(i["pos"], i["pvel"], i["vel"], i["vel_old"], es, FLIP, dtype), rows))
    if op == "gather":
        return dict(pos_sorted=(pref.gather(i["pos"], i["order"]).astype(dtype), None))
    if op == "union":
        sp = np.zeros((0, D), np.float32) if P == 0 else i["sp"]
        return dict(phi=(pref.levelset_union_sorted(sp, i["cs"], shape, B, r["rf"], dtype), None))
    if op == "averaged":
        sp = np.zeros((B, 0, D), np.float32) if P == 0 else i["sp"].reshape(B, N, D)
        return dict(phi=(gref.levelset_raw(sp, i["cs"], shape, r["rf"], dtype), None))
    if op == "smooth":
        return dict(phi=(gref.smooth_pass(i["phi_in"].astype(dtype), r["mode"], r["band"], BOUND_VALUE), None))
    if op == "p2g":
        sp = np.zeros((B, 0, D), np.float32) if P == 0 else i["sp"].reshape(B, N, D)
        pv = sp if P == 0 else i["spvel"].reshape(B, N, D)
        vel, den, known = lref.p2g(sp, pv, i["cs"], shape, dtype)
        return dict(vel=(vel, None), weight=(den, None), known=(known, None))
    if op == "extrap":
        v, m = lref.extrapolate_layer(i["vel"].astype(dtype), i["mark"], r["layer"], bnd, dtype)
        return dict(vel_out=(v, None), mark_out=(m, None))
    if op == "flags":
        liquid = np.zeros((B,) + shape, bool) if P == 0 else lref.liquid_mask(i["cs"], B, shape, bnd)
        f, touch = lref.flags_of(liquid)
        return dict(flags=(f, None), touch=(touch, None))
    if op == "forces":
        return dict(out=(lref.forces(i["vel"], i["liquid"], FORCE[:D], bnd, dtype), None))
    if op == "marks":
        return dict(mark=(rref.extrapolate_marks(i["phi"], bool(r["inside"])), None))
    if op == "layer":
        ph, m = rref.extrapolate_layer(i["phi"].astype(dtype), i["mark"], r["layer"], bool(r["inside"]), dtype)
        return dict(phi=(ph, None), mark=(m, None))
    if op == "count":
        keep, kept, seeds = rref.resample_count(i["sp"], i["cs"], i["phi"], i["flags"], bnd, r["minp"], r["maxp"], r["rf"], dtype)
        return dict(keep=(keep, keep != 255), kept=(kept, None), seeds=(seeds, None))
    if op == "scatter":
        po, pv, written = rref.resample_scatter(i["sp"], i["spvel"], i["cs"], i["keep"], i["seeds"], i["new_start"], i["vel"], r["minp"], SEED,
                                                STEP, dtype)
        rows = np.broadcast_to(written[:, None], (P, D))
        return dict(pos_out=(po, rows), pvel_out=(pv, rows))
    raise KeyError(op)
