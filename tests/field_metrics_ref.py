"""NumPy restatement of the fused field metrics as include/deepfluids_hip_metrics.h defines them, in either precision:
``dtype=float64`` is the truth (every step in fp64; the order of a sum then does not matter at the level the tests look at), ``float32``
is the op-for-op twin of csrc/metrics.hip -- the per-cell terms and the per-thread sums in fp32, the sums across threads and workgroups
in fp64 in the header's order, rounded to fp32 once -- whose bits the kernels must give.  The differences are not re-derived: the
Jacobians and divergences are those of oracle/df_oracle.py, the twins the stencil tests already use (tests/stencil_ref.py).

Shared by tests/test_field_metrics_host.py (no GPU) and tests/test_gpu_field_metrics.py."""
import functools
import os
import re

import numpy as np

import df_oracle as orc

F32, F64 = np.float32, np.float64
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(name):
    src = open(os.path.join(_ROOT, "deep_fluids_amd", "csrc", "metrics.hip")).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, name
    return int(m.group(1))


K_THREADS, K_CELLS_PER_THREAD = _const("kThreads"), _const("kCellsPerThread")      # 256, 4
K_CELLS_PER_BLOCK = K_THREADS * K_CELLS_PER_THREAD                                 # 1024 cells per workgroup
WAVE = 64

# the word of every quantity in an output row, read from the header (the enum the ctypes binding also reads)
_HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(_ROOT, "include", "deepfluids_hip_metrics.h")).read(), flags=re.S)
WORD = {n[len("DF_FM_"):].lower(): int(v) for n, v in re.findall(r"(DF_FM_\w+)\s*=\s*(\d+)", _HDR)}
WORDS = WORD.pop("words")
INTS = ("count", "div_count", "argmax")
SUMS = ("sum_abs", "sum_sq", "sum_abs_x", "sum_sq_x", "sum_abs_jac", "sum_abs_div_g", "sum_abs_div_x")
MAXES = ("max_abs", "max_abs_div_g", "max_abs_div_x")
assert sorted(WORD) == sorted(INTS + SUMS + MAXES)


def _tree(v):
    """the wave tree of step 2: [..., 64] -> [...]"""
    v = v.copy()
    off = WAVE // 2
    while off > 0:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def _waves(v):
    """[..., 256] fp64 -> [...]: the tree inside each wave, then the wave sums in ascending order"""
    w = _tree(v.reshape(v.shape[:-1] + (K_THREADS // WAVE, WAVE)))
    acc = w[..., 0]
    for k in range(1, K_THREADS // WAVE):
        acc = acc + w[..., k]
    return acc


def ordered_sum(v, dtype):
    """v [B,N] in ``dtype``, 0 at the cells that are not counted (a thread's sums start at +0 and its terms are >= +0, so adding such a
    zero changes no bit) -> [B] in ``dtype``, summed in the header's order"""
    B, N = v.shape
    nblk = -(-N // K_CELLS_PER_BLOCK)
    p = np.zeros((B, nblk * K_CELLS_PER_BLOCK), dtype)
    p[:, :N] = v
    p = p.reshape(B, nblk, K_CELLS_PER_THREAD, K_THREADS)            # cell 1024 w + 256 i + t
    t = np.zeros((B, nblk, K_THREADS), dtype)
    for i in range(K_CELLS_PER_THREAD):                              # 1. per thread, ascending i, in dtype
        t = t + p[:, :, i]
    assert t.dtype == dtype
    blk = _waves(t.astype(F64))                                      # 2. [B, nblk] in fp64
    k = -(-nblk // K_THREADS)
    q = np.zeros((B, k * K_THREADS), F64)
    q[:, :nblk] = blk
    q = q.reshape(B, k, K_THREADS)                                   # 3. thread t: workgroups t, t + 256, ...
    a = np.zeros((B, K_THREADS), F64)
    for i in range(k):
        a = a + q[:, i]
    return _waves(a).astype(dtype)


def counted_cells(shape, mask):
    """bool [B, (Z,) Y, X] of the counted cells of fields [B,(Z,)Y,X,D]"""
    cells = tuple(shape[:-1])
    if mask is None:
        return np.ones(cells, bool)
    mask = np.asarray(mask)
    assert mask.shape in (cells, cells[1:]), (mask.shape, cells)
    return np.broadcast_to(mask != 0, cells).copy()


def metrics(g, x, mask=None, dtype=F32):
    """every quantity of the header as arrays [B]: the counts and ``argmax`` int32, the sums and maxima in ``dtype``"""
    g, x = np.asarray(g, dtype), np.asarray(x, dtype)
    assert g.shape == x.shape and g.shape[-1] == g.ndim - 2
    D, B = g.shape[-1], g.shape[0]
    cnt = counted_cells(g.shape, mask)
    d = g - x
    a1, a2, m = np.abs(d[..., 0]) + np.abs(d[..., 1]), d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1], np.fmax(np.abs(d[..., 0]), np.abs(d[..., 1]))
    x1, x2 = np.abs(x[..., 0]) + np.abs(x[..., 1]), x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]
    if D == 3:
        a1, a2, m = a1 + np.abs(d[..., 2]), a2 + d[..., 2] * d[..., 2], np.fmax(m, np.abs(d[..., 2]))
        x1, x2 = x1 + np.abs(x[..., 2]), x2 + x[..., 2] * x[..., 2]
    jg, jx = ((orc.jacobian3(g)[0], orc.jacobian3(x)[0]) if D == 3 else (orc.jacobian(g)[0], orc.jacobian(x)[0]))
    aj = np.zeros(g.shape[:-1], dtype)
    for a in range(D):                                               # axis x, y(, z); within it the components: J[..., k * D + a]
        for k in range(D):
            aj = aj + np.abs(jg[..., k * D + a] - jx[..., k * D + a])
    div = orc.divergence3 if D == 3 else orc.divergence
    inner = np.zeros(g.shape[:-1], bool)
    inner[(slice(None),) + (slice(0, -1),) * D] = True
    dg, dx = np.zeros(g.shape[:-1], dtype), np.zeros(g.shape[:-1], dtype)
    dg[inner], dx[inner] = np.abs(div(g)[..., 0]).ravel(), np.abs(div(x)[..., 0]).ravel()
    for v in (a1, a2, m, x1, x2, aj, dg, dx):
        assert v.dtype == dtype
    flat = lambda v: v.reshape(B, -1)                                # noqa: E731
    cnt, dcnt = flat(cnt), flat(cnt & inner)
    zero = dtype(0)
    out = {"count": cnt.sum(1).astype(np.int32), "div_count": dcnt.sum(1).astype(np.int32)}
    for name, v, c in (("sum_abs", a1, cnt), ("sum_sq", a2, cnt), ("sum_abs_x", x1, cnt), ("sum_sq_x", x2, cnt), ("sum_abs_jac", aj, cnt),
                       ("sum_abs_div_g", dg, dcnt), ("sum_abs_div_x", dx, dcnt)):
        out[name] = ordered_sum(np.where(c, flat(v), zero), dtype)
    # Non-finite values (the header is silent; this is C's fmaxf and the kernel's `mm > m` from m = -1, idx = -1, stated here and not
    # read off a result): a NaN component is dropped by fmax, so m is a NaN only where every component of d is one; such a cell never
    # wins the comparison, it neither moves max_abs nor becomes the arg-max (an entry whose counted cells ALL have m = NaN keeps
    # -1 / -1); the maxima of |div| drop a NaN in the same way.  The sums take every counted cell and become non-finite.
    with np.errstate(invalid="ignore"):
        mm = np.where(cnt & ~np.isnan(flat(m)), flat(m), dtype(-1))
    out["argmax"] = np.where((mm >= 0).any(1), mm.argmax(1), -1).astype(np.int32)      # np.argmax: the first, i.e. lowest, of equals
    out["max_abs"] = np.where(out["count"] > 0, mm.max(1), zero).astype(dtype)
    out["max_abs_div_g"] = np.fmax.reduce(np.where(dcnt, flat(dg), zero), axis=1).astype(dtype)
    out["max_abs_div_x"] = np.fmax.reduce(np.where(dcnt, flat(dx), zero), axis=1).astype(dtype)
    return out


def derived(r, D):
    """the derived means of ``ops.FieldMetrics`` from a result of ``metrics``, in fp64 (nan where the header says so)"""
    f = {k: np.asarray(v, F64) for k, v in r.items()}
    with np.errstate(divide="ignore", invalid="ignore"):
        n = f["count"]
        rel = lambda a, b: np.where(b == 0, np.nan, a / np.where(b == 0, 1.0, b))      # noqa: E731
        return {"l1": f["sum_abs"] / (n * D), "rmse": np.sqrt(f["sum_sq"] / (n * D)), "rel_l1": rel(f["sum_abs"], f["sum_abs_x"]),
                "rel_l2": np.sqrt(rel(f["sum_sq"], f["sum_sq_x"])), "jacobian_l1": f["sum_abs_jac"] / (n * D * D),
                "div_l1_g": f["sum_abs_div_g"] / f["div_count"], "div_l1_x": f["sum_abs_div_x"] / f["div_count"]}


def raw_words(r):
    """the int32 rows [B, DF_FM_WORDS] the kernel writes for a float32 result of ``metrics``"""
    B = len(r["count"])
    raw = np.zeros((B, WORDS), np.int32)
    for name, word in WORD.items():
        v = np.asarray(r[name])
        raw[:, word] = v if name in INTS else v.astype(F32).view(np.int32)
    return raw


# ---- the shapes of the GPU test and the boundary each one crosses -----------------------------------------------------------------------
# (B, (Z,) Y, X)
SHAPES = [
    ((1, 2, 2), "2-D at the stencils' minimum extents: every cell on a far face, one divergence value"),
    ((1, 2, 2, 2), "3-D at the minimum extents"),
    ((3, 5, 7, 9), "B = 3, every extent odd: 315 cells, one ragged workgroup per entry"),
    ((1, 2, 16, 32), "exactly one full workgroup (1024 cells)"),
    ((3, 17, 130), "2-D, B = 3: 2210 cells, three workgroups per entry, the last ragged -- the second launch combines them"),
    ((1, 3, 19, 18), "3-D, 1026 cells: a second workgroup of two cells"),
    ((1, 513, 512), "257 workgroups: one thread of the second launch adds two workgroup sums"),
]


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(g, x) float32, read-only, seeded by the shape"""
    D = len(shape) - 1
    rng = np.random.RandomState(1000 + sum(shape) + len(shape))
    x = rng.uniform(-1, 1, shape + (D,)).astype(F32)
    g = (x + rng.uniform(-0.1, 0.1, shape + (D,)).astype(F32)).astype(F32)
    return _ro(g), _ro(x)


@functools.lru_cache(maxsize=None)
def case_mask(shape, kind):
    """the masks of the GPU test: ``shared`` [(Z,)Y,X], ``per_entry`` [B,..], ``one_empty`` (per entry, all zero for entry 0),
    ``single`` (shared, one cell)"""
    rng = np.random.RandomState(7 + sum(shape))
    if kind == "shared":
        return _ro((rng.uniform(size=shape[1:]) < 0.6).astype(np.uint8))
    if kind == "per_entry":
        return _ro((rng.uniform(size=shape) < 0.6).astype(np.uint8) * np.uint8(3))      # any non-zero byte counts
    if kind == "one_empty":
        m = (rng.uniform(size=shape) < 0.6).astype(np.uint8)
        m[0] = 0
        return _ro(m)
    assert kind == "single"
    m = np.zeros(shape[1:], np.uint8)
    m[tuple(n // 2 for n in shape[1:])] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def reference(shape, kind=None):
    """(fp32 twin, fp64 truth) on the shared inputs, computed once per case"""
    g, x = inputs(shape)
    mask = None if kind is None else case_mask(shape, kind)
    return metrics(g, x, mask, F32), metrics(g, x, mask, F64)
