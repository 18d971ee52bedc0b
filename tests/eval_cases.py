"""The table of tests/test_gpu_eval_edges.py and tests/test_eval_cases_host.py: one row per call of an entry point of csrc/nn.hip,
csrc/metrics.hip and csrc/ssim.hip (include/deepfluids_hip_nn.h, _metrics.h, _ssim.h), the seeded read-only inputs of a row, and its
result by the NumPy restatements (nn_ref.Ops32 / Ops64, field_metrics_ref, ssim_ref) in fp64 or in their fp32 twin.  Plain data and
NumPy; no torch import.

A row: name, op (a key of ENTRY), its extents and scalar arguments by the header's names, off (payload offset of every fp32 / int32
operand in elements: 0 = 16-byte aligned, 1 = 4-byte aligned and not 8, 2 = 8-byte aligned and not 16; a mask's byte offset is
2 * off + 1 when off > 0; operands the header wants 8-byte aligned stay at 0 unless the row sets ws_off), twin (the row whose seeded inputs
it shares: a loose row's aligned twin, a hostile row's clean base), hostile (what is planted), and reach: the branch of the kernel the
row exists for, as data -- ``facts(r)`` recomputes every such entry from the extents and the host test compares the two.

What a comparison is held to is ``RULE[op]``: "bits" (the header fixes the order and the twin repeats it: bit for bit, a NaN must be a
NaN) or "tolerance" (everything after an ELU: nn_ref.tolerance against fp64).  ``GUARD[op]`` is not a tolerance of any kernel: it is the
count of fp32 roundings on the op's longest chain, and the host test holds the TWIN to that many eps of the fp64 restatement's largest
magnitude, so that a twin that restates something else does not go unnoticed."""
import functools
import zlib

import numpy as np

import field_metrics_ref as fref
import nn_ref as R
import ssim_ref as sref

F32, F64 = np.float32, np.float64
O32, O64 = R.Ops32(), R.Ops64()
OPS_OF = {F32: O32, F64: O64}

ENTRY = {"bn_fwd": "df_nn_bn_elu_dropout_fwd", "bn_bwd": "df_nn_bn_elu_dropout_bwd", "bn_infer": "df_nn_bn_elu_infer",
         "adv_fwd": "df_nn_window_advance_fwd", "adv_bwd": "df_nn_window_advance_bwd", "rows_copy": "df_nn_rows_copy",
         "mse_fwd": "df_nn_mse_fwd", "mse_bwd": "df_nn_mse_bwd", "rollout": "df_nn_rollout", "metrics": "df_field_metrics%(d)dd",
         "ssim": "df_ssim", "group_mean": "df_ssim_group_mean"}
# the size queries a row's harness asks before the call
QUERY = {"mse_fwd": "df_nn_mse_workspace_bytes", "metrics": "df_field_metrics_workspace_bytes", "ssim": "df_ssim_workspace_bytes"}
RULE = {"bn_fwd": "bits", "bn_bwd": "bits", "bn_infer": "tolerance", "adv_fwd": "bits", "adv_bwd": "bits", "rows_copy": "bits",
        "mse_fwd": "bits", "mse_bwd": "bits", "rollout": "tolerance", "metrics": "bits", "ssim": "bits", "group_mean": "bits"}
TOLERANCE_OUTPUTS = {"bn_fwd": ("act", "out")}          # of a "bits" op: what lies behind the ELU
# fp32 roundings on the longest chain (see the module docstring).  bn: a row thread's <= 3 additions, two column sums, d, d*d, rstd,
# xh, y, the series (2 ulp), inv -- 16 -- times the largest |gamma * rstd| of the rows, 1.5 / sqrt(0.5) < 4 (the constant column and B = 1
# have xh == 0 exactly); its backward two more sums and the combination, the same factor twice.  mse: d, d*d, three additions, the final
# rounding.  metrics: a thread's <= 4 cells of <= 9 terms of <= 4 roundings each, relative to a sum of non-negative terms.
GUARD = {"bn_fwd": 64, "bn_bwd": 256, "bn_infer": 64, "adv_fwd": 2, "adv_bwd": 1, "rows_copy": 0, "mse_fwd": 8, "mse_bwd": 3, "metrics": 144,
         "group_mean": 0}
# ssim: not in eps.  The twin's absolute deviation of a map value: the cancellation E[p^2] - mu^2 against v2 of a few 1e-3; 4 x 4.3e-5
# is the guard tests/test_ssim_host.py already holds the twin to at C <= 3.  The planes are sums over C channels scaled by 1 / C^2, so
# the cancelling terms do not grow with C.
SSIM_GUARD = 4 * 4.3e-5

EPS, DECAY, KEEP = R.EPS, R.DECAY, 0.5
SEED, STEP, WINDOW = 7, 3, 2
RATIO = F32(0.37)
CODE_STD, OUT_STD = F32(1.7), F32(0.4)
K_COLS, K_ROW_T, K_THREADS, K_ROLL, K_MSE_BLOCK, K_INFER_ROWS = 32, 32, 256, 1024, 1024, 1024
LDS_LIMIT = 15360                   # 2 Z + P + 2 N1 + 2 N2 at most (4 (Z + P + 2 N1 + 2 N2 + Z + 1024) <= 65536)

ROWS = []


def _add(name, op, reach, **kw):
    r = dict(name=name, op=op, off=0, twin=None, hostile=None, reach=reach)
    r.update(kw)
    ROWS.append(r)
    return r


def _ceil(a, b):
    return -(-a // b)


# ---- nn: the block between the linear layers ---------------------------------------------------------------------------------------------
BN_PAIRS = [(31, 1), (31, 64), (32, 31), (32, 32), (32, 1024), (33, 1), (33, 33), (33, 1024), (64, 31), (64, 64), (64, 1056), (65, 32),
            (65, 33), (65, 1056)]
BN_B, BN_N = (31, 32, 33, 64, 65), (1, 31, 32, 33, 64, 1024, 1056)


def bn_reach(B, N):
    """column blocks, whether the last one is whole, the trips of a row thread's loop (the longest and the shortest of the 32)"""
    return dict(col_blocks=_ceil(N, K_COLS), whole_blocks=N % K_COLS == 0, row_trips=(_ceil(B, K_ROW_T), B // K_ROW_T))


def _bn(name, B, N, ops=("bn_fwd", "bn_bwd"), **kw):
    for op in ops:
        _add("%s-%s" % (op, name), op, bn_reach(B, N), B=B, N=N, keep=kw.get("keep", KEEP),
             decay=kw.get("decay", DECAY), const_col=kw.get("const_col"), hostile=kw.get("hostile"),
             twin=None if kw.get("twin") is None else "%s-%s" % (op, kw["twin"]))


for _B, _N in BN_PAIRS:
    _bn("B%d-N%d" % (_B, _N), _B, _N)
_bn("keep1", 33, 33, keep=1.0)                                       # every element kept, inv == 1
_bn("decay0", 5, 40, ops=("bn_fwd",), decay=0.0)
_bn("decay1", 5, 40, ops=("bn_fwd",), decay=1.0)
_bn("B1", 1, 33)                                                      # the Bessel factor is 1, var is 0
_bn("const-col", 33, 40, const_col=7)                                 # var == 0, rstd == 1 / sqrt(eps)
_bn("clean", 33, 40, ops=("bn_fwd",))                                 # the base of the two poisoned rows
_bn("nan", 33, 40, ops=("bn_fwd",), hostile=("nan", 5, 7), twin="clean")
_bn("inf", 33, 40, ops=("bn_fwd",), hostile=("inf", 5, 7), twin="clean")


def infer_reach(B, N):
    """column blocks of 256, rows of the grid (capped at 1024), the trips of the row loop (the longest)"""
    return dict(col_blocks=_ceil(N, K_THREADS), grid_rows=min(B, K_INFER_ROWS), row_trips=_ceil(B, K_INFER_ROWS))


def elu_sweep():
    """the pre-activations of the sweep row, fp32: the edges of the header's series"""
    tiny = np.nextafter(F32(0), F32(1))
    v = [F32(0.0), F32(-0.0), tiny, -tiny, F32(1e-8), F32(-1e-8), np.nextafter(F32(-17.5), F32(0)), F32(-17.5),
         np.nextafter(F32(-17.5), F32(-100)), F32(-87), F32(-104), F32(-1e30)]
    c = F32(1.44269502)
    for n in range(1, 26):                                                # the two neighbouring fp32 values between which rintf(y * c) goes from -n to -(n + 1)
        a = F32(-(n + 0.5) / F64(c))
        while np.rint(a * c) != -n:
            a = np.nextafter(a, F32(0))
        while np.rint(np.nextafter(a, F32(-100)) * c) == -n:
            a = np.nextafter(a, F32(-100))
        v += [a, np.nextafter(a, F32(-100))]
    return np.array(v, F32)


_add("bn_infer-B1025-N257", "bn_infer", infer_reach(1025, 257), B=1025, N=257, sweep=False)
_add("bn_infer-B2049-N1", "bn_infer", infer_reach(2049, 1), B=2049, N=1, sweep=False)
_add("bn_infer-elu-sweep", "bn_infer", infer_reach(2, len(elu_sweep())), B=2, N=len(elu_sweep()), sweep=True)

# ---- nn: window step, rows copy, MSE ---------------------------------------------------------------------------------------------------------
def flat_reach(total):
    """workgroups of an element-per-thread launch and the live threads of the last one"""
    return dict(blocks=_ceil(total, K_THREADS), last=total - (_ceil(total, K_THREADS) - 1) * K_THREADS)


#       name           B   W  Z    P   i
ADV = [("n255",        51, 3, 3,   2,  0),
       ("n256-P1",     64, 3, 3,   1,  1),
       ("n257",        1,  3, 200, 57, 0),
       ("P-eq-Z",      3,  3, 4,   4,  0),
       ("last-i",      5,  4, 3,   2,  2),        # i = W - 2
       ("W2",          5,  2, 3,   2,  0)]
for _n, _B, _W, _Z, _P, _i in ADV:
    _add("adv_fwd-" + _n, "adv_fwd", flat_reach(_B * (_Z + _P)), B=_B, W=_W, Z=_Z, P=_P, i=_i)
    _add("adv_bwd-" + _n, "adv_bwd", flat_reach(_B * (_Z + _P)), B=_B, Z=_Z, P=_P, null=())
for _null in (("gx",), ("gy",), ("gx", "gy")):
    _add("adv_bwd-no-" + "-".join(_null), "adv_bwd", dict(flat_reach(51 * 5), launches=len(_null) < 2), B=51, Z=3, P=2, null=_null)
for _B, _Z in ((51, 5), (257, 1)):                                    # B * Z = 255 and 257
    for _ss in (0, 1, 7):
        for _ds in (0, 1, 7):
            _add("rows_copy-n%d-s%d-d%d" % (_B * _Z, _ss, _ds), "rows_copy", dict(flat_reach(_B * _Z), gap=_ds), B=_B, Z=_Z, ss=_Z + _ss,
                 ds=_Z + _ds)


def mse_reach(n):
    """workgroups of the first launch (one fp64 partial each), and the live elements of the last one"""
    return dict(blocks=_ceil(n, K_MSE_BLOCK), last=n - (_ceil(n, K_MSE_BLOCK) - 1) * K_MSE_BLOCK, final_trips=_ceil(_ceil(n, K_MSE_BLOCK), K_THREADS))


MSE_N = (1, 255, 256, 1023, 1024, 1026, 256 * 1024 + 1)
for _n in MSE_N:
    _add("mse_fwd-n%d" % _n, "mse_fwd", mse_reach(_n), n=_n, same=False, ws_off=0)
    _add("mse_bwd-n%d" % _n, "mse_bwd", flat_reach(_n), n=_n, same=False)
_add("mse_fwd-ws-off2", "mse_fwd", mse_reach(1026), n=1026, same=False, ws_off=2, twin="mse_fwd-n1026")      # 8-byte aligned, not 16
_add("mse_fwd-same", "mse_fwd", mse_reach(1026), n=1026, same=True, ws_off=0)                               # a == b: exactly +0.0
_add("mse_bwd-same", "mse_bwd", flat_reach(1026), n=1026, same=True)


# ---- nn: the rollout --------------------------------------------------------------------------------------------------------------------------
def rollout_reach(Z, P, N1, N2):
    """per layer the chunks of its matrix-vector product as (nb, sk, idle threads); the trips of the advance loop over the code"""
    return dict(layers=tuple(tuple(c[1:] for c in R.matvec_chunks(K, N)) for K, N in ((Z + P, N1), (N1, N2), (N2, Z))),
                code_trips=_ceil(Z, K_ROLL), lds=2 * Z + P + 2 * N1 + 2 * N2)


#           name              S  F  Z     P  N1    N2   scale
ROLLOUT = [("own-widths",     2, 3, 16,   2, 1024, 512, 0.5),        # sk = 1 with every thread live; sk = 2
           ("second-chunk",   2, 3, 3,    2, 1025, 8,   0.5),        # chunk 2 has nb = 1, sk = 1024 > K
           ("ragged-tail",    2, 3, 3,    2, 1500, 600, 0.5),        # nb = 476 (sk = 2, 72 idle threads); nb = 600 (sk = 1)
           ("long-code",      2, 3, 1030, 3, 40,   33,  0.5),        # Z > 1024 in the advance loop and two chunks in layer 3
           ("all-parameters", 2, 3, 4,    4, 16,   8,   0.5),        # P == Z: every code entry comes from the data
           ("one-step",       1, 2, 3,    1, 16,   8,   0.5),        # F = 2, S = 1
           ("scenes",         3, 3, 3,    2, 80,   40,  0.5)]        # each scene alone is bit-equal to the same scene in the batch
for _n, _S, _F, _Z, _P, _N1, _N2, _sc in ROLLOUT:
    _add("rollout-" + _n, "rollout", rollout_reach(_Z, _P, _N1, _N2), S=_S, F=_F, Z=_Z, P=_P, N1=_N1, N2=_N2, scale=_sc)

# ---- metrics -----------------------------------------------------------------------------------------------------------------------------------
# (B, (Z,) Y, X): the shapes of field_metrics_ref.SHAPES that are cheap, and the block counts of the xcd_block remap the particle table found
# worth having: 7 and 17 workgroups (remainder 7 and 1 of the 8 XCDs, quotient 0 and 2)
METRIC_SHAPES = [(1, 2, 2), (1, 2, 2, 2), (3, 5, 7, 9), (3, 17, 130), (1, 3, 19, 18), (7, 5, 7), (1, 5, 59, 59)]
# mask: the header says "A cell is COUNTED when the mask is NULL or its byte is non-zero": the bytes 2 and 255 count
MASK_BYTES = (0, 2, 255)


def metrics_reach(shape):
    ncell = int(np.prod(shape[1:]))
    nblk = _ceil(ncell, fref.K_CELLS_PER_BLOCK)
    return dict(nblk=nblk, nblk_total=shape[0] * nblk, xcd=(shape[0] * nblk % 8, shape[0] * nblk // 8), record_bytes=4 * (len(shape) - 1))


def _metrics(name, shape, **kw):
    kw = dict(dict(mask=None, hostile=None, twin=None), **kw)
    base = _add("metrics-" + name, "metrics", metrics_reach(shape), shape=shape, **kw)
    _add("metrics-" + name + "-loose", "metrics", metrics_reach(shape), shape=shape, off=1, mask=kw["mask"], hostile=kw["hostile"],
         twin=kw["twin"] or base["name"], aligned=base["name"])


for _shape in METRIC_SHAPES:
    _metrics("x".join(map(str, _shape)), _shape)
for _shape in ((3, 5, 7, 9), (7, 5, 7)):
    for _kind in ("bytes", "shared-bytes"):
        _metrics("x".join(map(str, _shape)) + "-" + _kind, _shape, mask=_kind)
for _shape in ((3, 5, 7, 9), (3, 17, 130)):
    _tag = "x".join(map(str, _shape))
    _metrics(_tag + "-holed", _shape, mask="holed")                                     # the base of the masked NaN: the NaN's cell and its readers are not counted
    _metrics(_tag + "-nan", _shape, hostile=("nan", False), twin="metrics-" + _tag)
    _metrics(_tag + "-inf", _shape, hostile=("inf", False), twin="metrics-" + _tag)
    # every component of the cell a NaN: fmaxf has nothing finite to keep, m is a NaN and `mm > m` is what keeps it out of max_abs / argmax
    _metrics(_tag + "-nan-all", _shape, hostile=("nan-all", False), twin="metrics-" + _tag)
    _metrics(_tag + "-nan-masked", _shape, mask="holed", hostile=("nan", True), twin="metrics-" + _tag + "-holed")

# ---- ssim ---------------------------------------------------------------------------------------------------------------------------------------
def ssim_reach(H, W, C, filter_size=11):
    S = min(filter_size, H, W)
    OH, OW = H - S + 1, W - S + 1
    return dict(S=S, OH=OH, OW=OW, tiles=(_ceil(OH, sref.TILE), _ceil(OW, sref.TILE)), last_tile=(OH - (_ceil(OH, sref.TILE) - 1) * sref.TILE,
                OW - (_ceil(OW, sref.TILE) - 1) * sref.TILE), pooled=((H + 1) // 2, (W + 1) // 2), odd=(H % 2, W % 2), record_bytes=4 * C,
                final_trips=_ceil(_ceil(OH, sref.TILE) * _ceil(OW, sref.TILE), K_THREADS))


def _ssim(name, shape, C, N=2, **kw):
    kw = dict(dict(filter_size=11, maps=True, pools=True, off=0, twin=None, hostile=None), **kw)
    return _add("ssim-" + name, "ssim", ssim_reach(shape[0], shape[1], C, kw["filter_size"]), shape=shape, C=C, N=N, **kw)


for _shape, _ in sref.SSIM_SHAPES:                                        # C = 4: the default: arm of the switch
    _ssim("%dx%d-c4" % _shape, _shape, 4)
for _C in (1, 2, 3):                                                      # every record width at a 4-byte aligned address
    _ssim("33x45-c%d" % _C, (33, 45), _C, N=3)
    _ssim("33x45-c%d-loose" % _C, (33, 45), _C, N=3, off=1, twin="ssim-33x45-c%d" % _C)
_ssim("33x45-c4-loose", (33, 45), 4, off=1, twin="ssim-33x45-c4")            # (its aligned twin is among the C = 4 rows above)
_ssim("33x45-c4-loose2", (33, 45), 4, off=2, twin="ssim-33x45-c4")          # a 16-byte record at an 8-byte aligned address
for _shape in ((1, 40), (40, 1), (2, 2), (43, 43), (42, 42), (44, 75)):
    _ssim("%dx%d-c3" % _shape, _shape, 3)
for _fs in (2, 3, 10):
    _ssim("33x45-c2-f%d" % _fs, (33, 45), 2, filter_size=_fs)
_ssim("554x522-c1", (554, 522), 1, N=1)                                   # 17 x 16 = 272 tiles: a thread of the final kernel adds two
_ssim("33x45-c3-no-maps", (33, 45), 3, N=3, maps=False, twin="ssim-33x45-c3")
_ssim("33x45-c3-no-pools", (33, 45), 3, N=3, pools=False, twin="ssim-33x45-c3")
_ssim("44x75-c3-nan", (44, 75), 3, hostile=("nan", 1, 20, 37, 1), twin="ssim-44x75-c3")      # image 1, pixel (20, 37), channel 1
for _G, _M in ((1, 1), (3, 5), (1, 257), (2, 300)):
    _add("group_mean-G%d-M%d" % (_G, _M), "group_mean", dict(trips=_ceil(_M, K_THREADS), last=_M - (_ceil(_M, K_THREADS) - 1) * K_THREADS),
         G=_G, M=_M)


def group_mean_ssim_row(r):
    """the df_ssim call whose rows a group_mean row reads: G * M images of 11 x 11, one channel, one output pixel each, no optional output"""
    return dict(name=r["name"] + "/ssim", op="ssim", off=0, twin=None, hostile=None, reach=ssim_reach(11, 11, 1), shape=(11, 11), C=1,
                N=r["G"] * r["M"], filter_size=11, maps=False, pools=False)


BY_NAME = {r["name"]: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
for _r in ROWS:
    assert _r["twin"] is None or _r["twin"] in BY_NAME, _r


def rows(op=None, **match):
    return [r for r in ROWS if (op is None or r["op"] == op) and all(r.get(k) == v for k, v in match.items())]


def names(op=None, **match):
    return [r["name"] for r in rows(op, **match)]


def entry_point(r):
    return ENTRY[r["op"]] % dict(d=len(r["shape"]) - 1) if r["op"] == "metrics" else ENTRY[r["op"]]


def facts(r):
    """``r["reach"]`` recomputed from the extents alone"""
    op = r["op"]
    if op in ("bn_fwd", "bn_bwd"):
        return bn_reach(r["B"], r["N"])
    if op == "bn_infer":
        return infer_reach(r["B"], r["N"])
    if op in ("adv_fwd", "adv_bwd"):
        f = flat_reach(r["B"] * (r["Z"] + r["P"]))
        return dict(f, launches=len(r["null"]) < 2) if op == "adv_bwd" and r["null"] else f
    if op == "rows_copy":
        return dict(flat_reach(r["B"] * r["Z"]), gap=r["ds"] - r["Z"])
    if op == "mse_fwd":
        return mse_reach(r["n"])
    if op == "mse_bwd":
        return flat_reach(r["n"])
    if op == "rollout":
        return rollout_reach(r["Z"], r["P"], r["N1"], r["N2"])
    if op == "metrics":
        return metrics_reach(r["shape"])
    if op == "ssim":
        return ssim_reach(r["shape"][0], r["shape"][1], r["C"], r["filter_size"])
    return dict(trips=_ceil(r["M"], K_THREADS), last=r["M"] - (_ceil(r["M"], K_THREADS) - 1) * K_THREADS)


def offsets(r):
    """payload offset per kind of operand: ``f`` fp32 / int32 operands the header wants 4-byte aligned (elements), ``m`` the mask (bytes),
    ``d`` operands it wants 8-byte aligned (in floats: 0 or 2)"""
    return dict(f=r["off"], m=2 * r["off"] + 1 if r["off"] else 0, d=r.get("ws_off", 0))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def _rng(r, salt=0):
    # a loose row and a hostile row draw what their twin draws
    return np.random.RandomState((zlib.crc32((r["twin"] or r["name"]).encode()) + salt) % (2 ** 31))


def _f32(a):
    return np.asarray(a, F64).astype(F32)


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


_POISON = {"nan": np.nan, "nan-all": np.nan, "inf": np.inf}


def nan_cell(shape):
    """the cell of the hostile metrics rows: inner on every axis, at least two away from the far faces (so none of its readers reads
    backwards) -> (entry, flat cell, component)"""
    ext = shape[1:]
    co = tuple(max(n // 2 - 1, 0) for n in ext)
    assert all(c + 2 <= n - 1 for c, n in zip(co, ext)) and all(c >= 1 for c in co), shape
    return 1, int(np.ravel_multi_index(co, ext)), 0


def readers(shape, cell):
    """the cells of an entry whose terms read ``cell``: itself and, per axis, the one in front of it (a cell on a far face reads
    backwards: nan_cell keeps away from those)"""
    ext = shape[1:]
    co = np.unravel_index(cell, ext)
    out = [cell]
    for a in range(len(ext)):
        assert 1 <= co[a] and co[a] + 1 < ext[a] - 1
        c = list(co)
        c[a] -= 1
        out.append(int(np.ravel_multi_index(c, ext)))
    return out


def _mask_of(r):
    shape, kind = r["shape"], r["mask"]
    if kind is None:
        return None
    rng = np.random.RandomState(11 + sum(shape))
    if kind in ("bytes", "shared-bytes"):
        return rng.choice(np.array(MASK_BYTES, np.uint8), size=shape if kind == "bytes" else shape[1:], p=(0.4, 0.3, 0.3)).astype(np.uint8)
    assert kind == "holed"
    m = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=shape, p=(0.3, 0.3, 0.2, 0.2)).astype(np.uint8)
    e, cell, _ = nan_cell(shape)
    m.reshape(shape[0], -1)[e, readers(shape, cell)] = 0
    return m


def _bn_inputs(r):
    rng = _rng(r)
    B, N = r["B"], r["N"]
    x = _f32(rng.normal(0.3, 1.5, (B, N)))
    x[0, 0] = 0.0
    i = dict(x=x, gamma=_f32(rng.uniform(0.5, 1.5, N)), beta=_f32(rng.uniform(-0.5, 0.5, N)), moving_mean=_f32(rng.uniform(-0.2, 0.2, N)),
             moving_var=_f32(rng.uniform(0.5, 1.5, N)), gout=_f32(rng.normal(0, 1, (B, N))))
    if r["const_col"] is not None:
        x[:, r["const_col"]] = 0.75
    if r["hostile"]:
        kind, row, col = r["hostile"]
        x[row, col] = _POISON[kind]
    i["kept"] = R.mask(R.mask_key(SEED, STEP, WINDOW, 1), B, N, r["keep"])
    if r["op"] == "bn_bwd":                                                # on the twin's own activations and statistics, as test_gpu_nn.py
        _, act, mean, rstd, _, _ = O32.bn_fwd(x, i["gamma"], i["beta"], i["moving_mean"], i["moving_var"], i["kept"], r["keep"])
        act = act.copy()
        if B > 2:
            act[1, 0] = 0.0                                                # an exact zero takes gd
        i.update(act=act, mean=mean, rstd=rstd)
    return i


def _build(r):
    op = r["op"]
    rng = _rng(r, 1)
    if op in ("bn_fwd", "bn_bwd"):
        return _bn_inputs(r)
    if op == "bn_infer":
        B, N = r["B"], r["N"]
        i = dict(gamma=_f32(rng.uniform(0.5, 1.5, N)), beta=_f32(rng.uniform(-0.5, 0.5, N)), moving_mean=_f32(rng.uniform(-0.2, 0.2, N)),
                 moving_var=_f32(rng.uniform(0.5, 1.5, N)), x=_f32(rng.normal(0.3, 1.5, (B, N))))
        if r["sweep"]:
            # x == moving_mean: xh is exactly +0; gamma = -1 makes xh * gamma exactly -0, and -0 + beta is beta, bit for bit, -0 included
            i.update(x=np.broadcast_to(i["moving_mean"], (B, N)).copy(), gamma=np.full(N, -1, F32), beta=elu_sweep())
        return i
    if op == "adv_fwd":
        B, W, K0 = r["B"], r["W"], r["Z"] + r["P"]
        return dict(x=_f32(rng.normal(0, 1, (B, K0))), y=_f32(rng.normal(0, 1, (B, r["Z"]))), xw=_f32(rng.normal(0, 1, (B, W, K0))))
    if op == "adv_bwd":
        return dict(gx_next=_f32(rng.normal(0, 1, (r["B"], r["Z"] + r["P"]))))
    if op == "rows_copy":
        return dict(src=_f32(rng.normal(0, 1, ((r["B"] - 1) * r["ss"] + r["Z"],))))
    if op in ("mse_fwd", "mse_bwd"):
        a = _f32(rng.normal(0, 1, r["n"]))
        return dict(a=a, b=a.copy() if r["same"] else _f32(rng.normal(0, 1, r["n"])), gout=np.array([0.75], F32))
    if op == "rollout":
        S, F, Z, P = r["S"], r["F"], r["Z"], r["P"]
        p = R.init_params(rng, Z + P, r["N1"], Z, scale=r["scale"], n2=r["N2"])
        i = dict(x_test=_f32(rng.normal(0, 1, (S * (F - 1), Z + P))), y_test=_f32(rng.normal(0, 1, (S * (F - 1), Z))))
        i.update({k: v.astype(F32) for k, v in p.items()})
        return i
    if op == "metrics":
        g, x = fref.inputs(r["shape"])
        i = dict(g=g, x=x, mask=_mask_of(r))
        if r["hostile"]:
            e, cell, k = nan_cell(r["shape"])
            g = g.copy()
            g.reshape(r["shape"][0], -1, g.shape[-1])[e, cell, slice(None) if r["hostile"][0] == "nan-all" else k] = _POISON[r["hostile"][0]]
            i["g"] = g
        return i
    if op == "ssim":
        x, g = sref.inputs(r["shape"], r["C"], 0.05, r["N"])
        if r["hostile"]:
            kind, n, y, xx, c = r["hostile"]
            g = g.copy()
            g[n, y, xx, c] = _POISON[kind]
        return dict(a=g, b=x)
    if op == "group_mean":
        x, g = sref.inputs((11, 11), 1, 0.05, r["G"] * r["M"])
        return dict(a=g, b=x)
    raise KeyError(op)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return _ro(_build(BY_NAME[name]))


def inputs(r):
    """the operands of a row by name (read-only NumPy arrays; None = passed as NULL); seeded, computed once"""
    return _inputs(r["name"])


# ---- the restatements -----------------------------------------------------------------------------------------------------------------------
def _params(i, dt):
    return {k: i[k].astype(dt) for k in R.NAMES}


def _restate(r, dt):
    op, i = r["op"], inputs(r)
    ops = OPS_OF[dt]
    c = lambda *ks: [i[k].astype(dt) for k in ks]      # noqa: E731
    if op == "bn_fwd":
        with np.errstate(invalid="ignore", over="ignore"):
            out, act, mean, rstd, mm, mv = ops.bn_fwd(*c("x", "gamma", "beta", "moving_mean", "moving_var"), i["kept"], r["keep"], r["decay"])
        return dict(out=out, act=act, mean=mean, rstd=rstd, moving_mean=mm, moving_var=mv)
    if op == "bn_bwd":
        gx, gg, gb = ops.bn_bwd(*c("x", "act", "gout", "gamma", "mean", "rstd"), i["kept"], r["keep"])
        return dict(gx=gx, ggamma=gg, gbeta=gb)
    if op == "bn_infer":
        return dict(out=ops.bn_infer(*c("x", "gamma", "beta", "moving_mean", "moving_var")))
    if op == "adv_fwd":
        return dict(x_next=ops.advance(*c("x", "y", "xw"), r["i"], RATIO, r["Z"]))
    if op == "adv_bwd":
        g, = c("gx_next")
        gx = g.copy()
        gx[:, r["Z"]:] = 0
        out = dict(gx=gx, gy=g[:, :r["Z"]] * dt(RATIO))
        return {k: v for k, v in out.items() if k not in r["null"]}
    if op == "rows_copy":
        B, Z, ss, ds = r["B"], r["Z"], r["ss"], r["ds"]
        dst = np.full((B - 1) * ds + Z, np.nan, dt)                      # NaN: the element keeps what it held
        for b in range(B):
            dst[b * ds:b * ds + Z] = i["src"][b * ss:b * ss + Z]
        return dict(dst=dst)
    if op == "mse_fwd":
        return dict(out=np.array([ops.mse(*c("a", "b"))], dt))
    if op == "mse_bwd":
        return dict(ga=ops.mse_bwd(*c("a", "b"), gout=i["gout"][0]))
    if op == "rollout":
        return dict(z_out=R.rollout(ops, _params(i, dt), i["x_test"], i["y_test"], r["S"], r["F"], r["Z"], CODE_STD, OUT_STD))
    if op == "metrics":
        with np.errstate(invalid="ignore", over="ignore"):
            return fref.metrics(i["g"], i["x"], i["mask"], dt)
    if op == "ssim":
        with np.errstate(invalid="ignore"):
            out = sref.ssim(i["a"], i["b"], dt, filter_size=r["filter_size"])
            out.update(pool_a=sref.pool(i["a"], dt), pool_b=sref.pool(i["b"], dt))
        return out
    if op == "group_mean":
        s = sref.ssim(i["a"], i["b"], dt)
        return dict(rows=sref.raw_words(s), mean=np.stack([sref.group_mean(s["sum"], s["count"], r["G"]), sref.group_mean(s["sum_cs"], s["count"], r["G"])], axis=1))
    raise KeyError(op)


@functools.lru_cache(maxsize=None)
def _expected(name, dtname):
    return _ro(_restate(BY_NAME[name], np.dtype(dtname).type))


def expected(r, dtype):
    """{output: array}: the row's result in ``dtype`` arithmetic by the restatement; computed once, read-only"""
    return _expected(r["name"], np.dtype(dtype).name)


def ssim_sigma(r):
    S = min(r["filter_size"], *r["shape"])
    return S, sref.DEFAULTS["filter_sigma"] * S / r["filter_size"]


def nonfinite(r):
    """where a hostile row's result is not finite, by reasoning on the definition alone -> {output: bool array}; every other element
    is finite (and, the GPU test adds, bit-equal to the clean twin's)"""
    op, h = r["op"], r["hostile"]
    if op == "bn_fwd":
        # NaN: the column's sums, so its mean, var, rstd, every activation and both moving averages.  +inf: mean = inf, d = x - inf is
        # -inf or (at the element itself) NaN, var and all that follows NaN.  A dropped element of `out` is 0 whatever act is.
        _, _, col = h
        B, N = r["B"], r["N"]
        colv = np.arange(N) == col
        full = np.broadcast_to(colv, (B, N))
        return dict(act=full, out=full & inputs(r)["kept"], mean=colv, rstd=colv, moving_mean=colv, moving_var=colv)
    if op == "metrics":
        # (entry 1) counted: every sum over terms of g at the cell or at a reader of it: a1, a2, aj, |div g|; never a term of x alone, a
        # count, or (the NaN) a maximum, which `mm > m` and fmaxf keep it out of; +inf wins them.  Not counted (masked, its readers too):
        # nothing.
        kind, masked = h
        B = r["shape"][0]
        e = np.arange(B) == nan_cell(r["shape"])[0]
        none = np.zeros(B, bool)
        hit = none if masked else e
        out = {k: none for k in fref.INTS + fref.SUMS + fref.MAXES}
        out.update(sum_abs=hit, sum_sq=hit, sum_abs_jac=hit, sum_abs_div_g=hit)
        if kind == "inf":
            out.update(max_abs=hit, max_abs_div_g=hit, argmax=hit)         # (an integer word: it differs from the clean run's, it is the cell)
        return out
    if op == "ssim":
        # every tap is non-zero: an output is NaN iff its S x S window covers the pixel; the pooled quad that owns it; the image's rows
        _, n, y, x, c = h
        N, (H, W), C = r["N"], r["shape"], r["C"]
        S, OH, OW = r["reach"]["S"], r["reach"]["OH"], r["reach"]["OW"]
        m = np.zeros((N, OH, OW), bool)
        m[n, max(y - S + 1, 0):min(y, OH - 1) + 1, max(x - S + 1, 0):min(x, OW - 1) + 1] = True
        pa = np.zeros((N, (H + 1) // 2, (W + 1) // 2, C), bool)
        pa[n, y // 2, x // 2, c] = True
        img = np.arange(N) == n
        return dict(ssim_map=m, cs_map=m, pool_a=pa, pool_b=np.zeros_like(pa), mean=img, mean_cs=img, sum=img, sum_cs=img)
    raise KeyError(op)
