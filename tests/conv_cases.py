"""The case table of tests/test_gpu_conv_edges.py (GPU) and tests/test_conv_cases_host.py (no GPU): one row per branch of the host code of
csrc/conv.hip, csrc/conv_small.hip and csrc/conv_bf16.hip -- conv_common, launch / launch_n, tiny2d_ok, launch_small_n / _k,
thin_k_mfma_ok / launch_thin_k_mfma, thin_n_mfma_ok / launch_thin_n_mfma, upconv_fwd_impl, df_conv_s2_dgrad, upconv_dgrad_impl,
launch_bf16x3.  Data only; imports nothing.

A row is a dict:
  id, entry   entry = "fwd" df_conv_fwd | "fwd_bf16x3" | "s2_fwd" | "s2_dgrad" | "up_fwd" | "up_fwd_bf16x3" | "up_dgrad" | "up_dgrad_bf16x3"
  shape       (B, D, H, W) as the entry point takes them: the OUTPUT grid of "s2_fwd", the gradient's (coarse) grid of "s2_dgrad", the COARSE
              grid of the "up_*" entry points; D = 1 when kz = 1
  cin, cout, kz, flags     as the entry point takes them
  mode        "fwd" only: the pack mode of wp (1: the call is a dgrad, x holds Cin = the layer's output channels)
  off         payload offset in floats per operand slot x | wp | bias | residual | mask_src | y (x: gy / g, y: gx / acc of the dgrads);
              0 = 16-byte aligned, 1 = 4-byte aligned only
  null        slots passed as NULL although the call needs them (error rows); a slot whose flag is not set is always NULL
  reaches     the kernel instantiations the call launches, in launch order (names as `nm -C` prints them, without blanks), or the
              negative DF_E* code it must return without launching anything.  OBSERVED without a GPU: tests/test_conv_cases_host.py runs
              every row through tests/wgrad_launch_recorder.cpp.  The rows state it as (family, N tile, VEC, ...) -- see _names -- and the
              tile shape follows from the one rule all launchers share: W >= 12 takes the 16-wide tile.
  form        "s2_dgrad" only: what df_conv_s2_dgrad_form answers (1 live-tap classes, 0 generic parity-class kernel)
  twin        (id of the row with the same arguments and other offsets / flags, "bits" | "tol"): "bits" where the code claims the same
              summation order (VEC = false against VEC = true on the same chunk length), "tol" for another kernel

UNREACHABLE: {instantiation: reason}; empty -- every instantiation of these families in the release library has a row."""

UNREACHABLE = {}

LRELU, RESIDUAL, MASK, BIAS, ADDUP, VALU_ONLY = 1, 2, 4, 8, 16, 32
EINVAL, ESHAPE, EALIGN = -1, -2, -3
SLOTS = ("x", "wp", "bias", "residual", "mask_src", "y")
EPI = (0, BIAS, BIAS | LRELU, RESIDUAL, MASK, BIAS | LRELU | RESIDUAL | MASK)      # the epilogues of a family that takes them all
EPI_BL = (0, BIAS, BIAS | LRELU)                                                   # ... of one that takes BIAS / LRELU only
FAMILIES = ("conv_mfma_kernel<", "conv_tiny2d_kernel(", "conv_small_n_kernel<", "conv_small_k_kernel<", "conv_thin_k_mfma_kernel<",
            "conv_thin_n_mfma_kernel<", "conv_bf16x3_kernel<", "pack_kernel(", "upconv_pack_kernel(", "pack_bf16x3_kernel(",
            "upconv_pack_bf16x3_kernel(")
# the pack kernel behind each entry point's operand (every non-error row packs with it; the packed-size test calls its query)
PACKS = {"fwd": "pack_kernel", "s2_fwd": "pack_kernel", "fwd_bf16x3": "pack_bf16x3_kernel", "s2_dgrad": "upconv_pack_kernel",
         "up_fwd": "upconv_pack_kernel", "up_dgrad": "upconv_pack_kernel", "up_fwd_bf16x3": "upconv_pack_bf16x3_kernel",
         "up_dgrad_bf16x3": "upconv_pack_bf16x3_kernel"}
WAVES = {128: "2,2,2,2", 64: "2,2,2,1", 32: "4,1,1,1"}      # WM, WN, MB, NB of an N tile


def _b(v):
    return "true" if v else "false"


def _tile(d3, W, small=False):
    """TZ, TY, TX of the MFMA / small-K kernels (128 voxels) or, small=True, of conv_small_n_kernel (256 voxels)"""
    if small:
        return ("4,4,16" if W >= 12 else "4,8,8") if d3 else ("1,16,16" if W >= 12 else "1,32,8")
    return ("2,4,16" if W >= 12 else "4,4,8") if d3 else ("1,8,16" if W >= 12 else "1,16,8")


def _names(r):
    """the row's claim (family, ...) -> instantiation names"""
    what = r["reaches"]
    if isinstance(what, int):
        return what
    d3, W, fam = r["kz"] == 3, r["shape"][3], what[0]
    t = _tile(d3, W)
    if fam == "mfma":          # (nt, vec): stride 1, 3 taps per axis
        return ["conv_mfma_kernel<%d,%s,%s,%s,1,3,16,3,false>" % (r["kz"], t, WAVES[what[1]], _b(what[2]))]
    if fam == "mfma_s2":       # (nt, vec): stride 2
        return ["conv_mfma_kernel<%d,%s,%s,%s,2,3,16,3,false>" % (r["kz"], t, WAVES[what[1]], _b(what[2]))]
    if fam == "mfma_up":       # (nt, vec, chunk): 2 taps per axis; df_upconv_dgrad launches it once per parity class
        n = (8 if d3 else 4) if r["entry"] == "up_dgrad" else 1
        return ["conv_mfma_kernel<%d,%s,%s,%s,1,2,%d,2,false>" % (2 if d3 else 1, t, WAVES[what[1]], _b(what[2]), what[3])] * n
    if fam == "s2d":           # the live-tap classes of df_conv_s2_dgrad in class order: output parity 0 -> two taps, 1 -> one
        out = []
        for c in range(8 if d3 else 4):
            nz, ny, nx = (2 - ((c >> 2) & 1) if d3 else 1), 2 - ((c >> 1) & 1), 2 - (c & 1)
            out.append("conv_mfma_kernel<%d,%s,2,2,2,2,true,1,%d,%d,%d,true>" % (nz, t, ny, 32 if nz * ny * nx >= 4 else 64, nx))
        return out
    if fam == "tiny":
        return ["conv_tiny2d_kernel"]
    if fam == "small_n":       # (vec,)
        return ["conv_small_n_kernel<%d,%s,%d,%s>" % (r["kz"], _tile(d3, W, True), r["cout"], _b(what[1]))]
    if fam == "small_k":
        return ["conv_small_k_kernel<%d,%s>" % (r["kz"], t)]
    if fam == "thin_k":        # (load passes,)
        return ["conv_thin_k_mfma_kernel<%d,%d,%d>" % (r["cin"], r["cout"], what[1])]
    if fam == "thin_n":
        return ["conv_thin_n_mfma_kernel<%d,%d>" % (r["cout"], r["cin"])]
    if fam == "bf16":          # (nt,): the N tile follows the padded N alone (no narrowing)
        up = r["entry"].startswith("up_")
        n = (8 if d3 else 4) if r["entry"] == "up_dgrad_bf16x3" else 1
        return ["conv_bf16x3_kernel<%d,%s,%s,%d>" % ((2 if d3 else 1) if up else r["kz"], t, WAVES[what[1]], 2 if up else 3)] * n
    raise ValueError(what)


ROWS = []


def row(rid, entry, shape, cin, cout, kz, flags, reaches, off=None, mode=0, null=(), twin=None, form=None):
    assert all(k in SLOTS for k in (off or {})) and all(k in SLOTS for k in null), rid
    r = dict(id=rid, entry=entry, shape=tuple(shape), cin=cin, cout=cout, kz=kz, flags=flags, mode=mode, null=tuple(null), twin=twin,
             form=form, off=dict((s, (off or {}).get(s, 0)) for s in SLOTS), reaches=reaches)
    r["names"] = _names(r)
    ROWS.append(r)
    return r


def _one_tile(d3, w16, B):
    """B images of exactly one 128-voxel tile"""
    return (B, 2, 4, 16) if d3 and w16 else (B, 4, 4, 8) if d3 else (B, 1, 8, 16) if w16 else (B, 1, 16, 8)


# ---- df_conv_fwd on conv_mfma_kernel: every N tile x VEC x tile shape x dimensionality ------------------------------------------------------
# launch_n keeps the 128 | 64 wide tile only from 129 tiles on: the tile count comes from the batch (images of exactly one tile)
n = 0
for kz in (3, 1):
    for w16 in (True, False):
        for nt, B, cout in ((128, 129, 65), (64, 129, 33), (32, 3, 5)):
            rid = "mfma_%s_w%d_n%d" % ("3d" if kz == 3 else "2d", 16 if w16 else 8, nt)
            row(rid, "fwd", _one_tile(kz == 3, w16, B), 16, cout, kz, EPI[n % 6], ("mfma", nt, True))
            row(rid + "_scalar", "fwd", _one_tile(kz == 3, w16, B), 16, cout, kz, EPI[n % 6], ("mfma", nt, False), off={"x": 1}, twin=(rid, "bits"))
            n += 1
# ragged tiles on every axis, extents of 1, tile counts 1 | 3 | 8 | 9 (129 above); Cin 20 -> Kpad 32 with a zero tail, Cout 31 -> colok off
for i, (kz, shape) in enumerate([(3, (1, 3, 5, 17)), (3, (1, 1, 3, 15)), (3, (3, 1, 1, 13)), (3, (1, 5, 4, 40)), (3, (1, 5, 5, 9)), (3, (1, 3, 3, 7)),
                                 (3, (1, 1, 1, 1)), (3, (9, 4, 4, 8)), (1, (1, 1, 9, 17)), (1, (1, 1, 7, 15)), (1, (3, 1, 1, 12)), (1, (1, 1, 17, 9)),
                                 (1, (1, 1, 15, 7)), (1, (1, 1, 1, 1)), (1, (9, 1, 16, 8)), (1, (1, 1, 24, 33))]):
    row("mfma_shape%d" % i, "fwd", shape, 20, 31, kz, EPI[i % 6], ("mfma", 32, True))
# channel counts at the padding edges: Cin 5 | 33 scalar by count, 12 | 20 scalar by offset; Cout 5 ... 129 (Npad 32 | 64 | 128 | 256)
for i, (cin, cout) in enumerate([(5, 5), (12, 31), (16, 33), (20, 65), (33, 129), (4, 31), (3, 16)]):
    rid = "mfma_c%d_%d" % (cin, cout)
    row(rid, "fwd", (2, 3, 5, 13), cin, cout, 3, EPI[i % 6], ("mfma", 32, cin % 4 == 0))
    if cin % 4 == 0:
        row(rid + "_scalar", "fwd", (2, 3, 5, 13), cin, cout, 3, EPI[i % 6], ("mfma", 32, False), off={"x": 1}, twin=(rid, "bits"))
row("mfma_2d_c16_129_wide", "fwd", (129, 1, 8, 16), 16, 129, 1, BIAS | LRELU, ("mfma", 128, True))      # two 128-wide N tiles, the second one column
for i, fl in enumerate(EPI):
    row("mfma_epi%d" % fl, "fwd", (1, 3, 5, 17), 12, 33, 3, fl, ("mfma", 32, True))
row("mfma_dgrad_3d", "fwd", (1, 3, 5, 17), 33, 20, 3, MASK, ("mfma", 32, False), mode=1)
row("mfma_dgrad_2d", "fwd", (2, 1, 9, 17), 24, 40, 1, MASK, ("mfma", 32, True), mode=1)

# ---- conv_tiny2d_kernel: 2-D, H * W <= 256, Cin % 32 == 0, Cout % 16 == 0, Cout >= 32, x 16-byte aligned --------------------------------------
row("tiny_hw1", "fwd", (1, 1, 1, 1), 32, 32, 1, BIAS, ("tiny",))
row("tiny_hw15_b5", "fwd", (5, 1, 3, 5), 32, 48, 1, BIAS | LRELU, ("tiny",))                 # 75 pixels: the last block holds 11; a wave returns early
row("tiny_hw48", "fwd", (2, 1, 6, 8), 64, 80, 1, 0, ("tiny",))                               # second workgroup: three waves return early
row("tiny_hw256", "fwd", (1, 1, 16, 16), 32, 32, 1, RESIDUAL, ("tiny",))
row("tiny_not_hw257", "fwd", (1, 1, 1, 257), 32, 32, 1, BIAS, ("mfma", 32, True))
row("tiny_not_cin48", "fwd", (1, 1, 4, 4), 48, 32, 1, BIAS, ("mfma", 32, True))
row("tiny_not_cout40", "fwd", (1, 1, 4, 4), 32, 40, 1, BIAS, ("mfma", 32, True))
row("tiny_not_cout16", "fwd", (1, 1, 4, 4), 32, 16, 1, BIAS, ("mfma", 32, True))
row("tiny_not_3d", "fwd", (1, 1, 4, 4), 32, 32, 3, BIAS, ("mfma", 32, True))
for fl in EPI:
    row("tiny_epi%d" % fl, "fwd", (3, 1, 5, 7), 32, 48, 1, fl, ("tiny",))
row("tiny_epi9_x1", "fwd", (3, 1, 5, 7), 32, 48, 1, BIAS | LRELU, ("mfma", 32, False), off={"x": 1}, twin=("tiny_epi9", "tol"))
row("tiny_dgrad", "fwd", (2, 1, 8, 6), 64, 32, 1, MASK, ("tiny",), mode=1)

# ---- conv_small_n_kernel: Cout 1..4, both dimensionalities and tile shapes, VEC by channel count ----------------------------------------------
n = 0
for kz, shape in ((3, (2, 5, 5, 17)), (3, (1, 5, 9, 9)), (1, (2, 1, 17, 17)), (1, (1, 1, 33, 9))):
    for cout in (1, 2, 3, 4):
        tag = "%s_w%d_co%d" % ("3d" if kz == 3 else "2d", shape[3], cout)
        row("small_n_" + tag, "fwd", shape, 12, cout, kz, EPI[n % 6], ("small_n", True))
        row("small_n_" + tag + "_x1", "fwd", shape, 12, cout, kz, EPI[n % 6], ("small_n", False), off={"x": 1}, twin=("small_n_" + tag, "bits"))
        n += 1
row("small_n_c5", "fwd", (1, 3, 4, 13), 5, 3, 3, BIAS, ("small_n", False))        # Cin % 4 != 0
row("small_n_c3_c3", "fwd", (1, 1, 9, 9), 3, 3, 1, BIAS, ("small_n", False))      # thin on both sides: the thin-N rule comes first

# ---- conv_small_k_kernel: Cin 1..4, Cout >= 32; nwn = 1 (Cout <= 64) | 2 (<= 128) | 4 waves side by side --------------------------------------
n = 0
for kz, shape in ((3, (1, 3, 5, 17)), (3, (2, 5, 5, 9)), (1, (1, 1, 9, 17)), (1, (1, 1, 17, 9))):
    for cout in (32, 64, 96, 160, 300):
        row("small_k_%s_w%d_co%d" % ("3d" if kz == 3 else "2d", shape[3], cout), "fwd", shape, n % 4 + 1, cout, kz, EPI[n % 6], ("small_k",))
        n += 1
row("small_k_dgrad", "fwd", (1, 3, 5, 17), 3, 128, 3, MASK, ("small_k",), mode=1)

# ---- conv_thin_k_mfma_kernel: 3-D, Cin 1..4 -> 64 | 128, W % 8 == 0, W >= 32, W * Cin % 16 == 0, <= 448, B * D * H >= 4 ------------------------
# one load pass up to 64 float4 per row, two above; W = 40: the last chunk starts at W - 32; row counts 4 (the minimum), 5 and 15 (odd)
n = 0
ROWSETS = ((1, 1, 4), (1, 5, 1), (1, 3, 5))      # (B, D, H): 4, 5, 15 rows
for cout in (64, 128):
    for cin, w1, w2 in ((1, 32, 272), (2, 40, 136), (3, 32, 112), (4, 40, 112)):
        row("thin_k_%d_%d_w%d" % (cin, cout, w1), "fwd", ROWSETS[n % 3] + (w1,), cin, cout, 3, EPI[n % 6], ("thin_k", 1))
        row("thin_k_%d_%d_w%d" % (cin, cout, w2), "fwd", ROWSETS[(n + 1) % 3] + (w2,), cin, cout, 3, EPI[(n + 3) % 6], ("thin_k", 2))
        n += 1
row("thin_k_dgrad", "fwd", (1, 2, 3, 32), 3, 128, 3, MASK, ("thin_k", 1), mode=1)
TK = dict(entry="fwd", shape=(1, 2, 3, 32), cin=4, cout=128, kz=3)
ALLF = BIAS | LRELU | RESIDUAL | MASK
row("thin_k_base", flags=ALLF, reaches=("thin_k", 1), **TK)
row("thin_k_not_valu_only", flags=ALLF | VALU_ONLY, reaches=("small_k",), twin=("thin_k_base", "tol"), **TK)
for s in ("x", "y", "bias", "residual", "mask_src"):
    row("thin_k_not_%s1" % s, flags=ALLF, reaches=("small_k",), off={s: 1}, twin=("thin_k_base", "tol"), **TK)
row("thin_k_not_w24", "fwd", (1, 2, 3, 24), 4, 128, 3, BIAS, ("small_k",))
row("thin_k_not_w36", "fwd", (1, 2, 3, 36), 4, 128, 3, BIAS, ("small_k",))            # W % 8 != 0
row("thin_k_not_w40_c3", "fwd", (1, 2, 3, 40), 3, 128, 3, BIAS, ("small_k",))         # W * Cin % 16 != 0
row("thin_k_not_rows3", "fwd", (1, 3, 1, 32), 4, 128, 3, BIAS, ("small_k",))
row("thin_k_not_cout96", "fwd", (1, 2, 3, 32), 4, 96, 3, BIAS, ("small_k",))
row("thin_k_not_2d", "fwd", (6, 1, 1, 32), 4, 128, 1, BIAS, ("small_k",))

# ---- conv_thin_n_mfma_kernel: 3-D, 64 | 128 -> Cout 1..3, W % 8 == 0, W >= 32, BIAS / LRELU only; H 9 | 13 split in 2 | 3 ranges -----------------
TN_SHAPES = ((1, 2, 1, 32), (1, 2, 4, 40), (1, 3, 9, 32), (2, 1, 13, 40), (1, 2, 9, 40), (1, 1, 13, 32))
n = 0
for cin in (64, 128):
    for cout in (1, 2, 3):
        row("thin_n_%d_%d" % (cin, cout), "fwd", TN_SHAPES[n], cin, cout, 3, EPI_BL[n % 3], ("thin_n",))
        n += 1
TN = dict(entry="fwd", shape=(1, 2, 9, 32), cin=128, cout=3, kz=3)
row("thin_n_base", flags=BIAS | LRELU, reaches=("thin_n",), **TN)
row("thin_n_not_valu_only", flags=BIAS | LRELU | VALU_ONLY, reaches=("small_n", True), twin=("thin_n_base", "tol"), **TN)
row("thin_n_not_x1", flags=BIAS | LRELU, reaches=("small_n", False), off={"x": 1}, twin=("thin_n_base", "tol"), **TN)
row("thin_n_not_y1", flags=BIAS | LRELU, reaches=("small_n", True), off={"y": 1}, twin=("thin_n_base", "tol"), **TN)
row("thin_n_not_residual", flags=BIAS | RESIDUAL, reaches=("small_n", True), **TN)
row("thin_n_not_mask", flags=MASK, reaches=("small_n", True), **TN)
row("thin_n_not_w24", "fwd", (1, 2, 5, 24), 128, 3, 3, BIAS, ("small_n", True))
row("thin_n_not_w36", "fwd", (1, 2, 5, 36), 128, 3, 3, BIAS, ("small_n", True))
row("thin_n_not_cin32", "fwd", (1, 2, 5, 32), 32, 3, 3, BIAS, ("small_n", True))
row("thin_n_not_cout4", "fwd", (1, 2, 5, 32), 64, 4, 3, BIAS, ("small_n", True))
row("thin_n_not_2d", "fwd", (2, 1, 5, 32), 64, 3, 1, BIAS, ("small_n", True))

# ---- df_conv_s2_fwd: stride 2, every N tile x VEC x tile shape x dimensionality; shape = the OUTPUT grid ------------------------------------
n = 0
for kz in (3, 1):
    for w16 in (True, False):
        for nt, B, cout in ((128, 129, 65), (64, 129, 33), (32, 2, 31)):
            rid = "s2_%s_w%d_n%d" % ("3d" if kz == 3 else "2d", 16 if w16 else 8, nt)
            row(rid, "s2_fwd", _one_tile(kz == 3, w16, B), 16, cout, kz, EPI_BL[n % 3], ("mfma_s2", nt, True))
            row(rid + "_scalar", "s2_fwd", _one_tile(kz == 3, w16, B), 16, cout, kz, EPI_BL[n % 3], ("mfma_s2", nt, False), off={"x": 1},
                twin=(rid, "bits"))
            n += 1
for i, (kz, shape, cin, cout) in enumerate([(3, (1, 3, 5, 17), 5, 33), (3, (1, 1, 1, 1), 20, 5), (3, (3, 3, 3, 7), 12, 129), (1, (1, 1, 9, 17), 33, 31),
                                            (1, (9, 1, 1, 1), 20, 65), (1, (1, 1, 17, 9), 12, 5)]):
    row("s2_shape%d" % i, "s2_fwd", shape, cin, cout, kz, EPI_BL[i % 3], ("mfma_s2", 32, cin % 4 == 0))

# ---- df_upconv_fwd: 2 taps per axis, one launch over the parity classes; 3-D vector loads of a 32-multiple Kpad take 32-channel chunks -------
n = 0
for d3 in (True, False):
    for w16 in (True, False):
        for nt, cout in ((128, 65), (64, 33), (32, 5)):
            B = 2 if nt == 32 else 17 if d3 else 33           # 8 | 4 classes x B tiles > 128
            variants = (("c32", 32, 0, True, 32), ("c16", 16, 0, True, 16), ("scalar", 16, 1, False, 16)) if d3 else \
                       (("vec", 32, 0, True, 16), ("scalar", 32, 1, False, 16))
            for tag, cin, xo, vec, ck in variants:
                rid = "up_%s_w%d_n%d_%s" % ("3d" if d3 else "2d", 16 if w16 else 8, nt, tag)
                row(rid, "up_fwd", _one_tile(d3, w16, B), cin, cout, 3 if d3 else 1, EPI_BL[n % 3], ("mfma_up", nt, vec, ck), off={"x": xo},
                    twin=(rid[:-6] + ("c16" if d3 else "vec"), "bits") if tag == "scalar" else None)
            n += 1
for i, (kz, shape, cin, cout, ck) in enumerate([(3, (1, 3, 5, 17), 5, 33, 16), (3, (1, 1, 1, 1), 20, 5, 32), (3, (1, 3, 3, 7), 33, 129, 16),
                                                (1, (1, 1, 9, 17), 33, 31, 16), (1, (3, 1, 1, 1), 20, 65, 16), (1, (1, 1, 17, 9), 12, 5, 16)]):
    row("up_shape%d" % i, "up_fwd", shape, cin, cout, kz, EPI_BL[i % 3], ("mfma_up", 32, cin % 4 == 0, ck))      # Cin 20: Kpad 32

# ---- df_upconv_dgrad: the same kernels once per class, accumulating into acc; the kernel's N is the entry point's Cin ------------------------
row("updg_3d_ragged", "up_dgrad", (1, 3, 5, 17), 20, 12, 3, 0, ("mfma_up", 32, True, 16))
row("updg_3d_ragged_scalar", "up_dgrad", (1, 3, 5, 17), 20, 12, 3, 0, ("mfma_up", 32, False, 16), off={"x": 1}, twin=("updg_3d_ragged", "bits"))
row("updg_3d_c32", "up_dgrad", (2, 2, 4, 16), 33, 32, 3, 0, ("mfma_up", 32, True, 32))
row("updg_3d_w7_c5", "up_dgrad", (1, 3, 3, 7), 5, 5, 3, 0, ("mfma_up", 32, False, 16))
row("updg_3d_wide", "up_dgrad", (129, 2, 4, 16), 65, 16, 3, 0, ("mfma_up", 128, True, 16))
row("updg_2d_ragged", "up_dgrad", (3, 1, 9, 17), 31, 20, 1, 0, ("mfma_up", 32, True, 16))
row("updg_2d_wide", "up_dgrad", (129, 1, 8, 16), 129, 16, 1, 0, ("mfma_up", 128, True, 16))
row("updg_2d_n64", "up_dgrad", (129, 1, 16, 8), 33, 6, 1, 0, ("mfma_up", 64, False, 16))

# ---- df_conv_s2_dgrad: live-tap classes (Cin > 64, Cout % 4 == 0 padded to a 64-multiple, gy 16-byte aligned), else the generic kernel ---------
row("s2dg_3d_w17", "s2_dgrad", (1, 3, 5, 17), 68, 64, 3, 0, ("s2d",), form=1)
row("s2dg_3d_w17_g1", "s2_dgrad", (1, 3, 5, 17), 68, 64, 3, 0, ("mfma_up", 32, False, 16), off={"x": 1}, form=0, twin=("s2dg_3d_w17", "tol"))
row("s2dg_3d_w7", "s2_dgrad", (2, 3, 3, 7), 128, 52, 3, 0, ("s2d",), form=1)
row("s2dg_2d_w17", "s2_dgrad", (2, 1, 9, 17), 65, 128, 1, 0, ("s2d",), form=1)
row("s2dg_2d_w9", "s2_dgrad", (1, 1, 17, 9), 100, 64, 1, 0, ("s2d",), form=1)
row("s2dg_2d_w9_g1", "s2_dgrad", (1, 1, 17, 9), 100, 64, 1, 0, ("mfma_up", 32, False, 16), off={"x": 1}, form=0, twin=("s2dg_2d_w9", "tol"))
row("s2dg_generic_c32", "s2_dgrad", (1, 3, 5, 17), 32, 32, 3, 0, ("mfma_up", 32, True, 32), form=0)
row("s2dg_generic_cout48", "s2_dgrad", (1, 3, 5, 17), 128, 48, 3, 0, ("mfma_up", 32, True, 16), form=0)      # Kpad 48: no 64-multiple
row("s2dg_generic_cout6", "s2_dgrad", (2, 1, 9, 17), 128, 6, 1, 0, ("mfma_up", 32, False, 16), form=0)

# ---- bf16x3 mode: N tile by the padded N; Kpad rounds to 32 ---------------------------------------------------------------------------------
n = 0
for kz in (3, 1):
    for shape in ((1, 3 if kz == 3 else 1, 5, 17), (2, 3 if kz == 3 else 1, 5, 9)):
        for nt, cout in ((128, 65), (64, 33), (32, 17)):
            row("bf_%s_w%d_n%d" % ("3d" if kz == 3 else "2d", shape[3], nt), "fwd_bf16x3", shape, (16, 20, 36)[n % 3], cout, kz, EPI[n % 6], ("bf16", nt))
            cs = (1,) + shape[1:] if kz == 3 else shape
            row("bfup_%s_w%d_n%d" % ("3d" if kz == 3 else "2d", shape[3], nt), "up_fwd_bf16x3", cs, (36, 16, 20)[n % 3], cout, kz, EPI_BL[n % 3], ("bf16", nt))
            n += 1
row("bf_dgrad", "fwd_bf16x3", (1, 3, 5, 17), 36, 20, 3, MASK, ("bf16", 32), mode=1)
row("bfupdg_3d", "up_dgrad_bf16x3", (1, 3, 5, 17), 20, 36, 3, 0, ("bf16", 32))
row("bfupdg_3d_w7", "up_dgrad_bf16x3", (2, 3, 3, 7), 65, 16, 3, 0, ("bf16", 128))
row("bfupdg_2d", "up_dgrad_bf16x3", (2, 1, 9, 17), 33, 20, 1, 0, ("bf16", 64))

# ---- error rows: a code, no launch, the output untouched -----------------------------------------------------------------------------------------
OK_ROWS = list(ROWS)
FLAGGED = ("fwd", "fwd_bf16x3", "s2_fwd", "up_fwd", "up_fwd_bf16x3")
for e in ("fwd", "fwd_bf16x3", "s2_fwd", "s2_dgrad", "up_fwd", "up_fwd_bf16x3", "up_dgrad", "up_dgrad_bf16x3"):
    base = dict(entry=e, shape=(2, 2, 4, 16), cin=32, cout=32, kz=3)
    fl = 0 if e.endswith("dgrad") or e.endswith("dgrad_bf16x3") else BIAS
    for s in ("x", "wp", "y"):
        row("err_%s_null_%s" % (e, s), flags=fl, reaches=EINVAL, null=(s,), **base)
    for i in range(4):
        row("err_%s_extent%d_zero" % (e, i), e, tuple(0 if j == i else v for j, v in enumerate(base["shape"])), 32, 32, 3, fl, EINVAL)
    row("err_%s_extent_negative" % e, e, (2, 2, -4, 16), 32, 32, 3, fl, EINVAL)
    row("err_%s_cin_zero" % e, e, (2, 2, 4, 16), 0, 32, 3, fl, EINVAL)
    row("err_%s_cout_negative" % e, e, (2, 2, 4, 16), 32, -32, 3, fl, EINVAL)
    row("err_%s_kz2" % e, e, (2, 2, 4, 16), 32, 32, 2, fl, ESHAPE)
    row("err_%s_kz1_d2" % e, e, (2, 2, 4, 16), 32, 32, 1, fl, ESHAPE)
    row("err_%s_wp1" % e, flags=fl, reaches=EALIGN, off={"wp": 1}, **base)
    if e in FLAGGED:
        row("err_%s_bias_without" % e, flags=BIAS | LRELU, reaches=EINVAL, null=("bias",), **base)
        row("err_%s_addup" % e, flags=fl | ADDUP, reaches=EINVAL, **base)
        row("err_%s_bit10" % e, flags=fl | (1 << 10), reaches=EINVAL, **base)
        if e != "fwd":
            row("err_%s_valu_only" % e, flags=fl | VALU_ONLY, reaches=EINVAL, **base)
    if e in ("fwd", "fwd_bf16x3"):
        row("err_%s_residual_without" % e, flags=RESIDUAL, reaches=EINVAL, null=("residual",), **base)
        row("err_%s_mask_without" % e, flags=MASK, reaches=EINVAL, null=("mask_src",), **base)
    elif e in FLAGGED:
        row("err_%s_residual" % e, flags=BIAS | RESIDUAL, reaches=EINVAL, **base)
        row("err_%s_mask" % e, flags=MASK, reaches=EINVAL, **base)
    if e not in ("fwd", "fwd_bf16x3", "s2_fwd"):
        row("err_%s_cin4" % e, e, (2, 2, 4, 16), 4, 32, 3, fl, ESHAPE)
        row("err_%s_cout4" % e, e, (2, 2, 4, 16), 32, 4, 3, fl, ESHAPE)
    if e.endswith("bf16x3"):
        row("err_%s_x1" % e, flags=fl, reaches=EALIGN, off={"x": 1}, **base)
        row("err_%s_x2" % e, flags=fl, reaches=EALIGN, off={"x": 2}, **base)
        k18 = (32, 18) if e == "up_dgrad_bf16x3" else (18, 32)      # the K side (the dgrad's is Cout) must be a multiple of 4
        row("err_%s_k18" % e, e, (2, 2, 4, 16), k18[0], k18[1], 3, fl, ESHAPE)
        row("err_%s_cout8" % e, e, (2, 2, 4, 16), 32, 8, 3, fl, ESHAPE)
        row("err_%s_cin8" % e, e, (2, 2, 4, 16), 8, 32, 3, fl, ESHAPE)
        row("err_%s_k18_x1" % e, e, (2, 2, 4, 16), k18[0], k18[1], 3, fl, ESHAPE, off={"x": 1})      # the channel condition keeps its code
ERR_ROWS = [r for r in ROWS if isinstance(r["reaches"], int)]
assert len(OK_ROWS) + len(ERR_ROWS) == len(ROWS) and len({r["id"] for r in ROWS}) == len(ROWS)


def by_id(rid):
    return [r for r in ROWS if r["id"] == rid][0]


# ---- relations between rows ------------------------------------------------------------------------------------------------------------------------
# launch_n: "same packed operand ... same summation order per output, bitwise equal": image 0 of a row that keeps the 128 | 64 wide N tile against the
# same image alone (B = 1: the tile narrows to 32)
NARROWED = [r["id"] for r in OK_ROWS if r["reaches"][0] in ("mfma", "mfma_s2", "mfma_up") and r["reaches"][1] in (128, 64) and r["off"]["x"] == 0]
# conv_tiny2d_kernel: "Chosen by the image size alone (not the batch): results do not depend on the batch size"
TINY_BATCH = ["tiny_hw15_b5", "tiny_hw48", "tiny_epi15"]
