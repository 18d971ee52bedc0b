"""The case table of tests/test_gpu_wgrad_edges.py (GPU) and tests/test_wgrad_cases_host.py (no GPU): one row per branch of the host code
of csrc/conv_wgrad.hip -- conv_wgrad_impl, launch_thin_wgrad, df_conv_s2_wgrad, upconv_wgrad_impl.  Data only; imports nothing.

A row:  (id, entry, shape, Cin, Cout, kz, algo, bias, xoff, goff, form, reaches, twin)
  entry    "conv"  df_conv_wgrad_algo (algo None: df_conv_wgrad) | "conv_bf16x3" | "up"  df_upconv_wgrad_algo (None: df_upconv_wgrad) |
           "up_bf16x3" | "s2"  df_conv_s2_wgrad
  shape    (B, D, H, W): the extents the entry point takes -- the COARSE input grid for "up", the OUTPUT grid for "s2"; D = 1 when kz = 1
  bias     False: gb = NULL
  xoff, goff   payload offset of x / gy in floats: 0 = 16-byte aligned, 2 = 8-byte aligned only, 1 = 4-byte aligned only
  form     what df_conv_wgrad_form / df_upconv_wgrad_form answers for (shape, channels, kz, algo or 0).  The queries see no pointers and
           no precision mode, so for offset rows and bf16x3 rows this is the answer for aligned fp32 operands, not the kernel that runs.
           None for "s2" (no query).
  reaches  the kernel instantiations the call launches (in launch order, without the *_reduce_kernel and pad_rows_kernel launches), or
           "EALIGN" where the entry point must refuse the pointers.  OBSERVED, without a GPU: tests/test_wgrad_launches_host.py runs every
           row through tests/wgrad_launch_recorder.cpp, a program that links the release library, answers the HIP runtime calls of the
           host path itself and names each launched kernel from the library's symbol table.  tests/test_wgrad_cases_host.py keeps the
           column complete: the set of names here equals the set of weight-gradient instantiations in that symbol table.
  twin     for offset rows: (id of the aligned row with the same arguments, "bits" | "tol").  "bits": the offset call runs the same
           kernel, or one documented to give the same partial sums bit for bit (staged -> register-ring (x,y,z) kernel); "tol": another
           kernel, both within the tolerance of the oracle.

No instantiation of the release library is unreachable: UNREACHABLE stays empty (an entry would read {name: reason})."""

UNREACHABLE = {}


def _b(v):
    return "true" if v else "false"


def D(xv, gv, wp):
    return ["wgrad_kernel<%s,%s,%d>" % (_b(xv), _b(gv), wp)]


def WX(wp, cs):
    return ["wgrad_wx_kernel<%d,%d>" % (wp, cs)]


def WXY(wp, cs):      # two launches: the xi_y pair with and without the bias sum
    return ["wgrad_wxy_kernel<%d,%d,true>" % (wp, cs), "wgrad_wxy_kernel<%d,%d,false>" % (wp, cs)]


def XYZ(wp, cs):
    return ["wgrad_wxyz_fused_kernel<%d,%d>" % (wp, cs)]


def STG(wp):
    return ["wgrad_wxyz_staged_kernel<%d>" % wp]


def UXYZ(wp, cs):
    return ["wgrad_wxyz_up_fused_kernel<%d,%d>" % (wp, cs)]


def UP2(wp, cs):
    return ["wgrad_up2_kernel<%d,%d>" % (wp, cs)]


def S2(wp):
    return ["wgrad_s2_kernel<%d>" % wp]


def BF(w16):
    return ["wgrad_bf16x3_kernel<%d>" % w16]


def SN(kz, co):
    return ["wgrad_small_n_kernel<%d,%d>" % (kz, co)]


def TH(ct, nj, swap, np_):
    return ["wgrad_thin_mfma_kernel<%d,%d,%s,%d>" % (ct, nj, _b(swap), np_)]


FAMILIES = ("wgrad_kernel<", "wgrad_s2_kernel<", "wgrad_up2_kernel<", "wgrad_wx_kernel<", "wgrad_wxy_kernel<", "wgrad_wxyz_fused_kernel<",
            "wgrad_wxyz_up_fused_kernel<", "wgrad_wxyz_staged_kernel<", "wgrad_bf16x3_kernel<", "wgrad_small_n_kernel<",
            "wgrad_thin_mfma_kernel<")

T, F = True, False
ROWS = [
    # ---- df_conv_wgrad_algo, direct kernel: algo 1, or no Winograd form for the row length / channel counts ----------------------------
    ("dir_w64", "conv", (1, 1, 3, 64), 32, 48, 1, 1, T, 0, 0, 0, D(1, 1, 8), None),
    ("dir_w128", "conv", (1, 1, 2, 128), 18, 34, 1, 1, T, 0, 0, 0, D(1, 1, 16), None),
    ("dir_w32_3d", "conv", (2, 3, 3, 32), 34, 66, 3, 1, T, 0, 0, 0, D(1, 1, 4), None),
    ("dir_w112", "conv", (1, 1, 2, 112), 16, 16, 1, 1, T, 0, 0, 0, D(1, 1, 14), None),
    ("dir_w96", "conv", (1, 1, 3, 96), 130, 20, 1, 1, T, 0, 0, 0, D(1, 1, 12), None),       # two blocks of input channels
    ("dir_w56_nobias", "conv", (1, 1, 2, 56), 32, 32, 1, 1, F, 0, 0, 0, D(1, 1, 7), None),
    ("dir_w16_3d", "conv", (1, 3, 5, 16), 8, 130, 3, 1, T, 0, 0, 0, D(1, 1, 2), None),      # two blocks of output channels
    ("dir_w24", "conv", (2, 1, 3, 24), 64, 64, 1, 0, T, 0, 0, 0, D(1, 1, 3), None),         # no Winograd form at W = 24
    ("dir_w48", "conv", (1, 1, 2, 48), 128, 128, 1, 1, T, 0, 0, 0, D(1, 1, 6), None),
    ("dir_w20", "conv", (1, 1, 3, 20), 32, 32, 1, None, T, 0, 0, 0, D(1, 1, 0), None),      # W % 8 != 0; df_conv_wgrad itself
    ("dir_w8_3d", "conv", (1, 2, 2, 8), 66, 34, 3, 0, T, 0, 0, 0, D(1, 1, 0), None),        # W = 8 has no unrolled variant
    ("dir_5_7", "conv", (2, 3, 3, 9), 5, 7, 3, 0, T, 0, 0, 0, D(0, 0, 0), None),
    ("dir_6_7", "conv", (1, 1, 4, 10), 6, 7, 1, 0, T, 0, 0, 0, D(1, 0, 0), None),
    ("dir_5_6", "conv", (1, 1, 4, 16), 5, 6, 1, 0, T, 0, 0, 0, D(0, 1, 0), None),
    ("dir_3_64_2d", "conv", (1, 1, 4, 16), 3, 64, 1, 0, F, 0, 0, 0, D(0, 1, 0), None),      # thin, but the matrix-core form is 3-D only
    ("dir_2_128", "conv", (1, 2, 2, 16), 2, 128, 3, 0, T, 0, 0, 0, D(1, 1, 2), None),       # thin (SWAP) without an instantiation
    # ---- Winograd in x: algo 2, or the default where H is odd -------------------------------------------------------------------------
    ("wx_w64_c128", "conv", (1, 1, 3, 64), 128, 128, 1, 2, T, 0, 0, 1, WX(8, 128), None),
    ("wx_w64", "conv", (1, 1, 3, 64), 32, 64, 1, 2, T, 0, 0, 1, WX(8, 0), None),
    ("wx_w128", "conv", (1, 1, 2, 128), 128, 128, 1, 2, T, 0, 0, 1, WX(16, 0), None),
    ("wx_w96", "conv", (1, 1, 3, 96), 48, 32, 1, 2, T, 0, 0, 1, WX(12, 0), None),
    ("wx_w48", "conv", (1, 1, 3, 48), 128, 128, 1, 2, T, 0, 0, 1, WX(6, 0), None),
    ("wx_w112", "conv", (1, 1, 2, 112), 32, 32, 1, 2, T, 0, 0, 1, WX(14, 0), None),
    ("wx_w56_3d", "conv", (1, 2, 3, 56), 64, 96, 3, 2, T, 0, 0, 1, WX(7, 0), None),
    ("wx_w32_c128", "conv", (2, 1, 3, 32), 128, 128, 1, 2, T, 0, 0, 1, WX(4, 128), None),
    ("wx_w32", "conv", (1, 1, 3, 32), 96, 128, 1, 2, T, 0, 0, 1, WX(4, 0), None),
    ("wx_w32_nobias", "conv", (1, 1, 3, 32), 96, 128, 1, 2, F, 0, 0, 1, WX(4, 0), None),
    ("wx_w16_c128_3d", "conv", (1, 3, 3, 16), 128, 128, 3, 2, T, 0, 0, 1, WX(2, 128), None),
    ("wx_w16_default", "conv", (1, 1, 5, 16), 34, 130, 1, 0, T, 0, 0, 1, WX(2, 0), None),
    # ---- Winograd in (x,y): algo 3 (H even, >= 4), or the default from 4096 image rows ------------------------------------------------
    ("wxy_w64_c128", "conv", (1, 1, 4, 64), 128, 128, 1, 3, T, 0, 0, 2, WXY(8, 128), None),
    ("wxy_w64", "conv", (1, 1, 4, 64), 64, 32, 1, 3, T, 0, 0, 2, WXY(8, 0), None),
    ("wxy_w128", "conv", (1, 1, 4, 128), 32, 32, 1, 3, T, 0, 0, 2, WXY(16, 0), None),
    ("wxy_w96_c128", "conv", (1, 1, 4, 96), 128, 128, 1, 3, T, 0, 0, 2, WXY(12, 128), None),
    ("wxy_w96", "conv", (1, 1, 4, 96), 32, 96, 1, 3, T, 0, 0, 2, WXY(12, 0), None),
    ("wxy_w48_c128", "conv", (1, 1, 6, 48), 128, 128, 1, 3, T, 0, 0, 2, WXY(6, 128), None),
    ("wxy_w48", "conv", (1, 1, 4, 48), 96, 32, 1, 3, T, 0, 0, 2, WXY(6, 0), None),
    ("wxy_w112", "conv", (1, 1, 4, 112), 128, 128, 1, 3, T, 0, 0, 2, WXY(14, 0), None),
    ("wxy_w56", "conv", (1, 1, 4, 56), 32, 32, 1, 3, T, 0, 0, 2, WXY(7, 0), None),
    ("wxy_w32_c128_3d", "conv", (1, 3, 4, 32), 128, 128, 3, 3, T, 0, 0, 2, WXY(4, 128), None),
    ("wxy_w32_nobias", "conv", (2, 1, 4, 32), 34, 66, 1, 3, F, 0, 0, 2, WXY(4, 0), None),
    ("wxy_w16_c128", "conv", (1, 1, 4, 16), 128, 128, 1, 3, T, 0, 0, 2, WXY(2, 128), None),
    ("wxy_w16_default", "conv", (64, 1, 64, 16), 32, 32, 1, 0, T, 0, 0, 2, WXY(2, 0), None),
    # ---- Winograd in (x,y,z): register-ring kernel (algo 4, and every shape but the staged ones), staged default, zero-padded rows ------
    ("xyz_w64_c128_algo4", "conv", (1, 4, 4, 64), 128, 128, 3, 4, T, 0, 0, 3, XYZ(8, 128), None),
    ("xyz_w32_c128_algo4", "conv", (1, 4, 4, 32), 128, 128, 3, 4, T, 0, 0, 3, XYZ(4, 128), None),
    ("xyz_w16_c128", "conv", (2, 4, 6, 16), 128, 128, 3, 0, T, 0, 0, 3, XYZ(2, 128), None),
    ("xyz_w112_c128", "conv", (1, 4, 4, 112), 128, 128, 3, 0, T, 0, 0, 3, XYZ(14, 128), None),
    ("xyz_w128_c128_nobias", "conv", (1, 4, 4, 128), 128, 128, 3, 0, F, 0, 0, 3, XYZ(16, 128), None),
    ("xyz_w56_c128", "conv", (1, 4, 4, 56), 128, 128, 3, 4, T, 0, 0, 3, XYZ(7, 128), None),
    ("xyz_w128_c64", "conv", (1, 4, 4, 128), 64, 64, 3, 0, T, 0, 0, 3, XYZ(16, 64), None),
    ("xyz_w64_c64", "conv", (1, 4, 6, 64), 64, 64, 3, 0, T, 0, 0, 3, XYZ(8, 64), None),
    ("xyz_w32_c64_nobias", "conv", (1, 6, 4, 32), 64, 64, 3, 4, F, 0, 0, 3, XYZ(4, 64), None),
    ("xyz_w16_c64", "conv", (1, 4, 4, 16), 64, 64, 3, 0, T, 0, 0, 3, XYZ(2, 64), None),
    ("stg_w64", "conv", (1, 4, 4, 64), 128, 128, 3, 0, T, 0, 0, 3, STG(8), None),
    ("stg_w32", "conv", (1, 4, 4, 32), 128, 128, 3, None, T, 0, 0, 3, STG(4), None),
    ("pad_w28_c128", "conv", (1, 4, 4, 28), 128, 128, 3, 0, T, 0, 0, 3, STG(4), None),
    ("pad_w28_c128_algo4", "conv", (1, 4, 4, 28), 128, 128, 3, 4, F, 0, 0, 3, XYZ(4, 128), None),
    ("pad_w14_c64", "conv", (1, 4, 4, 14), 64, 64, 3, 4, T, 0, 0, 3, XYZ(2, 64), None),
    # ---- thin layers on the matrix cores (3-D, W % 16 == 0): both orientations, one and two passes per thin row (W * Ct > 256) ----------
    ("thin_128_1", "conv", (1, 2, 3, 16), 128, 1, 3, 0, T, 0, 0, 10, TH(1, 4, 0, 1), None),
    ("thin_128_2", "conv", (1, 2, 2, 32), 128, 2, 3, 0, T, 0, 0, 10, TH(2, 4, 0, 1), None),
    ("thin_128_3", "conv", (2, 3, 4, 32), 128, 3, 3, 0, T, 0, 0, 10, TH(3, 4, 0, 1), None),
    ("thin_128_4_nobias", "conv", (1, 2, 3, 64), 128, 4, 3, 0, F, 0, 0, 10, TH(4, 4, 0, 1), None),
    ("thin_128_3_two", "conv", (1, 2, 3, 96), 128, 3, 3, 0, T, 0, 0, 10, TH(3, 4, 0, 2), None),
    ("thin_64_3", "conv", (1, 2, 3, 16), 64, 3, 3, 0, T, 0, 0, 10, TH(3, 2, 0, 1), None),
    ("thin_64_3_two", "conv", (1, 2, 2, 112), 64, 3, 3, 0, T, 0, 0, 10, TH(3, 2, 0, 2), None),
    ("thin_3_128", "conv", (1, 2, 3, 16), 3, 128, 3, 0, T, 0, 0, 10, TH(3, 4, 1, 1), None),
    ("thin_3_128_two", "conv", (1, 2, 2, 96), 3, 128, 3, 0, T, 0, 0, 10, TH(3, 4, 1, 2), None),
    ("thin_3_64_nobias", "conv", (2, 2, 3, 32), 3, 64, 3, 0, F, 0, 0, 10, TH(3, 2, 1, 1), None),
    ("thin_3_64_two", "conv", (1, 2, 3, 128), 3, 64, 3, 0, T, 0, 0, 10, TH(3, 2, 1, 2), None),
    # ---- thin layers on the vector ALU: 2-D, algo 1, W % 16 != 0, a wide count without a matrix-core instantiation ----------------------
    ("small_3d_1", "conv", (1, 2, 3, 9), 64, 1, 3, 1, T, 0, 0, 11, SN(3, 1), None),
    ("small_3d_2", "conv", (1, 2, 2, 16), 64, 2, 3, 0, T, 0, 0, 11, SN(3, 2), None),          # 64 -> 2 has no matrix-core variant
    ("small_3d_3", "conv", (1, 3, 3, 12), 192, 3, 3, 0, T, 0, 0, 11, SN(3, 3), None),         # three 64-channel blocks, idle streams
    ("small_3d_4_nobias", "conv", (1, 2, 2, 8), 128, 4, 3, 0, F, 0, 0, 11, SN(3, 4), None),
    ("small_2d_1", "conv", (1, 1, 5, 12), 64, 1, 1, 0, T, 0, 0, 11, SN(1, 1), None),
    ("small_2d_2", "conv", (2, 1, 3, 16), 128, 2, 1, 0, T, 0, 0, 11, SN(1, 2), None),
    ("small_2d_3", "conv", (1, 1, 4, 20), 64, 3, 1, 0, T, 0, 0, 11, SN(1, 3), None),
    ("small_2d_4", "conv", (1, 1, 3, 7), 64, 4, 1, 0, T, 0, 0, 11, SN(1, 4), None),
    # ---- df_conv_wgrad_bf16x3: split-operand kernel at W = 16 | 32 | 64 | 96, the fp32 kernels everywhere else --------------------------
    ("cbf_w16", "conv_bf16x3", (1, 1, 3, 16), 16, 32, 1, None, T, 0, 0, 0, BF(1), None),
    ("cbf_w32_nobias", "conv_bf16x3", (2, 1, 3, 32), 32, 32, 1, None, F, 0, 0, 1, BF(2), None),
    ("cbf_w64_3d", "conv_bf16x3", (1, 2, 3, 64), 64, 64, 3, None, T, 0, 0, 1, BF(4), None),
    ("cbf_w96", "conv_bf16x3", (1, 1, 2, 96), 18, 130, 1, None, T, 0, 0, 0, BF(6), None),
    ("cbf_xyz", "conv_bf16x3", (1, 4, 4, 16), 64, 64, 3, None, T, 0, 0, 3, XYZ(2, 64), None),   # (x,y,z) exists: both modes take it
    ("cbf_w24", "conv_bf16x3", (2, 1, 3, 24), 64, 64, 1, None, T, 0, 0, 0, D(1, 1, 3), None),
    ("cbf_thin", "conv_bf16x3", (2, 3, 4, 32), 128, 3, 3, None, T, 0, 0, 10, SN(3, 3), None),   # this mode skips the matrix-core thin form
    ("cbf_pad", "conv_bf16x3", (1, 4, 4, 14), 64, 64, 3, None, T, 0, 0, 3, XYZ(2, 64), None),
    # ---- df_conv_s2_wgrad -----------------------------------------------------------------------------------------------------------------
    ("s2_w8", "s2", (1, 1, 2, 8), 32, 32, 1, None, T, 0, 0, None, S2(1), None),
    ("s2_w16", "s2", (2, 1, 3, 16), 34, 66, 1, None, T, 0, 0, None, S2(2), None),
    ("s2_w32_3d", "s2", (1, 2, 2, 32), 64, 32, 3, None, T, 0, 0, None, S2(4), None),
    ("s2_w64_nobias", "s2", (1, 1, 2, 64), 32, 130, 1, None, F, 0, 0, None, S2(8), None),
    ("s2_w8_3d", "s2", (1, 3, 2, 8), 128, 128, 3, None, T, 0, 0, None, S2(1), None),
    # ---- df_upconv_wgrad_algo: 27-point form (3-D, fine extents with an (x,y,z) instantiation, algo 0 | 4) -------------------------------
    ("uxyz_w64_c128", "up", (1, 2, 2, 32), 128, 128, 3, 0, T, 0, 0, 3, UXYZ(8, 128), None),
    ("uxyz_w32_c128", "up", (1, 2, 2, 16), 128, 128, 3, 0, T, 0, 0, 3, UXYZ(4, 128), None),
    ("uxyz_w16_c128", "up", (2, 2, 2, 8), 128, 128, 3, None, T, 0, 0, 3, UXYZ(2, 128), None),
    ("uxyz_w112_c128", "up", (1, 2, 2, 56), 128, 128, 3, 0, T, 0, 0, 3, UXYZ(14, 128), None),
    ("uxyz_w128_c128_nobias", "up", (1, 2, 2, 64), 128, 128, 3, 0, F, 0, 0, 3, UXYZ(16, 128), None),
    ("uxyz_w56_c128", "up", (1, 2, 2, 28), 128, 128, 3, 4, T, 0, 0, 3, UXYZ(7, 128), None),
    ("uxyz_w128_c64", "up", (1, 2, 2, 64), 64, 64, 3, 0, T, 0, 0, 3, UXYZ(16, 64), None),
    ("uxyz_w64_c64", "up", (1, 3, 2, 32), 64, 64, 3, 0, T, 0, 0, 3, UXYZ(8, 64), None),
    ("uxyz_w32_c64", "up", (1, 2, 2, 16), 64, 64, 3, 4, T, 0, 0, 3, UXYZ(4, 64), None),
    ("uxyz_w16_c64_nobias", "up", (1, 2, 2, 8), 64, 64, 3, 0, F, 0, 0, 3, UXYZ(2, 64), None),
    # ---- ... three-product parity-class kernel (algo != 1) ------------------------------------------------------------------------------------
    ("up2_w32_c128", "up", (2, 1, 3, 32), 128, 128, 1, 0, T, 0, 0, 0, UP2(4, 128), None),
    ("up2_w32_c128_3d_algo2", "up", (1, 2, 2, 32), 128, 128, 3, 2, T, 0, 0, 0, UP2(4, 128), None),
    ("up2_w48_c128", "up", (1, 1, 2, 48), 128, 128, 1, 0, T, 0, 0, 0, UP2(6, 128), None),
    ("up2_w24_c128_nobias", "up", (1, 1, 3, 24), 128, 128, 1, 0, F, 0, 0, 0, UP2(3, 128), None),
    ("up2_w16", "up", (1, 1, 3, 16), 32, 48, 1, 0, T, 0, 0, 0, UP2(2, 0), None),
    ("up2_w16_3d_dc1", "up", (1, 1, 2, 16), 32, 32, 3, 0, T, 0, 0, 0, UP2(2, 0), None),
    ("up2_w8", "up", (2, 1, 2, 8), 34, 66, 1, 0, T, 0, 0, 0, UP2(1, 0), None),
    ("up2_w8_3d_algo3", "up", (1, 2, 3, 8), 32, 32, 3, 3, T, 0, 0, 0, UP2(1, 0), None),
    # ---- ... generic direct kernel on the parity classes (algo 1, or no three-product variant) -------------------------------------------------
    ("upg_w32_c128_algo1", "up", (1, 1, 2, 32), 128, 128, 1, 1, T, 0, 0, 0, D(1, 1, 4), None),
    ("upg_w48_c128_algo1", "up", (1, 1, 2, 48), 128, 128, 1, 1, T, 0, 0, 0, D(1, 1, 0), None),
    ("upg_w24_c128_algo1", "up", (1, 1, 2, 24), 128, 128, 1, 1, T, 0, 0, 0, D(1, 1, 0), None),
    ("upg_w16_algo1", "up", (1, 1, 3, 16), 32, 48, 1, 1, T, 0, 0, 0, D(1, 1, 2), None),
    ("upg_w16_3d_algo1", "up", (1, 2, 2, 16), 64, 64, 3, 1, T, 0, 0, 0, D(1, 1, 2), None),
    ("upg_w8_algo1", "up", (1, 1, 2, 8), 32, 32, 1, 1, T, 0, 0, 0, D(1, 1, 0), None),
    ("upg_w64_algo1", "up", (1, 1, 2, 64), 64, 64, 1, 1, T, 0, 0, 0, D(1, 1, 8), None),
    ("upg_w64_default", "up", (1, 1, 2, 64), 32, 48, 1, 0, T, 0, 0, 0, D(1, 1, 8), None),
    ("upg_w32_default", "up", (1, 1, 2, 32), 64, 64, 1, 0, T, 0, 0, 0, D(1, 1, 4), None),
    ("upg_w56_algo1_nobias", "up", (1, 1, 2, 56), 32, 32, 1, 1, F, 0, 0, 0, D(1, 1, 7), None),
    ("upg_w7_3d", "up", (1, 3, 5, 7), 64, 64, 3, 0, T, 0, 0, 0, D(1, 1, 0), None),
    ("upg_w48_c64", "up", (1, 1, 2, 48), 64, 64, 1, 0, T, 0, 0, 0, D(1, 1, 0), None),
    # ---- df_upconv_wgrad_bf16x3: split-operand kernel with a.up = 1 at Wc = 16 | 32 | 64 | 96 where the 27-point form is not available ------
    ("ubf_w16", "up_bf16x3", (1, 1, 3, 16), 32, 32, 1, None, T, 0, 0, 0, BF(1), None),
    ("ubf_w16_nobias", "up_bf16x3", (2, 1, 2, 16), 16, 48, 1, None, F, 0, 0, 0, BF(1), None),
    ("ubf_w32", "up_bf16x3", (1, 1, 2, 32), 128, 128, 1, None, T, 0, 0, 0, BF(2), None),
    ("ubf_w32_nobias", "up_bf16x3", (1, 1, 3, 32), 64, 32, 1, None, F, 0, 0, 0, BF(2), None),
    ("ubf_w64", "up_bf16x3", (1, 1, 2, 64), 64, 64, 1, None, T, 0, 0, 0, BF(4), None),
    ("ubf_w64_nobias", "up_bf16x3", (1, 1, 2, 64), 32, 66, 1, None, F, 0, 0, 0, BF(4), None),
    ("ubf_w96", "up_bf16x3", (1, 1, 2, 96), 32, 32, 1, None, T, 0, 0, 0, BF(6), None),
    ("ubf_w96_nobias", "up_bf16x3", (1, 1, 2, 96), 128, 128, 1, None, F, 0, 0, 0, BF(6), None),
    ("ubf_w16_3d_c32", "up_bf16x3", (1, 2, 3, 16), 32, 32, 3, None, T, 0, 0, 0, BF(1), None),
    ("ubf_w32_3d_hc1", "up_bf16x3", (1, 2, 1, 32), 128, 128, 3, None, T, 0, 0, 0, BF(2), None),
    ("ubf_xyz", "up_bf16x3", (1, 2, 2, 16), 128, 128, 3, None, T, 0, 0, 3, UXYZ(4, 128), None),   # 27-point form: both modes take it
    ("ubf_w7", "up_bf16x3", (1, 1, 3, 7), 32, 32, 1, None, T, 0, 0, 0, D(1, 1, 0), None),
    ("ubf_w8", "up_bf16x3", (2, 1, 2, 8), 34, 66, 1, None, T, 0, 0, 0, UP2(1, 0), None),
]


def _offsets(base, by_offset):
    """the six offset variants of the aligned row ``base``: by_offset[(xoff, goff)] = (reaches, "bits" | "tol")"""
    out = []
    for (xo, go), (reaches, rel) in sorted(by_offset.items()):
        out.append(("%s_x%d_g%d" % (base[0], xo, go),) + base[1:8] + (xo, go, base[10], reaches, (base[0], rel)))
    return out


def _row(rid):
    return [r for r in ROWS if r[0] == rid][0]


def _scalar(same8, same8_rel="bits"):
    """8-byte offsets keep ``same8``; a 4-byte offset of x / gy / both takes the direct kernel with scalar loads of that operand"""
    return {(2, 0): (same8, same8_rel), (0, 2): (same8, same8_rel), (2, 2): (same8, same8_rel),
            (1, 0): (D(0, 1, 0), "tol"), (0, 1): (D(1, 0, 0), "tol"), (1, 1): (D(0, 0, 0), "tol")}


# ---- operand alignment: one shape per family -------------------------------------------------------------------------------------------------
ALIGN_ROWS = (
    # thin layer: the matrix-core kernel needs 16 bytes (raw buffer loads of 16 | 8 bytes, 16-byte loads of the thin rows)
    _offsets(_row("thin_128_3"), {o: (SN(3, 3), "tol") for o in ((2, 0), (0, 2), (2, 2), (1, 0), (0, 1), (1, 1))})
    # zero-padded rows: pad_rows_kernel copies 16 bytes per lane; without it W = 28 has no Winograd form
    + _offsets(_row("pad_w28_c128"), _scalar(D(1, 1, 0), "tol"))
    # staged default: 16-byte row loads; at 8 bytes the register-ring (x,y,z) kernel, which gives the same bits
    + _offsets(_row("stg_w32"), _scalar(XYZ(4, 128)))
    + _offsets(_row("xyz_w16_c64"), _scalar(XYZ(2, 64)))
    + _offsets(_row("wx_w32"), _scalar(WX(4, 0)))
    # 27-point up-sampling form: 16 bytes; at 8 bytes the three-product parity-class kernel
    + _offsets(_row("uxyz_w16_c128"), _scalar(UP2(1, 0), "tol"))
    + _offsets(_row("up2_w16"), _scalar(UP2(2, 0)))
    + _offsets(_row("upg_w64_default"), _scalar(D(1, 1, 8)))
    # split-operand kernels: 8 bytes
    + _offsets(_row("ubf_w16"), {(2, 2): (BF(1), "bits"), (1, 1): (D(0, 0, 0), "tol"), (0, 1): (D(1, 0, 0), "tol")})
    + _offsets(_row("cbf_w16"), {(2, 0): (BF(1), "bits"), (1, 0): (D(0, 1, 0), "tol")})
    # stride 2: 8 bytes or DF_EALIGN
    + _offsets(_row("s2_w16"), {(2, 0): (S2(2), "bits"), (0, 2): (S2(2), "bits"), (2, 2): (S2(2), "bits"),
                                (1, 0): ("EALIGN", "tol"), (0, 1): ("EALIGN", "tol"), (1, 1): ("EALIGN", "tol")})
)
ALL_ROWS = ROWS + ALIGN_ROWS

# ---- relations between rows -------------------------------------------------------------------------------------------------------------------
# zero-padded rows: (row, padded row length).  conv_wgrad_impl copies x and gy into rows of Wp and calls itself with the same B, D, H,
# channels, precision mode and algo argument, so make_plan gets the same arguments as for a caller-made padded tensor: the same kernel,
# the same partial ranges, the same reduction order -- equal bit for bit.
PADDED = [("pad_w28_c128", 32), ("pad_w28_c128_algo4", 32), ("pad_w14_c64", 16)]
# one sample among three: rows run at B = 3 with the row's sample in the middle and zeros around it
BATCH_ROWS = ["dir_w64", "wx_w32", "wxy_w32_nobias", "xyz_w16_c64", "stg_w32", "thin_128_3", "thin_3_128", "small_3d_3", "cbf_w16", "s2_w16",
              "uxyz_w32_c64", "up2_w16", "upg_w7_3d", "ubf_w16_3d_c32"]
