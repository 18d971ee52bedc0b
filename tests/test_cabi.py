"""CPU-side checks of the C-ABI boundary: the library loads, exports every symbol the public header declares,
and rejects bad arguments with the documented status codes BEFORE touching the device (no GPU needed)."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from deep_fluids_amd import _lib


def test_library_present_and_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "build it first: python -c 'import __graft_entry__ as g; g.build()'"
    declared = _lib.declared_symbols()
    assert len(declared) >= 28
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in declared if s not in exported]
    assert not missing, missing
    assert sorted(_lib.SIGNATURES) == declared          # the ctypes table binds exactly the header
    # ... and the release library exports nothing BUT the header: no debug / tuning entry points, no mutable switches
    extra = sorted(s for s in exported if s.startswith("df_") and s not in declared)
    assert not extra, extra


def _abi_fingerprint(signatures):
    """SHA-256 over the ctypes class names (on the LP64 hosts of ROCm c_int64 is `c_long` and c_uint32 `c_uint`)"""
    lines = sorted("%s:%s:%s" % (n, r.__name__, ",".join(a.__name__ for a in args)) for n, (r, args) in signatures.items())
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def test_signatures_are_parsed_from_the_header_completely_and_strictly():
    P, I64, I32, F32, U32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint32
    known = {P, I64, I32, F32, U32, ctypes.c_char_p}
    assert set(_lib.CTYPES.values()) == known
    assert len(_lib.SIGNATURES) == len(_lib.declared_symbols()) == 239
    for name, (res, args) in _lib.SIGNATURES.items():
        assert res in known and all(a in known for a in args), name
        assert ctypes.c_char_p not in args, name
    # rows of the hand-written table this parser replaced, verbatim: one per type the dictionary knows
    pins = {
        "df_version": (I32, []),
        "df_last_error": (ctypes.c_char_p, []),
        "df_mg_omega": (F32, []),
        "df_pressure_workspace_bytes": (I64, [I64, I64, I64, I64]),
        "df_resample_scatter3d": (I32, [P, P, P, P, P, P, P, P, P, I64, I64, I64, I64, I64, I32, U32, U32, P]),
        "df_density_noise_inflow3d": (I32, [P, P, P, P, F32, F32, F32, I64, I64, I64, I64, I32, P]),
        "df_wall_buoyancy3d": (I32, [P, P, P, I64, I64, I64, I64, F32, F32, F32, I32, P]),
        "df_conv_fwd": (I32, [P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I32, I32, F32, P]),
        "df_mesh_emit": (I32, [P, P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I32, I32, F32, P]),
        "df_pressure_cg_direction_mg": (I32, [P, I64, P, I64, P, I32, I64, I64, I64, I64, I32, I32, I64, F32, I64, P]),
    }
    for name, row in pins.items():
        assert _lib.SIGNATURES[name] == row, name
    # header text, not only the file: what the dictionary does not know is refused by name, never bound as a guess
    sigs, consts = _lib.parse_header("#define DF_VERSION 3 /* c */\nenum { DF_A = 1, DF_B = -2 };\n"
                                     "int64_t df_f(const float* x, int n,\n         uint32_t s, df_stream_t stream);\nfloat df_g(void);\n")
    assert sigs == {"df_f": (I64, [P, I32, U32, P]), "df_g": (F32, [])} and consts == {"DF_VERSION": 3, "DF_A": 1, "DF_B": -2}
    with pytest.raises(_lib.DeepFluidsHipError, match=r"df_scale.*`double`"):
        _lib.parse_header("int df_ok(int64_t n);\nint df_scale(float* x, double s, int64_t n);\n")
    with pytest.raises(_lib.DeepFluidsHipError, match=r"df_norm.*`double`"):
        _lib.parse_header("int df_ok(int64_t n);\ndouble df_norm(const float* x, int64_t n);\n")
    with pytest.raises(_lib.DeepFluidsHipError, match=r"df_taps.*`float w\[27\]`"):
        _lib.parse_header("int df_taps(float w[27], int64_t n);\n")
    with pytest.raises(_lib.DeepFluidsHipError, match="not a .* prototype: int helper"):          # nothing with a parenthesis is skipped
        _lib.parse_header("int df_ok(int64_t n);\nint helper(int64_t n);\n")


def test_a_missing_header_is_named(monkeypatch, tmp_path):
    gone = str(tmp_path / "deepfluids_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", gone)
    with pytest.raises(_lib.DeepFluidsHipError, match=re.escape(gone)):
        _lib._read_header()


@pytest.fixture(scope="module")
def header_as_compiled(tmp_path_factory):
    """What a C compiler makes of the header: {name: int} for DF_VERSION, every enumerator, sizeof(df_noise_params) and `offsetof.<field>`"""
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    enumerators = [n for body in re.findall(r"\benum\s*\{(.*?)\}", src, re.S) for n in re.findall(r"\b(DF_\w+)\s*=", body)]
    assert len(enumerators) == 11, enumerators
    lines = ['printf("%s %%ld\\n", (long)%s);' % (n, n) for n in ["DF_VERSION"] + enumerators]
    lines.append('printf("sizeof %ld\\n", (long)sizeof(df_noise_params));')
    lines += ['printf("offsetof.%s %%ld\\n", (long)offsetof(df_noise_params, %s));' % (f[0], f[0]) for f in _lib.NoiseParams._fields_]
    d = tmp_path_factory.mktemp("cabi")
    (d / "layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "deepfluids_hip.h"\nint main(void) {\n  %s\n  return 0;\n}\n'
                                % "\n  ".join(lines))
    cc = next((c for c in ("cc", "gcc", "clang", "hipcc", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    assert cc is not None, "no C compiler (cc, gcc, clang, hipcc) found: the struct mirror cannot be checked"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.dirname(_lib.HEADER_PATH), str(d / "layout.c"), "-o", str(d / "layout")])
    out = subprocess.check_output([str(d / "layout")]).decode()
    return enumerators, {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_noise_params_mirrors_the_c_struct(header_as_compiled):
    c = header_as_compiled[1]
    assert ctypes.sizeof(_lib.NoiseParams) == c["sizeof"] == 56
    for name, _ in _lib.NoiseParams._fields_:
        assert getattr(_lib.NoiseParams, name).offset == c["offsetof." + name], name
    assert sum(ctypes.sizeof(t) for _, t in _lib.NoiseParams._fields_) == c["sizeof"]      # no padding: no field of the C struct is left out


def test_constants_come_from_the_header(header_as_compiled):
    enumerators, c = header_as_compiled
    for name in enumerators + ["DF_VERSION"]:
        assert getattr(_lib, name) == c[name] == _lib.CONSTANTS[name], name
    assert _lib.DF_VERSION == 207
    assert (_lib.DF_OK, _lib.DF_EINVAL, _lib.DF_ESHAPE, _lib.DF_EALIGN, _lib.DF_EWORKSPACE) == (0, -1, -2, -3, -4)
    assert (_lib.DF_CONV_LRELU, _lib.DF_CONV_RESIDUAL, _lib.DF_CONV_MASK, _lib.DF_CONV_BIAS, _lib.DF_CONV_ADDUP,
            _lib.DF_CONV_VALU_ONLY) == (1, 2, 4, 8, 16, 32)


def test_query_memoises_only_entry_points_without_a_pointer_argument(monkeypatch):
    class Stub(object):
        def __init__(self):
            self.calls = []

        def df_conv_s2_dgrad_form(self, *args):
            self.calls.append(("df_conv_s2_dgrad_form",) + args)
            return 1

        def df_l1_mean_workspace_bytes(self, n):
            self.calls.append(("df_l1_mean_workspace_bytes", n))
            return 8 * n

    stub = Stub()
    monkeypatch.setattr(_lib, "_lib", stub)
    monkeypatch.setattr(_lib, "_QUERY_CACHE", {})          # the stub's answers must not outlive the test
    assert ctypes.c_void_p in _lib.SIGNATURES["df_conv_s2_dgrad_form"][1]
    assert _lib.query("df_conv_s2_dgrad_form", 0x7F0000001000, 64, 64) == 1
    assert _lib.query("df_conv_s2_dgrad_form", 0x7F0000002000, 64, 64) == 1
    assert _lib.query("df_conv_s2_dgrad_form", 0x7F0000002000, 64, 64) == 1
    assert _lib._QUERY_CACHE == {} and len(stub.calls) == 3          # asked every time, nothing kept
    assert _lib.query("df_l1_mean_workspace_bytes", 100) == 800
    assert _lib.query("df_l1_mean_workspace_bytes", 100) == 800
    assert _lib._QUERY_CACHE == {("df_l1_mean_workspace_bytes", 100): 800} and len(stub.calls) == 4      # the second is a cache hit


def test_release_library_holds_only_the_production_kernel_instantiations():
    """The shipped library must hold exactly the production instantiations of `wino3d_kernel<FL, MODE>` -- MODE in {0 plain, 2 pooled
    adjoint, 3 up-sampling-aware forward on the coarse halo block} -- with these epilogues (FL): -1 run-time flags, 0 none, 2 residual,
    4 mask, 9 bias + lrelu, 25 ... + add-up, 73 ... + sign words, 132 mask from sign words, 345 add-up + sign words without the primary
    output."""
    out = subprocess.check_output(["nm", "-C", _lib.LIB_PATH]).decode()
    import re
    inst = sorted(set(re.findall(r"wino3d_kernel<([-0-9, ]+)>", out)))
    got = sorted(tuple(int(v) for v in i.split(",")) for i in inst)
    assert got, "no wino3d_kernel symbols in the library (stripped?)"
    assert all(len(g) == 2 and g[1] in (0, 2, 3) for g in got), got
    want = sorted([(f, 0) for f in (-1, 0, 2, 4, 9, 25, 73, 132, 345)] + [(0, 2), (9, 3), (73, 3)])
    assert got == want, got
    # the 2-D twin and the weight-gradient kernels have no experiment template switches; there are no tuning knobs (df_debug_* entry points)
    assert "df_debug_" not in out

    def family(name):
        """the template argument lists of `name<...>` in the library, as a set of tuples"""
        return {tuple(v.strip() for v in a.split(",")) for a in re.findall(r"\b%s<([^<>]*)>" % name, out)}

    # the 3-D stencils (stencil.hip, df_jacobian3d_fwd / _bwd): <WJ, WC> | <HJ, HC> = which outputs / incoming gradients there are -- both,
    # the Jacobian alone, the curl alone; the LDS-staged adjoint takes one gradient of 9 or 3 floats per record
    pairs = {("true", "true"), ("true", "false"), ("false", "true")}
    assert family("jacobian3d_fwd_vec_kernel") == pairs
    assert family("jacobian3d_bwd_vec_kernel") == pairs
    assert family("jacobian3d_bwd_lds_kernel") == {("3",), ("9",)}
    # the fused tail (velocity_loss.hip): tiles of kTileZ x kTileY = 2 x 8 rows of X = 64 | 112 | 128 voxels (XQ = X / 4), and the two
    # 16-byte kernels, which are no templates
    assert family("velocity_loss3d_tile_kernel") == {(xq, "2", "8") for xq in ("16", "28", "32")}
    for name in ("velocity_du3d_vec_kernel", "velocity_jl1_3d_vec_kernel"):
        assert name + "(" in out and name + "<" not in out, name
    for gone in ("velocity_loss3d_march", "velocity_jl1_3d_kernel(", "velocity_du3d_kernel("):
        assert gone not in out, gone
    # conv_bf16x3_kernel<KZ, TZ, TY, TX, WM, WN, MB, NB, KT>: nine arguments, no debug variant behind them
    bf16 = family("conv_bf16x3_kernel")
    assert bf16 and all(len(a) == 9 for a in bf16), sorted(bf16)


def test_version_and_error_convention():
    h = _lib.lib()
    assert h.df_version() == 207
    # the binding derived from the header, as sorted lines `name:restype:argtype,...`.  This digest is that of the hand-written table the
    # package carried up to version 207 (239 entry points);  a header change that alters it is an ABI change: DF_VERSION and the digest move together
    assert _abi_fingerprint(_lib.SIGNATURES) == "599d6e28e9bad131b0bc5c1ea177df2c3651c10931d88a6cea69aca1f2264348"
    # null pointers / bad extents are argument errors (< 0) caught on the host, with a message
    assert h.df_jacobian3d_fwd(None, None, None, 1, 4, 4, 4, None) == -1
    assert b"null input" in h.df_last_error()
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.addressof(buf)
    addr16 = (addr + 15) & ~15
    assert h.df_jacobian3d_fwd(addr16, addr16, addr16, 1, 1, 4, 4, None) == -2        # extent 1 < 2: DF_ESHAPE
    assert b">= 2" in h.df_last_error()
    assert h.df_jacobian3d_fwd(addr16, addr16 + 4, None, 1, 2, 2, 2, None) == -3      # misaligned output: DF_EALIGN
    assert h.df_conv_fwd(addr16, addr16, None, None, None, addr16, 1, 1, 4, 4, 16, 16, 2, 0, 0.0, None) == -2
    assert h.df_conv_fwd(addr16, addr16, None, None, None, addr16, 1, 1, 4, 4, 16, 16, 1, 8, 0.0, None) == -1  # BIAS flag, no bias
    assert h.df_l1_mean_fwd(addr16, addr16, 16, addr16, addr16, 8, None) == -4        # workspace too small
    assert h.df_conv_packed_elems(27, 128, 128, 0) == 27 * 128 * 128
    assert h.df_conv_packed_elems(27, 128, 3, 0) == 27 * 128 * 32                      # N padded to the 32-wide tile
    assert h.df_conv_packed_elems(27, 128, 3, 1) == 27 * 16 * 128                      # dgrad: K = 3 -> 16
    assert h.df_conv_wgrad_workspace_bytes(16, 64, 96, 64, 128, 128, 3) > 0


def test_python_surface_fails_loudly_without_gpu():
    import torch
    from deep_fluids_amd import ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.curl3(torch.zeros((1, 4, 4, 4, 3)))
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.l1_mean(torch.zeros(8), torch.zeros(8))


def test_sign_word_layout_decoder_roundtrip():
    """ops.sign_bits_to_mask documents the sign-word layout of conv_wino.hip (kSignBits): encode a random mask with an index-form restatement
    of the kernel's epilogue addressing (byte = (tile block, cout slice, wave = (th, xi_z), cout 16-block, lane = (kq, tl)), bit s =
    (dz, dy, dx)) and decode it back -- ragged extents included (bits of outputs outside the tensor are don't-care)."""
    import numpy as np
    import torch
    from deep_fluids_amd import ops
    rng = np.random.RandomState(0)
    for (B, D, H, W, C) in ((1, 4, 8, 8, 32), (2, 6, 10, 12, 64), (1, 5, 7, 9, 32)):
        m = rng.rand(B, D, H, W, C) > 0.5
        nbz, nby, nbx, ncs = -(-D // 4), -(-H // 8), -(-W // 8), C // 32
        by = np.zeros(B * nbz * nby * nbx * ncs * 1024, np.uint8)
        for b, z, y, x, c in zip(*np.nonzero(m)):
            bz, by_, bx = z // 4, y // 8, x // 8
            th, kq, xz = (z % 4) // 2, (y % 8) // 2, (x % 8) // 2
            s = (z % 2) * 4 + (y % 2) * 2 + (x % 2)
            cs, nb, tl = c // 32, (c // 16) % 2, c % 16
            blk = ((b * nbz + bz) * nby + by_) * nbx + bx
            by[(blk * ncs + cs) * 1024 + (th * 4 + xz) * 128 + nb * 64 + kq * 16 + tl] |= 1 << s
        pad = (-by.size) % 8
        words = torch.from_numpy(np.concatenate([by, np.zeros(pad, np.uint8)])).view(torch.int64)
        got = ops.sign_bits_to_mask(words, (B, D, H, W), C).numpy()
        np.testing.assert_array_equal(got, m)
