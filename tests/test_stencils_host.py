"""Host gate of tests/test_gpu_stencil_edges.py (no GPU):
  1. every argument check of the stencil and loss-tail entry points returns its documented code and message BEFORE any launch -- the
     pointers are host addresses that are never dereferenced, and only calls whose entry point returns at a DF_REQUIRE are made;
  2. the workspace sizes are the larger of the two directions' needs;
  3. the restatement of the loss tail (stencil_ref.loss_tail) agrees with the oracle in fp64;
  4. tie gate: on every loss case of the GPU file -- same shapes, same seeds, one shared table -- the op-for-op fp32 twin meets the
     bounds the GPU test applies to the kernels.  The inputs therefore hold no sign tie, and a kernel that computes what the twin
     computes passes.  A seed that fails here is replaced, never the bound."""
import ctypes

import numpy as np
import pytest

import df_oracle as orc
import stencil_ref as ref
from deep_fluids_amd import _lib

EINVAL, ESHAPE, EALIGN, EWORKSPACE = -1, -2, -3, -4
BIG = 1 << 30


@pytest.fixture(scope="module")
def h():
    return _lib.lib()


@pytest.fixture(scope="module")
def addr():
    """a 16-byte aligned host address (never dereferenced: every call below fails an argument check first)"""
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    yield a
    del buf


def expect(h, rc, code, text):
    msg = h.df_last_error().decode()
    assert rc == code, (rc, code, msg)
    assert text in msg, (text, msg)


# name -> (number of pointer arguments in front, index of the pointer check2 / check3 calls "input", required outputs, 3-D?)
STENCILS = {
    "df_curl2d_fwd": (2, 0, [1], False), "df_curl2d_bwd": (2, 0, [1], False), "df_divergence2d": (2, 0, [1], False),
    "df_divergence3d": (2, 0, [1], True),
    "df_jacobian2d_fwd": (3, 0, [], False), "df_jacobian2d_bwd": (3, 2, [], False),
    "df_jacobian3d_fwd": (3, 0, [], True), "df_jacobian3d_bwd": (3, 2, [], True),
}


def _call(h, name, ptrs, ext):
    return getattr(h, name)(*(list(ptrs) + list(ext) + [None]))


@pytest.mark.parametrize("name", sorted(STENCILS))
def test_stencil_argument_checks(h, addr, name):
    nptr, inp, outs, is_3d = STENCILS[name]
    good = (1, 2, 2, 2) if is_3d else (1, 2, 2)
    ptrs = [addr] * nptr
    nul = list(ptrs); nul[inp] = None
    expect(h, _call(h, name, nul, good), EINVAL, name + ": null input")
    for o in outs:
        nul = list(ptrs); nul[o] = None
        expect(h, _call(h, name, nul, good), EINVAL, name + ": null output")
    if not outs:      # the two optional pointers
        opt = [i for i in range(nptr) if i != inp]
        nul = list(ptrs)
        for i in opt:
            nul[i] = None
        expect(h, _call(h, name, nul, good), EINVAL, "both outputs null" if inp == 0 else "both incoming gradients null")
    for d in range(len(good)):
        e = list(good); e[d] = 0
        expect(h, _call(h, name, ptrs, e), EINVAL, name + ": non-positive extent")
        e[d] = -3
        expect(h, _call(h, name, ptrs, e), EINVAL, name + ": non-positive extent")
        if d > 0:
            e[d] = 1
            expect(h, _call(h, name, ptrs, e), ESHAPE, "every extent >= 2")
            for big in (BIG, BIG + 5):
                e[d] = big
                expect(h, _call(h, name, ptrs, e), ESHAPE, name + ": extent too large")


def test_stencil_alignment_contract(h, addr):
    """outputs written through vector types must be aligned to them (DF_EALIGN); a NULL optional output counts as aligned"""
    g3, g2 = (1, 2, 2, 2), (1, 2, 2)
    for off in (4, 8, 12):
        expect(h, _call(h, "df_jacobian3d_fwd", [addr, addr + off, addr], g3), EALIGN, "outputs must be 16-byte aligned")
        expect(h, _call(h, "df_jacobian3d_fwd", [addr, addr, addr + off], g3), EALIGN, "outputs must be 16-byte aligned")
        expect(h, _call(h, "df_jacobian3d_fwd", [addr, None, addr + off], g3), EALIGN, "outputs must be 16-byte aligned")
        expect(h, _call(h, "df_jacobian2d_fwd", [addr, addr + off, addr], g2), EALIGN, "j must be 16-byte aligned")
        expect(h, _call(h, "df_jacobian2d_fwd", [addr, addr + off, None], g2), EALIGN, "j must be 16-byte aligned")
    for off in (4, 12):
        expect(h, _call(h, "df_curl2d_fwd", [addr, addr + off], g2), EALIGN, "df_curl2d_fwd: u must be 8-byte aligned")
        expect(h, _call(h, "df_jacobian2d_bwd", [addr, addr, addr + off], g2), EALIGN, "df_jacobian2d_bwd: gx must be 8-byte aligned")
        expect(h, _call(h, "df_jacobian2d_bwd", [None, addr, addr + off], g2), EALIGN, "df_jacobian2d_bwd: gx must be 8-byte aligned")
    # the argument checks come first: a misaligned output with a bad extent reports the extent
    expect(h, _call(h, "df_curl2d_fwd", [addr, addr + 4], (1, 1, 2)), ESHAPE, ">= 2")


def _loss_call(h, name, ptrs, ext, ws, nbytes):
    return getattr(h, name)(*(list(ptrs) + list(ext) + [ws, nbytes, None]))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_loss_tail_argument_checks(h, addr, dim, direction):
    name = "df_velocity_loss%dd_%s" % (dim, direction)
    good = (2, 3, 4, 5)[4 - dim - 1:]
    n = int(np.prod(good))
    need = (-(-n // (ref.K_THREADS * ref.K_VPT3))) * 16 if direction == "fwd" else n * dim * 4
    full = getattr(h, "df_velocity_loss%dd_workspace_bytes" % dim)(*good)
    assert full >= need
    ptrs = [addr] * 5
    for i in (0, 1):
        nul = list(ptrs); nul[i] = None
        expect(h, _loss_call(h, name, nul, good, addr, full), EINVAL, name + ": null input")
    if direction == "fwd":
        for i in (3, 4):      # l1, jl1 (u, index 2, is optional)
            nul = list(ptrs); nul[i] = None
            expect(h, _loss_call(h, name, nul, good, addr, full), EINVAL, name + ": null output / workspace")
    else:
        nul = list(ptrs); nul[4] = None      # gpsi (g_l1, g_jl1, indices 2 and 3, are optional)
        expect(h, _loss_call(h, name, nul, good, addr, full), EINVAL, name + ": null output / workspace")
    expect(h, _loss_call(h, name, ptrs, good, None, full), EINVAL, name + ": null output / workspace")
    for d in range(len(good)):
        e = list(good); e[d] = 0
        expect(h, _loss_call(h, name, ptrs, e, addr, full), EINVAL, name + ": non-positive extent")
        if d > 0:
            e[d] = 1
            expect(h, _loss_call(h, name, ptrs, e, addr, full), ESHAPE, "every extent >= 2")
            for big in (BIG, BIG + 5):
                e[d] = big
                expect(h, _loss_call(h, name, ptrs, e, addr, 1 << 62), ESHAPE, name + ": extent too large")
    # B * Z * Y * X at 2^40 and above
    e = [1 << 22] + [1 << 9] * (len(good) - 1)
    e[0] = (1 << 40) // int(np.prod(e[1:]))
    expect(h, _loss_call(h, name, ptrs, e, addr, 1 << 62), ESHAPE, name + ": extent too large")
    expect(h, _loss_call(h, name, ptrs, good, addr, need - 1), EWORKSPACE, name + ": workspace too small")
    expect(h, _loss_call(h, name, ptrs, good, addr, 0), EWORKSPACE, name + ": workspace too small")
    if direction == "fwd":
        expect(h, _loss_call(h, name, ptrs, good, addr + 4, full), EALIGN, name + ": workspace must be 8-byte aligned")
    else:
        for off in (4, 8):
            expect(h, _loss_call(h, name, ptrs, good, addr + off, full), EALIGN, name + ": workspace must be 16-byte aligned")


def test_workspace_bytes_is_the_larger_need_and_zero_for_bad_extents(h):
    per = ref.K_THREADS * ref.K_VPT3
    for shape in [(1, 1, 1, 1), (1, 1, 1, 2), (1, 2, 2, 2), (2, 3, 4, 5), (1, 2, 8, 64), (16, 64, 96, 64)] + [s for s, _ in ref.LOSS3_CASES]:
        n = int(np.prod(shape))
        fwd, bwd = (-(-n // per)) * 16, n * 12
        assert h.df_velocity_loss3d_workspace_bytes(*shape) == max(fwd, bwd), shape
    assert h.df_velocity_loss3d_workspace_bytes(1, 1, 1, 1) == 16      # the forward's need is the larger one
    for shape in [(1, 1, 1), (1, 1, 2), (1, 1, 3), (2, 3, 5), (8, 128, 96)] + [s for s, _ in ref.LOSS2_CASES]:
        n = int(np.prod(shape))
        fwd, bwd = (-(-n // per)) * 16, n * 8
        assert h.df_velocity_loss2d_workspace_bytes(*shape) == max(fwd, bwd), shape
    assert h.df_velocity_loss2d_workspace_bytes(1, 1, 1) == 16
    for bad in (0, -1):
        for d in range(4):
            e = [2, 2, 2, 2]; e[d] = bad
            assert h.df_velocity_loss3d_workspace_bytes(*e) == 0
        for d in range(3):
            e = [2, 2, 2]; e[d] = bad
            assert h.df_velocity_loss2d_workspace_bytes(*e) == 0


def test_shape_table_reaches_the_branches_it_names():
    assert (ref.K_THREADS, ref.K_VOX_PER_BLOCK, ref.K_XCD_GROUP, ref.K_LDS_MAX_X, ref.K_VPT3) == (256, 1024, 48, 128, 4)
    blocks = lambda s: -(-int(np.prod(s)) // ref.K_VOX_PER_BLOCK)
    on, off = ref.JAC3_SHAPES[-2][0], ref.JAC3_SHAPES[-1][0]
    assert blocks(on) == 8 * ref.K_XCD_GROUP and blocks(off) == 8 * ref.K_XCD_GROUP + 1 and on[-1] % 4 == 0 and off[-1] % 4 == 0
    assert all(blocks(s) % (8 * ref.K_XCD_GROUP) for s, _ in ref.JAC3_SHAPES[:-2])
    for shape, path in ref.LOSS3_CASES:
        assert ref.expected_path(shape) == path, (shape, path)


@pytest.mark.parametrize("shape", [s for s, _ in ref.LOSS_CASES])
def test_loss_tail_restatement_agrees_with_the_oracle_in_fp64(shape):
    psi, x = ref.loss_inputs(shape)
    for w1, w2 in ref.LOSS_WEIGHTS:
        r = ref.loss_ref64(shape, w1, w2)
        l1, jl1, _, dpsi = ref.loss_tail(psi, x, w1, w2, ref.F64)
        assert abs(l1 - r["l1"]) <= 1e-13 * r["l1"] and abs(jl1 - r["j_l1"]) <= 1e-13 * r["j_l1"]
        assert np.abs(dpsi - r["dpsi"]).max() <= 1e-13 * np.abs(r["dpsi"]).max()
    # the fp32 twin's velocity is the stencil kernels' (the oracle in fp32, which the GPU tests compare bit for bit)
    np.testing.assert_array_equal(ref.loss_u32(shape), orc.curl3(psi) if len(shape) == 4 else orc.curl(psi))


@pytest.mark.parametrize("shape", [s for s, _ in ref.LOSS_CASES])
def test_tie_gate_fp32_twin_meets_the_gpu_bounds(shape):
    for w1, w2 in ref.LOSS_WEIGHTS:
        m = ref.twin_margins(shape, w1, w2)
        print("twin %-16s w=(%.1f, %.1f)  l1 %.3f  j_l1 %.3f  dpsi %.4f   (fractions of the bound)" % (shape, w1, w2, m["l1"], m["j_l1"], m["dpsi"]))
        assert m["l1"] <= 1.0 and m["j_l1"] <= 1.0 and m["dpsi"] <= 1.0, (shape, m)


def test_no_bit_exact_reference_holds_a_zero():
    """The GPU file compares the stencils bit for bit, which tells -0.0 from +0.0, while two correct kernels may differ in the sign of a
    zero (-(a) against 0 - a on a zero gradient channel).  No reference value of its cases is zero, so on these inputs bit equality
    and value equality are the same thing."""
    for shape, _ in ref.JAC3_SHAPES:
        assert all(int((v == 0).sum()) == 0 for v in ref.jac3_refs(shape).values()), shape
    for shape, _ in ref.ST2_SHAPES:
        psi, v, gu, gj, gw = ref.st2_inputs(shape)
        outs = [orc.curl(psi), orc.curl_bwd(gu), orc.divergence(v), orc.jacobian(v)[0], orc.jacobian(v)[1], orc.jacobian_bwd(gj),
                orc.jacobian_bwd(gj, gw), orc.jacobian_bwd(np.zeros_like(gj), gw)]
        assert all(int((o == 0).sum()) == 0 for o in outs), shape
    for shape, _ in ref.LOSS_CASES:
        assert int((ref.loss_u32(shape) == 0).sum()) == 0, shape
