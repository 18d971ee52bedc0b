"""-m gpu: the entry points of csrc/stencil.hip and csrc/velocity_loss.hip called through the raw C ABI at the edges where their host
code switches kernels -- X % 4, the 16-byte alignment of each operand, X <= kLdsMaxX, NULL optional pointers, the tile conditions of the
loss forward, the block count that turns the XCD remap on -- which the tests through deep_fluids_amd.ops (fresh, exact-size, 256-byte
aligned tensors) cannot reach.

Shapes (tests/stencil_ref.py derives them from kThreads = 256, kVoxPerBlock = 1024, kLdsMaxX = 128, kXcdGroup = 48, read from the sources):

  df_jacobian3d_fwd / _bwd  (B, Z, Y, X)
    (1, 2, 2, 2)        smallest legal extents; X % 4 != 0: the one-voxel-per-lane kernels
    (1, 2, 2, 4)        smallest 16-byte case, every voxel on a far face
    (2, 2, 3, 4)        two samples: a last-plane difference leaking into the next sample
    (1, 3, 5, 12)       ragged last block, interior plane and rows
    (1, 2, 2, 128)      X == kLdsMaxX: LDS-staged adjoint (one incoming gradient)
    (1, 2, 2, 132)      X == kLdsMaxX + 4: register adjoint
    (2, 3, 4, 5)        X % 4 != 0, two samples, interior plane
    (1, 3, 1024, 128)   384 = 8 * kXcdGroup workgroups: XCD remap on
    (1, 3, 1025, 128)   385 workgroups: XCD remap off
  2-D stencils  (B, Y, X):  (1, 2, 2), (2, 3, 5), (1, 2, 128) one workgroup of 256 pixels, (1, 2, 129) one pixel more, (1, 3, 1029)
  df_velocity_loss3d  (B, Z, Y, X):  tile kernel (1, 2, 8, 64), (2, 2, 8, 112), (1, 2, 8, 128), (2, 4, 16, 64);  curl3 + 16-byte
    reduction (1, 3, 8, 64), (1, 2, 3, 8);  one-kernel scalar form (1, 2, 3, 5), and every shape again with psi offset, x offset,
    u offset and u == NULL, which all take the scalar form
  df_velocity_loss2d  (B, Y, X):  (1, 2, 2), (2, 3, 5), (1, 2, 129), (1, 3, 1029)

Harness: every device buffer is a named gpu_util.Guarded object that lives until the result has been read; every output and the
workspace lie between two guard zones in an allocation pre-filled with one NaN bit pattern.  "Offset" = the operand starts one float
into its zone: 4-byte aligned, not 8-byte aligned.  After every call: return code 0, both guard zones bit-identical to the fill, no NaN
left in the output, and the values -- the stencils bit for bit against oracle/df_oracle.py, the loss tail within the bounds of
tests/test_gpu_stencils.py (stencil_ref.LOSS_REL etc.; the host gate shows that the op-for-op fp32 twin meets them on these inputs).
Only alignments that include/deepfluids_hip.h promises to handle are launched; the ones it promises to reject are checked to return
DF_EALIGN and to leave the buffer untouched."""
import numpy as np
import pytest
import torch

import df_oracle as orc
import stencil_ref as ref
from gpu_util import Guarded, assert_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
EALIGN = -3


@pytest.fixture(scope="module")
def k():
    """(library handle, stream)"""
    from deep_fluids_amd import _lib
    from deep_fluids_amd.ops import _stream
    return _lib.lib(), _stream()


def P(b):
    return None if b is None else b.ptr


def run(k, name, *args):
    h, s = k
    rc = getattr(h, name)(*(list(args) + [s]))
    assert rc == 0, "%s returned %d: %s" % (name, rc, h.df_last_error().decode())
    torch.cuda.synchronize()


def rejected(k, name, out, *args):
    """the call must return DF_EALIGN and must not have touched ``out``"""
    h, s = k
    rc = getattr(h, name)(*(list(args) + [s]))
    torch.cuda.synchronize()
    assert rc == EALIGN, "%s returned %d, not DF_EALIGN" % (name, rc)
    assert out.untouched(), "%s wrote into a buffer it rejected" % name


def ids(cases):
    return ["x".join(str(e) for e in (c[0] if isinstance(c[0], tuple) else c)) for c in cases]


# ---- df_jacobian3d_fwd / _bwd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, _ in ref.JAC3_SHAPES], ids=ids(ref.JAC3_SHAPES))
def test_jacobian3d_fwd_outputs_and_input_alignment(k, shape):
    x = ref.jac3_inputs(shape)[0]
    want = ref.jac3_refs(shape)
    for xoff in ((0, 1) if shape[-1] % 4 == 0 else (0,)):          # offset x: the one-voxel-per-lane kernel instead of the 16-byte one
        X = Guarded(x.shape, x, offset=xoff)
        for wj, wc in ((True, True), (True, False), (False, True)):
            what = "jacobian3d_fwd %s x+%d j=%d c=%d" % (shape, xoff, wj, wc)
            J = Guarded(shape + (9,)) if wj else None
            C = Guarded(shape + (3,)) if wc else None
            run(k, "df_jacobian3d_fwd", X.ptr, P(J), P(C), *shape)
            if wj:
                assert_bits(J.get(what), want["j"], what + " j")
            if wc:
                assert_bits(C.get(what), want["c"], what + " c")
        X.check_guards("x")


@pytest.mark.parametrize("shape", [s for s, _ in ref.JAC3_SHAPES], ids=ids(ref.JAC3_SHAPES))
def test_jacobian3d_bwd_gradients_and_each_operand_offset(k, shape):
    _, gj, gc = ref.jac3_inputs(shape)
    want = ref.jac3_refs(shape)
    for hj, hc in ((True, False), (False, True), (True, True)):
        for off in (None, "gj", "gc", "gx"):                       # exactly one operand offset: all of them take the scalar adjoint
            if (off == "gj" and not hj) or (off == "gc" and not hc):
                continue
            what = "jacobian3d_bwd %s gj=%d gc=%d offset=%s" % (shape, hj, hc, off)
            GJ = Guarded(gj.shape, gj, offset=int(off == "gj")) if hj else None
            GC = Guarded(gc.shape, gc, offset=int(off == "gc")) if hc else None
            GX = Guarded(shape + (3,), offset=int(off == "gx"))
            run(k, "df_jacobian3d_bwd", P(GJ), P(GC), GX.ptr, *shape)
            assert_bits(GX.get(what), want["both" if hj and hc else "gj" if hj else "gc"], what)


def test_jacobian3d_fwd_rejects_a_misaligned_output(k):
    shape = (1, 2, 2, 4)
    X = Guarded(shape + (3,), ref.jac3_inputs(shape)[0])
    J, C = Guarded(shape + (9,), offset=1), Guarded(shape + (3,), offset=1)
    J0, C0 = Guarded(shape + (9,)), Guarded(shape + (3,))
    rejected(k, "df_jacobian3d_fwd", J, X.ptr, J.ptr, C0.ptr, *shape)
    rejected(k, "df_jacobian3d_fwd", C, X.ptr, J0.ptr, C.ptr, *shape)
    assert J0.untouched() and C0.untouched()


@pytest.mark.parametrize("shape", ref.DIV3_SHAPES, ids=ids(ref.DIV3_SHAPES))
def test_divergence3d(k, shape):
    rng = np.random.RandomState(sum(shape) + 7)
    x = rng.uniform(-1, 1, shape + (3,)).astype(F32)
    want = orc.divergence3(x)
    for xoff, doff in ((0, 0), (1, 0), (0, 1), (1, 1)):
        what = "divergence3d %s x+%d d+%d" % (shape, xoff, doff)
        X = Guarded(x.shape, x, offset=xoff)
        D = Guarded(want.shape, offset=doff)
        run(k, "df_divergence3d", X.ptr, D.ptr, *shape)
        assert_bits(D.get(what), want, what)


# ---- 2-D stencils ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, _ in ref.ST2_SHAPES], ids=ids(ref.ST2_SHAPES))
def test_curl2d_and_divergence2d(k, shape):
    psi, v, gu, _, _ = ref.st2_inputs(shape)
    for ioff in (0, 1):
        what = "curl2d_fwd %s psi+%d" % (shape, ioff)
        PSI = Guarded(psi.shape, psi, offset=ioff)
        U = Guarded(shape + (2,))
        run(k, "df_curl2d_fwd", PSI.ptr, U.ptr, *shape)
        assert_bits(U.get(what), orc.curl(psi), what)
        for ooff in (0, 1):
            what = "curl2d_bwd %s gu+%d gpsi+%d" % (shape, ioff, ooff)
            GU = Guarded(gu.shape, gu, offset=ioff)
            GP = Guarded(shape + (1,), offset=ooff)
            run(k, "df_curl2d_bwd", GU.ptr, GP.ptr, *shape)
            assert_bits(GP.get(what), orc.curl_bwd(gu), what)
            what = "divergence2d %s x+%d d+%d" % (shape, ioff, ooff)
            V = Guarded(v.shape, v, offset=ioff)
            want = orc.divergence(v)
            D = Guarded(want.shape, offset=ooff)
            run(k, "df_divergence2d", V.ptr, D.ptr, *shape)
            assert_bits(D.get(what), want, what)
    # u is written as 8-byte records: a 4-byte aligned u is rejected, before any launch
    PSI = Guarded(psi.shape, psi)
    U = Guarded(shape + (2,), offset=1)
    rejected(k, "df_curl2d_fwd", U, PSI.ptr, U.ptr, *shape)


@pytest.mark.parametrize("shape", [s for s, _ in ref.ST2_SHAPES], ids=ids(ref.ST2_SHAPES))
def test_jacobian2d_fwd_bwd(k, shape):
    _, v, _, gj, gw = ref.st2_inputs(shape)
    oj, ow = orc.jacobian(v)
    for xoff in (0, 1):                                            # offset x: 4-byte loads instead of 8-byte records
        V = Guarded(v.shape, v, offset=xoff)
        for wj, ww, woff in ((True, True, 0), (True, True, 1), (True, False, 0), (False, True, 0), (False, True, 1)):
            what = "jacobian2d_fwd %s x+%d j=%d w=%d w+%d" % (shape, xoff, wj, ww, woff)
            J = Guarded(shape + (4,)) if wj else None
            W = Guarded(shape + (1,), offset=woff) if ww else None
            run(k, "df_jacobian2d_fwd", V.ptr, P(J), P(W), *shape)
            if wj:
                assert_bits(J.get(what), oj, what + " j")
            if ww:
                assert_bits(W.get(what), ow, what + " w")
    want = {(True, False): orc.jacobian_bwd(gj), (True, True): orc.jacobian_bwd(gj, gw), (False, True): orc.jacobian_bwd(np.zeros_like(gj), gw)}
    for hj, hw in ((True, False), (False, True), (True, True)):
        for off in (None, "gj", "gw"):
            if (off == "gj" and not hj) or (off == "gw" and not hw):
                continue
            what = "jacobian2d_bwd %s gj=%d gw=%d offset=%s" % (shape, hj, hw, off)
            GJ = Guarded(gj.shape, gj, offset=int(off == "gj")) if hj else None
            GW = Guarded(gw.shape, gw, offset=int(off == "gw")) if hw else None
            GX = Guarded(shape + (2,))
            run(k, "df_jacobian2d_bwd", P(GJ), P(GW), GX.ptr, *shape)
            assert_bits(GX.get(what), want[(hj, hw)], what)
    # j is written as 16-byte records and gx as 8-byte records: rejected when they are only 4-byte aligned
    V, GJ = Guarded(v.shape, v), Guarded(gj.shape, gj)
    J, W, GX = Guarded(shape + (4,), offset=1), Guarded(shape + (1,)), Guarded(shape + (2,), offset=1)
    rejected(k, "df_jacobian2d_fwd", J, V.ptr, J.ptr, W.ptr, *shape)
    assert W.untouched()
    rejected(k, "df_jacobian2d_bwd", GX, GJ.ptr, None, GX.ptr, *shape)


# ---- the loss tail -----------------------------------------------------------------------------------------------------------------------
class Loss(object):
    """one loss case: the shared inputs, ONE guarded workspace of exactly df_velocity_loss*_workspace_bytes for every call of both
    directions, refilled with NaN before each of them"""

    def __init__(self, k, shape):
        self.k, self.shape = k, tuple(shape)
        self.is_3d = len(shape) == 4
        self.dim = 3 if self.is_3d else 2
        self.psi, self.x = ref.loss_inputs(self.shape)
        self.u_ref = ref.loss_u32(self.shape)
        self.nbytes = int(getattr(k[0], "df_velocity_loss%dd_workspace_bytes" % self.dim)(*self.shape))
        assert self.nbytes > 0 and self.nbytes % 4 == 0
        self.ws = Guarded((self.nbytes // 4,))

    def fwd(self, what, psi_off=0, x_off=0, u_off=0, with_u=True):
        PSI = Guarded(self.psi.shape, self.psi, offset=psi_off)
        X = Guarded(self.x.shape, self.x, offset=x_off)
        U = Guarded(self.u_ref.shape, offset=u_off) if with_u else None
        L1, JL1 = Guarded((1,)), Guarded((1,))
        self.ws.refill()
        run(self.k, "df_velocity_loss%dd_fwd" % self.dim, PSI.ptr, X.ptr, P(U), L1.ptr, JL1.ptr, *(self.shape + (self.ws.ptr, self.nbytes)))
        self.ws.check_guards(what + " workspace")
        PSI.check_guards(what + " psi"); X.check_guards(what + " x")
        l1, jl1 = float(L1.get(what + " l1")[0]), float(JL1.get(what + " jl1")[0])
        if with_u:
            assert_bits(U.get(what + " u"), self.u_ref, what + " u against the oracle")
        return l1, jl1

    def bwd(self, what, u_off=0, x_off=0, g_off=0, scalars=None):
        U = Guarded(self.u_ref.shape, self.u_ref, offset=u_off)
        X = Guarded(self.x.shape, self.x, offset=x_off)
        G1 = Guarded((1,), [scalars[0]]) if scalars else None
        G2 = Guarded((1,), [scalars[1]]) if scalars else None
        GP = Guarded(self.psi.shape, offset=g_off)
        self.ws.refill()
        run(self.k, "df_velocity_loss%dd_bwd" % self.dim, U.ptr, X.ptr, P(G1), P(G2), GP.ptr, *(self.shape + (self.ws.ptr, self.nbytes)))
        self.ws.check_guards(what + " workspace")
        return GP.get(what + " gpsi")


def _loss_programme(k, shape, path):
    c = Loss(k, shape)
    tag = "velocity_loss%dd %s" % (c.dim, shape)
    # ---- forward: every path of this shape ----
    fw = {"aligned [%s]" % path: c.fwd(tag + " aligned")}
    fw["psi offset [scalar]"] = c.fwd(tag + " psi offset", psi_off=1)
    fw["x offset [scalar]"] = c.fwd(tag + " x offset", x_off=1)
    fw["u offset [scalar]"] = c.fwd(tag + " u offset", u_off=1)
    fw["u NULL [scalar]"] = c.fwd(tag + " u NULL", with_u=False)
    r = ref.loss_ref64(c.shape, 1.0, 1.0)
    for name, (l1, jl1) in fw.items():
        print("%s fwd %-22s l1 %.9g (rel err %.2e)  jl1 %.9g (rel err %.2e)" % (tag, name, l1, abs(l1 - r["l1"]) / r["l1"], jl1,
                                                                              abs(jl1 - r["j_l1"]) / r["j_l1"]))
    for name, (l1, jl1) in fw.items():
        assert abs(l1 - r["l1"]) <= ref.LOSS_REL * r["l1"] and abs(jl1 - r["j_l1"]) <= ref.LOSS_REL * r["j_l1"], (tag, name, l1, jl1, r["l1"], r["j_l1"])
    for na, (a1, a9) in fw.items():
        for nb, (b1, b9) in fw.items():
            assert abs(a1 - b1) <= ref.LOSS_PATH_REL * abs(b1) and abs(a9 - b9) <= ref.LOSS_PATH_REL * abs(b9), (tag, na, nb, a1, b1, a9, b9)
    if c.is_3d:      # u of the loss forward == df_jacobian3d_fwd(psi, NULL, u) | df_curl2d_fwd bit for bit (both equal the oracle; here directly)
        PSI, C = Guarded(c.psi.shape, c.psi), Guarded(c.u_ref.shape)
        run(k, "df_jacobian3d_fwd", PSI.ptr, None, C.ptr, *c.shape)
    else:
        PSI, C = Guarded(c.psi.shape, c.psi), Guarded(c.u_ref.shape)
        run(k, "df_curl2d_fwd", PSI.ptr, C.ptr, *c.shape)
    assert_bits(C.get(tag + " stencil u"), c.u_ref, tag + " stencil u")
    # ---- backward ----
    w = ref.LOSS_WEIGHTS[0]
    bw = {"aligned": c.bwd(tag + " bwd aligned", scalars=w), "u offset": c.bwd(tag + " bwd u offset", u_off=1, scalars=w),
          "x offset": c.bwd(tag + " bwd x offset", x_off=1, scalars=w), "gpsi offset": c.bwd(tag + " bwd gpsi offset", g_off=1, scalars=w)}
    rw = ref.loss_ref64(c.shape, *w)["dpsi"]
    scale = float(np.abs(rw).max())
    for name, g in bw.items():
        err = float(np.abs(g.astype(np.float64) - rw).max())
        print("%s bwd %-12s w=%s max err %.3e = %.4f of the bound" % (tag, name, w, err, err / (ref.DPSI_REL * scale)))
    for name, g in bw.items():
        assert float(np.abs(g.astype(np.float64) - rw).max()) <= ref.DPSI_REL * scale, (tag, name)
        assert float(np.abs(g.astype(np.float64) - bw["aligned"].astype(np.float64)).max()) <= ref.DPSI_PATH_REL * scale, (tag, name)
    g_null = c.bwd(tag + " bwd NULL scalars")
    g_one = c.bwd(tag + " bwd scalars 1.0", scalars=(1.0, 1.0))
    assert_bits(g_null, g_one, tag + ": g_l1 = g_jl1 = NULL against device scalars 1.0")
    r1 = r["dpsi"]
    err = float(np.abs(g_null.astype(np.float64) - r1).max())
    print("%s bwd NULL scalars max err %.3e = %.4f of the bound" % (tag, err, err / (ref.DPSI_REL * float(np.abs(r1).max()))))
    assert err <= ref.DPSI_REL * float(np.abs(r1).max()), tag
    if c.is_3d and c.shape[-1] % 4 == 0:      # the scalar adjoint chain (u offset, gpsi offset) against the 16-byte one under NULL scalars too
        g_s = c.bwd(tag + " bwd NULL scalars, u and gpsi offset", u_off=1, g_off=1)
        assert float(np.abs(g_s.astype(np.float64) - g_null.astype(np.float64)).max()) <= ref.DPSI_PATH_REL * float(np.abs(r1).max()), tag


@pytest.mark.parametrize("shape,path", ref.LOSS3_CASES, ids=ids(ref.LOSS3_CASES))
def test_velocity_loss3d_every_path_on_one_guarded_workspace(k, shape, path):
    _loss_programme(k, shape, path)


@pytest.mark.parametrize("shape,path", ref.LOSS2_CASES, ids=ids(ref.LOSS2_CASES))
def test_velocity_loss2d_every_path_on_one_guarded_workspace(k, shape, path):
    _loss_programme(k, shape, path)
