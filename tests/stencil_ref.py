"""What tests/test_gpu_stencil_edges.py (GPU) and tests/test_stencils_host.py (host gate) share: the block geometry read from the
kernel sources, the shape tables derived from it, the seeded inputs, the fp64 references (oracle/df_oracle.py; computed once per case)
and the one restatement the oracle lacks -- the loss tail's backward pass written as csrc/velocity_loss.hip computes it (the
per-voxel du with the kernels' sgn and operation order, then the curl adjoint), in either precision.  In fp64 it must agree with
oracle.velocity_loss; in fp32 it is the op-for-op twin whose only use is to show that the seeded inputs hold no sign tie, i.e. that
the bounds of the GPU test can be met at all.

The forward stencils, both Jacobian adjoints, both curls and both divergences exist in the oracle and are used from there."""
import functools
import os
import re

import numpy as np

import df_oracle as orc

F32, F64 = np.float32, np.float64
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deep_fluids_amd", "csrc")


def _const(fname, name):
    src = open(os.path.join(_CSRC, fname)).read()
    m = re.search(r"constexpr\s+int\s+[^;]*?\b%s\s*=\s*(\d+)\s*[;,]" % name, src)
    assert m, "%s not found in %s" % (name, fname)
    return int(m.group(1))


K_THREADS = _const("stencil_common.hpp", "kThreads")                       # 256
K_VOX_PER_BLOCK = K_THREADS * _const("stencil_common.hpp", "kVoxPerThread")   # 1024 voxels per workgroup of the 3-D kernels
K_XCD_GROUP = _const("stencil_common.hpp", "kXcdGroup")                    # 48: the remap is on when blocks % (8 * 48) == 0
K_LDS_MAX_X = _const("stencil.hip", "kLdsMaxX")                            # 128: the LDS-staged adjoint up to this X
K_VPT3 = _const("velocity_loss.hip", "kVpt3")                              # 4: voxels per thread of the loss forward (its partials)
K_TILE_Z, K_TILE_Y = _const("velocity_loss.hip", "kTileZ"), _const("velocity_loss.hip", "kTileY")

# the smallest [1, Z, Y, X] with X % 4 == 0, X <= kLdsMaxX and exactly 8 * kXcdGroup workgroups: Z = 3 keeps one interior plane
_XCD_ROWS = 8 * K_XCD_GROUP * K_VOX_PER_BLOCK // (3 * K_LDS_MAX_X)
assert 3 * _XCD_ROWS * K_LDS_MAX_X == 8 * K_XCD_GROUP * K_VOX_PER_BLOCK

# ---- the shape table -------------------------------------------------------------------------------------------------------------------
# (B, Z, Y, X) of df_jacobian3d_fwd / _bwd, and the branch each one is there for
JAC3_SHAPES = [
    ((1, 2, 2, 2), "smallest legal extents; X % 4 != 0: one-voxel-per-lane kernels only"),
    ((1, 2, 2, 4), "smallest 16-byte case: four quads, every voxel on a far face"),
    ((2, 2, 3, 4), "two samples: a last-plane difference must not reach into the next sample"),
    ((1, 3, 5, 12), "ragged last block (180 voxels), interior plane and rows"),
    ((1, 2, 2, K_LDS_MAX_X), "X == kLdsMaxX: the LDS-staged adjoint for one incoming gradient"),
    ((1, 2, 2, K_LDS_MAX_X + 4), "X == kLdsMaxX + 4: the register adjoint"),
    ((2, 3, 4, 5), "X % 4 != 0 with two samples, an interior plane and interior rows"),
    ((1, 3, _XCD_ROWS, K_LDS_MAX_X), "exactly 8 * kXcdGroup workgroups: XCD remap on"),
    ((1, 3, _XCD_ROWS + 1, K_LDS_MAX_X), "one more row: one more workgroup, XCD remap off"),
]
# (B, Y, X) of the 2-D stencils: one pixel per thread, 256 pixels per workgroup
ST2_SHAPES = [
    ((1, 2, 2), "smallest legal extents"),
    ((2, 3, 5), "two samples, odd extents"),
    ((1, 2, K_THREADS // 2), "exactly one workgroup of 256 pixels"),
    ((1, 2, K_THREADS // 2 + 1), "one pixel more: a second, ragged workgroup"),
    ((1, 3, 1029), "long odd rows, several workgroups"),
]
DIV3_SHAPES = [(1, 2, 2, 2), (2, 2, 3, 4), (1, 3, 5, 12), (2, 3, 4, 5), (1, 2, 2, K_LDS_MAX_X + 1)]
# the loss tail: (shape, the forward path the aligned call with u takes)
LOSS3_CASES = [
    ((1, 2, 8, 64), "tile"), ((2, 2, 8, 112), "tile"), ((1, 2, 8, 128), "tile"), ((2, 4, 16, 64), "tile"),
    ((1, 3, 8, 64), "vec16"), ((1, 2, 3, 8), "vec16"),
    ((1, 2, 3, 5), "scalar"),
]
LOSS2_CASES = [((1, 2, 2), "scalar"), ((2, 3, 5), "scalar"), ((1, 2, 129), "scalar"), ((1, 3, 1029), "scalar")]
LOSS_CASES = LOSS3_CASES + LOSS2_CASES
LOSS_WEIGHTS = ((0.7, 1.3), (1.0, 1.0))      # the device-scalar case and the NULL == 1 case
# bounds of the loss tail (the figures tests/test_gpu_stencils.py uses; every case is below 100,000 voxels: the strict form)
LOSS_REL, LOSS_PATH_REL, DPSI_REL, DPSI_PATH_REL = 2e-6, 1e-6, 1e-5, 1e-6
assert all(int(np.prod(s)) < 100000 for s, _ in LOSS_CASES)


def tile_path_taken(shape):
    """the host conditions of df_velocity_loss3d_fwd for the persistent tile kernel, for an aligned call with u on a whole MI355X"""
    B, Z, Y, X = shape
    n = B * Z * Y * X
    nb = -(-n // (K_THREADS * K_VPT3))
    ntl = (Z // K_TILE_Z) * (Y // K_TILE_Y) * B
    return X in (64, 112, 128) and Z % K_TILE_Z == 0 and Y % K_TILE_Y == 0 and 0 < ntl <= nb


def expected_path(shape):
    if tile_path_taken(shape):
        return "tile"
    return "vec16" if shape[-1] % 4 == 0 else "scalar"


def _ro(a):
    a.setflags(write=False)
    return a


# ---- seeded inputs (read-only; shared) -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jac3_inputs(shape):
    rng = np.random.RandomState(sum(shape))
    return tuple(_ro(rng.uniform(-1, 1, shape + (c,)).astype(F32)) for c in (3, 9, 3))      # x, gj, gc


@functools.lru_cache(maxsize=None)
def jac3_refs(shape):
    x, gj, gc = jac3_inputs(shape)
    j, c = orc.jacobian3(x)
    return {"j": _ro(j), "c": _ro(c), "gj": _ro(orc.jacobian3_bwd(gj=gj)), "gc": _ro(orc.jacobian3_bwd(gc=gc)),
            "both": _ro(orc.jacobian3_bwd(gj, gc))}


@functools.lru_cache(maxsize=None)
def st2_inputs(shape):
    rng = np.random.RandomState(sum(shape))
    return tuple(_ro(rng.uniform(-1, 1, shape + (c,)).astype(F32)) for c in (1, 2, 2, 4, 1))   # psi, v, gu, gj, gw


@functools.lru_cache(maxsize=None)
def loss_inputs(shape):
    """as test_fused_velocity_loss_vs_oracle_and_unfused_path draws them"""
    is_3d = len(shape) == 4
    rng = np.random.RandomState(sum(shape) + 1)
    psi = rng.uniform(-1, 1, shape + (3 if is_3d else 1,)).astype(F32)
    x = rng.uniform(-1, 1, shape + (3 if is_3d else 2,)).astype(F32)
    return _ro(psi), _ro(x)


@functools.lru_cache(maxsize=None)
def loss_ref64(shape, w1, w2):
    psi, x = loss_inputs(shape)
    r = orc.velocity_loss(psi.astype(F64), x.astype(F64), len(shape) == 4, w1, w2)
    return {"l1": float(r["l1"]), "j_l1": float(r["j_l1"]), "dpsi": _ro(r["dpsi"])}


@functools.lru_cache(maxsize=None)
def loss_u32(shape):
    psi, _ = loss_inputs(shape)
    return _ro(orc.curl3(psi) if len(shape) == 4 else orc.curl(psi))


# ---- the loss tail as the kernels compute it -------------------------------------------------------------------------------------------
def _sgn(d):
    return np.sign(d).astype(d.dtype)      # 1, -1, 0 at 0 (either zero): the kernels' sgn


def loss_tail(psi, x, w1, w2, dtype):
    """(l1, j_l1, du, dpsi) of csrc/velocity_loss.hip in ``dtype``, op for op:
      u        = curl(psi)                                                     (same arithmetic as the stencil kernels)
      l1, j_l1 = per-voxel sums of |u - x| and |D u - D x| in ``dtype`` -- (|d0| + |d1|) + |d2|, the Jacobian terms axis by axis x, y, z
                 -- then summed in fp64 and scaled by 1 / (C n), 1 / (C D n)
      du       = sgn(u - x) * s1 + (adj_x + adj_y + adj_z),  adj = the adjoint of D applied to g = sgn(D u - D x) * s9, with
                 s1 = (1 / (C n)) * w1 and s9 = (1 / (C D n)) * w2 rounded to ``dtype`` factor by factor
      dpsi     = curl^T du."""
    psi = np.asarray(psi, dtype); x = np.asarray(x, dtype)
    is_3d = psi.ndim == 5
    u = orc.curl3(psi) if is_3d else orc.curl(psi)
    nvox = int(np.prod(psi.shape[:-1]))
    C = 3 if is_3d else 2
    axes = (3, 2, 1) if is_3d else (2, 1)                       # x, y(, z): the kernels' order
    a1 = np.abs(u[..., 0] - x[..., 0]) + np.abs(u[..., 1] - x[..., 1])
    if is_3d:
        a1 = a1 + np.abs(u[..., 2] - x[..., 2])
    aj = np.zeros(psi.shape[:-1], dtype)
    for ax in axes:
        for c in range(C):
            aj = aj + np.abs(orc.fdiff(u[..., c], ax) - orc.fdiff(x[..., c], ax))
    l1 = float(a1.astype(F64).sum() * (1.0 / (float(C) * nvox)))
    jl1 = float(aj.astype(F64).sum() * (1.0 / (float(C * len(axes)) * nvox)))
    if dtype is F32:
        l1, jl1 = float(F32(l1)), float(F32(jl1))               # the final kernel stores the fp64 mean as a float
    s1 = dtype(dtype(1.0) / dtype(C * nvox)) * dtype(w1)
    s9 = dtype(dtype(1.0) / dtype(C * len(axes) * nvox)) * dtype(w2)
    du = np.empty_like(u)
    for c in range(C):
        acc = None
        for ax in axes:
            g = _sgn(orc.fdiff(u[..., c], ax) - orc.fdiff(x[..., c], ax)) * s9
            a = orc.fdiff_adj(g, ax)
            acc = a if acc is None else acc + a
        du[..., c] = _sgn(u[..., c] - x[..., c]) * s1 + acc
    assert du.dtype == dtype
    dpsi = orc.jacobian3_bwd(gc=du) if is_3d else orc.curl_bwd(du)
    assert dpsi.dtype == dtype
    return l1, jl1, du, dpsi


def twin_margins(shape, w1, w2):
    """the fp32 twin against the fp64 oracle on the shared inputs of one loss case, in units of the GPU test's bounds (<= 1 passes)"""
    psi, x = loss_inputs(shape)
    ref = loss_ref64(shape, w1, w2)
    l1, jl1, _, dpsi = loss_tail(psi, x, w1, w2, F32)
    scale = float(np.abs(ref["dpsi"]).max())
    return {"l1": abs(l1 - ref["l1"]) / (LOSS_REL * ref["l1"]), "j_l1": abs(jl1 - ref["j_l1"]) / (LOSS_REL * ref["j_l1"]),
            "dpsi": float(np.abs(dpsi.astype(F64) - ref["dpsi"]).max()) / (DPSI_REL * scale)}
