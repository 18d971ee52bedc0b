"""Drop-in counterpart of the reference's ``ops.py`` call surface on MI355X.

Same function names, argument order, defaults, return-tuple structure and channels-last layouts
as ``byungsook/deep-fluids/ops.py`` (cited per function), operating on ``torch`` CUDA(=HIP) tensors.
Every bit of arithmetic is done by hand-written gfx950 kernels in ``libdeepfluids_hip.so`` reached
through the C-ABI of ``include/deepfluids_hip.h`` (ctypes, PyTorch's current HIP stream);  PyTorch
supplies device memory, streams and autograd bookkeeping only.  There is no CPU / eager fallback:
a missing library or a non-GPU tensor raises.

TF-1 style hidden state (``slim`` variables inside ``tf.variable_scope``) is reproduced by a
name-keyed registry: ``variable_scope(name, reuse)`` + ``get_variables(scope)``; variable names
follow slim: ``<scope>/<layer>/weights`` ``[k,(k,)k,Cin,Cout]`` / ``[in,out]`` and ``.../biases``.
"""
import collections
import contextlib
import ctypes
import math
import numbers
import os as _os
import threading as _threading

import numpy as np
import torch

from . import _lib
from ._lib import call, query, DF_CONV_BIAS, DF_CONV_LRELU, DF_CONV_MASK, DF_CONV_RESIDUAL  # noqa: F401

__all__ = [
    "lrelu", "conv2d", "conv3d", "linear", "upscale", "upscale3", "resize_nearest_neighbor", "reshape",
    "int_shape", "get_conv_shape", "nchw_to_nhwc", "nhwc_to_nchw", "add", "concat", "sigmoid", "mse_mean",
    "jacobian", "jacobian3", "curl", "curl3", "divergence", "divergence3", "pgrad",
    "vort_np", "curl_np", "grad_np", "jacobian_np3", "l1_mean", "velocity_loss", "field_metrics", "field_metrics_workspace", "FieldMetrics",
    "fspecial_gauss", "ssim", "ms_ssim", "field_ssim", "ssim_workspace", "SSIMWorkspace",
    "denorm_img", "plane_view", "denorm_img3", "plane_view_np", "velocity_views3", "add_channels", "remove_channels",
    "advect", "advect_sequence", "advect_workspace", "density_image", "sphere_mask",
    "advect_velocity", "wall_buoyancy", "solve_pressure", "pressure_workspace", "smoke_step", "simulate_smoke", "default_buoyancy_force", "default_max_iter", "obstacle_flags", "ObstacleFlags",
    "open_sides", "SphereSource",
    "advect_particles", "particle_cells", "particle_levelset", "particle_levelset_averaged", "liquid_sequence", "seed_particles", "box_levelset", "sphere_levelset",
    "pack_particles", "unpack_particles", "extrapolate_levelset", "resample_particles", "Resample",
    "nn_bn_elu_dropout", "nn_window_advance", "nn_window_stack", "nn_mse", "nn_rollout", "nn_mask_state", "batch_norm_variables",
    "variable_scope", "get_variables", "get_variable", "reset_variables", "set_random_seed", "all_variables",
]


# --------------------------------------------------------------------------------------------------
# plumbing
# --------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _prep(t, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor on the MI355X (got %r)" % (name, type(t)))
    if not t.is_cuda:
        raise _lib.DeepFluidsHipError("%s is on %s: deep_fluids_amd has no CPU path (HIP kernels only)" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (the reference is fp32 end-to-end), got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _empty(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# --------------------------------------------------------------------------------------------------
# variable registry (tf.variable_scope / slim variables)
# --------------------------------------------------------------------------------------------------
_VARS = {}            # full name -> torch.Tensor (requires_grad leaf)
_UNNAMED = {}         # (scope prefix, layer kind) -> how many unnamed layers of that kind were created in this scope entry
_SCOPES = []          # stack of (name, reuse)
_RNG = np.random.RandomState(123)     # main.py:12 tf.set_random_seed(123) / config.py:69
_DEFAULT_DEVICE = "cuda"


class VariableScope(object):
    def __init__(self, name):
        self.name = name


def set_random_seed(seed):
    global _RNG
    _RNG = np.random.RandomState(seed)


def reset_variables():
    _VARS.clear()
    _DIRECT_GRADS.clear()


# Direct gradient targets: data_ptr of a variable -> the tensor its gradient kernel writes (the variable's slice of a trainer's flat gradient slab).
# A backward node then hands the weight / bias gradient kernels that slice as their OUTPUT and returns None for the input, instead of allocating a
# tensor that autograd's AccumulateGrad adds to the (zeroed) slab in a second launch: 42 launches and passes per 2-D step saved.  Valid only where
# every registered variable receives exactly ONE gradient per backward pass and nobody listens for post-accumulate hooks -- the single-process
# `de` / `ae` trainers register theirs (Trainer._build_variables); data parallelism and the GAN trainer (D is applied twice) do not.
_DIRECT_GRADS = {}


def _grad_out(ptr, shape, device):
    """-> (tensor the gradient kernel writes, what backward returns for that input)."""
    g = _DIRECT_GRADS.get(ptr)
    if g is not None:
        return g, None
    t = torch.empty(shape, dtype=torch.float32, device=device)
    return t, t


def all_variables():
    return dict(_VARS)


@contextlib.contextmanager
def variable_scope(name, reuse=False):
    inherited = bool(_SCOPES and _SCOPES[-1][1])
    _SCOPES.append((name, bool(reuse) or inherited))
    prefix = "/".join(s[0] for s in _SCOPES)
    for key in [k for k in _UNNAMED if k[0] == prefix]:      # slim's default layer names (Conv, Conv_1, ...) restart on
        del _UNNAMED[key]                                     # every entry of the scope, so reuse=True finds the same names
    try:
        yield VariableScope("/".join(s[0] for s in _SCOPES))
    finally:
        _SCOPES.pop()


def _scope_prefix():
    return "/".join(s[0] for s in _SCOPES)


def _reusing():
    return bool(_SCOPES and _SCOPES[-1][1])


def get_variable(name, shape, init="xavier", device=None):
    """slim model variable: Xavier-uniform weights / zero biases, created on first use,
    returned as-is under ``reuse=True`` (trainer.py:299-300 builds the test model that way)."""
    full = (_scope_prefix() + "/" if _SCOPES else "") + name
    if full in _VARS:
        if not _reusing():
            raise ValueError("Variable %s already exists; did you mean reuse=True?" % full)
        v = _VARS[full]
        if tuple(v.shape) != tuple(shape):
            raise ValueError("Variable %s has shape %s, requested %s" % (full, tuple(v.shape), tuple(shape)))
        return v
    if _reusing():
        raise ValueError("Variable %s does not exist (reuse=True)" % full)
    if init == "xavier":
        rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        lim = math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
        host = _RNG.uniform(-lim, lim, size=shape).astype(np.float32)
    elif init == "ones":
        host = np.ones(shape, np.float32)
    else:
        host = np.zeros(shape, np.float32)
    v = torch.from_numpy(host).to(device or _DEFAULT_DEVICE).requires_grad_(True)
    _VARS[full] = v
    return v


def set_variable(full_name, value):
    """Inject a variable by its full slim name (parity tests / checkpoint restore)."""
    t = torch.as_tensor(np.asarray(value, np.float32)).to(_DEFAULT_DEVICE).contiguous().requires_grad_(True)
    _VARS[full_name] = t
    return t


def get_variables(scope):
    """tf.contrib.framework.get_variables(vs): variables under a scope, creation order."""
    prefix = (scope.name if isinstance(scope, VariableScope) else str(scope)) + "/"
    return [v for k, v in _VARS.items() if k.startswith(prefix)]


def _layer_name(name, kind):
    if name is not None:
        return name
    key = (_scope_prefix(), kind)
    n = _UNNAMED.get(key, 0)
    _UNNAMED[key] = n + 1
    return kind if n == 0 else "%s_%d" % (kind, n)


# --------------------------------------------------------------------------------------------------
# autograd bindings of the HIP kernels
# --------------------------------------------------------------------------------------------------
class _Lrelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, leak):
        x = _prep(x, "x")
        y = torch.empty_like(x)
        call("df_lrelu_fwd", _ptr(x), _ptr(y), float(leak), x.numel(), _stream())
        ctx.save_for_backward(y)
        ctx.leak = float(leak)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = _prep(gy, "grad")
        gx = torch.empty_like(gy)
        call("df_lrelu_bwd", _ptr(gy), _ptr(y), _ptr(gx), ctx.leak, gy.numel(), _stream())
        return gx, None


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = _prep(a, "a"); b = _prep(b, "b")
        if a.shape != b.shape:
            raise ValueError("add: shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        y = torch.empty_like(a)
        call("df_add", _ptr(a), _ptr(b), _ptr(y), a.numel(), _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return g, g


# Convolution precision of the 128->128-class layers (forward and dgrad):
#   "fp32"   exact fp32 MFMA (v_mfma_f32_32x32x2_f32) -- the default, what the reference computes and bench.py reports;
#   "bf16x3" opt-in: operands split into bf16 hi/lo words, 3 bf16 MFMAs per product block (16 significand bits per
#            operand, fp32 accumulate): ~5x the matrix rate, velocity-field error ~1e-5 (tolerance 1e-4).
CONV_PRECISION = "fp32"


def _sfx(cin, cout):
    """'_bf16x3' when that mode is on and the layer is wide enough for it (thin layers stay on the fp32 VALU kernels)."""
    # (symmetric in cin / cout: the dgrad runs the same layer with the two swapped and must agree with the packed format)
    return "_bf16x3" if (CONV_PRECISION == "bf16x3" and cin >= 16 and cout >= 16 and cin % 4 == 0 and cout % 4 == 0) else ""


# Algorithm of the wide 3-D stride-1 convs (forward and dgrad), fp32 mode only:
#   "auto"     Winograd F(2x2x2,3x3x3) / F(2x2,3x3) (conv_wino.hip / conv_wino2d.hip: same fp32 arithmetic, 3.4x / 2.25x fewer
#              matrix FLOPs) where it applies (Cin and Cout multiples of 32; 3-D extents >= 6, 2-D extents >= 16 x 24) and the direct
#              implicit-GEMM kernel everywhere else;
#   "direct"   always the direct kernel;   "winograd"  Winograd wherever the channel counts allow (tests).
CONV_ALGO = "auto"


# Weight-gradient algorithm request handed to df_conv_wgrad_algo / df_upconv_wgrad_algo (a call argument of the C-ABI, not a
# library global): 0 best available (what df_conv_wgrad does), 1 direct kernels only, 2 at most Winograd in x, 3 Winograd in
# (x,y), 4 Winograd in (x,y,z) wherever instantiated.  Tests pin the variants against each other and the oracle.
WGRAD_ALGO = 0
# True: thin layers (Cin or Cout <= 4) take the general-shape vector-ALU kernels (DF_CONV_VALU_ONLY) instead of the
# matrix-core forms -- the two are compared in the tests.
THIN_VALU_ONLY = False


# Which algorithm every conv / weight-gradient call took, counted per (op, form, shape) when set to a dict (bench.py `dispatch`, tests):
# the library chooses by size and row length, and a shape outside the instantiated variants falls back to a slower kernel SILENTLY --
# this makes it visible.  None (default) = no bookkeeping.
DISPATCH_COUNTS = None
_WGRAD_FORMS = {0: "direct-mfma", 1: "winograd-x", 2: "winograd-xy", 3: "winograd-xyz", 10: "thin-mfma", 11: "thin-valu"}


def _count(op, form, dims, cin, cout):
    if DISPATCH_COUNTS is not None:
        key = "%s %s %s C%d->%d" % (op, form, "x".join(str(int(d)) for d in dims[1:] if int(d) > 1 or len(dims) < 4), cin, cout)
        DISPATCH_COUNTS[key] = DISPATCH_COUNTS.get(key, 0) + 1


def _wgrad(x, dp, gw, gb, B, D, H, W, cin, cout, kz, sfx=""):
    if DISPATCH_COUNTS is not None:
        fid = query("df_conv_wgrad_form", B, D, H, W, cin, cout, kz, int(WGRAD_ALGO))
        # (bf16x3 mode: the library keeps the fp32 (x,y,z) Winograd form where it exists -- it is faster than the split-operand kernel)
        form = "bf16x3" if (sfx and fid != 3) else _WGRAD_FORMS.get(fid, "?")
        _count("wgrad", form, (B, D, H, W), cin, cout)
    nbytes = query("df_conv_wgrad_workspace_bytes", B, D, H, W, cin, cout, kz)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    if sfx:
        call("df_conv_wgrad" + sfx, _ptr(x), _ptr(dp), _ptr(gw), _ptr(gb), B, D, H, W, cin, cout, kz, _ptr(ws), nbytes, _stream())
    else:
        call("df_conv_wgrad_algo", _ptr(x), _ptr(dp), _ptr(gw), _ptr(gb), B, D, H, W, cin, cout, kz, _ptr(ws), nbytes,
             int(WGRAD_ALGO), _stream())


# Levels whose kernels cannot fill the chip (B x voxels x taps <= this) run the weight gradient of a layer on a SECOND stream, concurrently
# with the same layer's dgrad: both only read the incoming gradient and each launches few workgroups with a long serial chain (the
# low-resolution levels, and every level of the 2-D net at the reference's default batch 8).  Same kernels, same arguments: results are
# bitwise those of the serial order.  0 = always serial.  Measured (profiles/r06_probes.md section 1): 2-D 128x96 B = 8 4.95 -> 4.46 ms;
# above ~1M the two kernels each fill the chip and only contend (cfg3's 16x24x16 level at B = 16: +1.7 % on the step).
CONCURRENT_WGRAD_WORK = int(_os.environ.get("DF_CONCURRENT_WGRAD_WORK", str(1 << 20)))
_SIDE_STREAMS = {}


def _side_stream(device):
    key = (device.index if device.index is not None else torch.cuda.current_device())
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return s


class _WgradLane(object):
    """The second stream of one backward node: ``run(fn, *tensors)`` launches ``fn`` there after everything issued so far on the
    node's own stream; ``tensors`` (what fn reads or writes) stay referenced until ``join()`` makes the node's stream wait for the
    lane -- the caching allocator would otherwise hand a freed block to the next allocation while the lane still uses it."""

    def __init__(self, dims, like, taps):
        n = int(taps)
        for d in dims:
            n *= int(d)
        # (not while a hipGraph is being captured: ROCm 7.2 replays a forked graph no faster than the serial one, and its launch
        #  costs the host 0.5-6 ms instead of 0.1 -- profiles/r06_probes.md, section 1)
        self.on = 0 < n <= CONCURRENT_WGRAD_WORK and not torch.cuda.is_current_stream_capturing()
        self.keep = []
        if self.on:
            self.main = torch.cuda.current_stream()
            self.side = _side_stream(like.device)

    def run(self, fn, *tensors):
        if not self.on:
            return fn()
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            fn()
        self.keep.extend(tensors)

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)
            self.keep = []


# Which 3-D Winograd family the plain stride-1 convs (forward and dgrad) take where `_use_wino` says 3:
#   "f224"  F(2,3) x F(2,3) x F(4,3) (conv_wino43.hip, round 6): 6 matrix multiply-adds per output voxel and channel pair -- the default;
#   "f222"  F(2,3)^3 (conv_wino.hip): 8 of them, about one bit more accurate.
# The 27-point forms of an up-sampling block's first conv (forward / pooled adjoint) exist in the F(2,3)^3 family only; both families write /
# read the same sign-word layout, so they mix freely inside a block.
WINO3D_FAMILY = _os.environ.get("DF_WINO3D_FAMILY", "f224")
# ... and the 2-D twin: "f24" (default) = F(2,3) x F(4,3) (conv_wino2d43.hip: 3 multiply-adds per output pixel and channel pair) for forward convs
# and dgrads, "f22" = F(2,3)^2 (conv_wino2d.hip: 4), "auto" = f24 for the forward convs, f22 for the dgrads (the default before the f24
# epilogue moved to 16-byte accesses along the channels -- its 32 scalar fp32 mask reads per lane were not hidden; now 8 float4 reads: cfg2
# step 16.93 ms with "auto", 16.46 with "f24", profiles/r06_probes.md section 7).  The 9-point forms of an up-sampling block's first conv
# exist in the F(2,3)^2 family only.
WINO2D_FAMILY = _os.environ.get("DF_WINO2D_FAMILY", "f24")


def _w2fam(mode):
    """The 2-D Winograd family of a conv with pack mode `mode` (0 forward, 1 dgrad)."""
    return WINO2D_FAMILY if WINO2D_FAMILY != "auto" else ("f24" if mode == 0 else "f22")


def _use_wino(cin, cout, dims, kz):
    """0: direct kernel; 3: 3-D Winograd F(2x2x2,3x3x3) (conv_wino.hip); 2: 2-D Winograd F(2x2,3x3) (conv_wino2d.hip)."""
    if CONV_ALGO == "direct" or CONV_PRECISION != "fp32" or cin % 32 or cout % 32:
        return 0
    if kz == 3:
        # (from 6 voxels per axis on: at 7x10x7 -- cfg4's lowest level -- the direct kernel has 24 workgroups of 184 us each, the Winograd
        #  kernel 64 of a sixth of the work)
        return 3 if (CONV_ALGO == "winograd" or min(dims[1], dims[2], dims[3]) >= 6) else 0
    return 2 if (CONV_ALGO == "winograd" or (dims[2] >= 16 and dims[3] >= 24)) else 0


# Sign-bit masks (conv_wino.hip): the forward convs of a fused generator block whose outputs only serve, in the backward pass, as the
# lrelu mask of the next layer's dgrad also emit that mask as bit words (1/32 of the bytes); the masked dgrad then reads the words
# instead of the fp32 activation.  Same arithmetic, bit-identical results; only the 3-D Winograd kernels have the path.
SIGN_BIT_MASKS = _os.environ.get("DF_SIGN_BIT_MASKS", "1") != "0"


# The kernel of one stride-1 3x3(x3) conv under the current options:
#   kind   "wino43" | "wino" | "wino2d43" | "wino2d" | "direct";
#   fn     C-ABI prefix of its `*_packed_elems` / `*_pack_weights` pair;
#   sfx    "_bf16x3" where the direct kernel runs in that mode, else "";
#   form   its DISPATCH_COUNTS label (the thin case -- Cin or Cout <= 4 -- is a label of the direct kernel);
#   bits   the sign-word layout its forward can emit for the masked dgrad of the layer above: 0 none, 3 the 3-D Winograd kernels' bytes (both
#          3-D families read and write them), 2 the words of the 2-D F(2,3) x F(4,3) kernel -- only where the dgrads run on that kernel too
#          (WINO2D_FAMILY "f24": forward and dgrad share the thread <-> output mapping the words are indexed by).
_ConvKernel = collections.namedtuple("_ConvKernel", "kind fn sfx form bits")


def _conv_kernel(cin, cout, dims, kz, mode, family=None):
    """Which kernel a stride-1 conv cin -> cout on `dims` takes (mode 0 forward, 1 dgrad: the same layer with the two channel counts either way
    round -- every rule is symmetric in them).  Decided here and nowhere else: packing, launch, dispatch label and sign words are all read
    off the answer.  ``family`` ("f222" /
    "f22") overrides WINO3D_FAMILY / WINO2D_FAMILY: the 27-point and 9-point up-sampling forms exist in those families only.  ``dims=None``
    (an operand for a kernel outside this choice: the stride-2 forward): the direct kernel's format.  Evaluated per call, never kept: an
    `options` block may change the answer at any time."""
    algo = _use_wino(cin, cout, dims, kz) if dims is not None else 0
    if algo == 3:
        return _KERNELS["wino43" if (family or WINO3D_FAMILY) == "f224" else "wino", 3 if SIGN_BIT_MASKS else 0]
    if algo == 2:
        bits = 2 if (SIGN_BIT_MASKS and _w2fam(0) == "f24" and _w2fam(1) == "f24") else 0
        return _KERNELS["wino2d43" if (family or _w2fam(mode)) == "f24" else "wino2d", bits]
    if min(cin, cout) <= 4:
        return _KERNELS["thin-valu-forced" if THIN_VALU_ONLY else "thin", 0]
    return _KERNELS["direct-mfma" + _sfx(cin, cout), 0]


# every possible answer, built once (the choice runs several times per conv and step: a lookup, not a construction)
_KERNELS = {(kind, bits): _ConvKernel(kind, fn, "", form, bits) for bits in (0, 2, 3) for kind, fn, form in (
    ("wino43", "df_wino43", "winograd-f2x2x4"), ("wino", "df_wino", "winograd-f2x2x2"), ("wino2d43", "df_wino2d43", "winograd-f2x4"),
    ("wino2d", "df_wino2d", "winograd-f2x2"))}
_KERNELS.update({(form, 0): _ConvKernel("direct", "df_conv", sfx, form, 0) for form, sfx in (
    ("thin", ""), ("thin-valu-forced", ""), ("direct-mfma", ""), ("direct-mfma_bf16x3", "_bf16x3"))})


def _pack(w, taps, cin, cout, mode, dims=None, fp32=False, family=None):
    """Packed MFMA operand of w for the stride-1 conv on `dims` (mode 0: forward, mode 1: dgrad).  ``fp32=True`` forces the exact-fp32
    operand format whatever CONV_PRECISION says (kernels that have no bf16x3 variant: the stride-2 forward).  ``family="f222"``: the
    F(2,3)^3 operand whatever WINO3D_FAMILY says (the 27-point forms)."""
    k = _conv_kernel(cin, cout, dims, 3 if taps == 27 else 1, mode, family)
    if k.kind != "direct":
        wp = torch.empty(query(k.fn + "_packed_elems", cin, cout, mode), dtype=torch.float32, device=w.device)
        call(k.fn + "_pack_weights", _ptr(w), _ptr(wp), cin, cout, mode, _stream())
        return wp
    sfx = "" if fp32 else k.sfx
    wp = torch.empty(query(k.fn + "_packed_elems" + sfx, taps, cin, cout, mode), dtype=torch.float32, device=w.device)
    call(k.fn + "_pack_weights" + sfx, _ptr(w), _ptr(wp), taps, cin, cout, mode, _stream())
    return wp


def _upconv_pack(w, cin, cout, kz, mode, sfx=""):
    """Packed operand of the parity-class kernels (df_upconv_*): mode 0 forward, 1 dgrad, 2 the stride-2 conv's dgrad."""
    wp = torch.empty(query("df_upconv_packed_elems" + sfx, cin, cout, kz, mode), dtype=torch.float32, device=w.device)
    call("df_upconv_pack_weights" + sfx, _ptr(w), _ptr(wp), cin, cout, kz, mode, _stream())
    return wp


def _bits_kind(cin, cout, dims, kz):
    """Which sign-word layout a forward conv (cin -> cout on `dims`) can emit for the masked dgrad of the layer above (`_ConvKernel.bits`)."""
    return _conv_kernel(cin, cout, dims, kz, 0).bits


def _new_bits(dims, c, like, kind=3):
    B, D, H, W = dims
    nbytes = query("df_wino_signbits_bytes", B, D, H, W, c) if kind == 3 else query("df_wino2d43_signbits_bytes", B, H, W, c)
    return torch.empty(nbytes // 8, dtype=torch.int64, device=like.device)


def sign_words2d_to_mask(bits, dims, c):
    """Decode the sign words of ``df_wino2d43_conv_bits`` (conv_wino2d43.hip) into a bool tensor ``[B, H, W, c]`` = (activation > 0).  One 32-bit word
    per (tile block of 16 x 32 pixels, 32-cout slice cs, thread); thread = (wave = 4 yh + rp, lane = 16 kq + 4 qm + qi); bit (4 nb + e) * 4 + cc =
    pixel (16 by + 4 rp + 2 (kq >> 1) + (qi >> 1), 32 bx + 16 (kq & 1) + 4 e + 2 yh + (qi & 1)), channel 32 cs + 16 nb + 4 qm + cc."""
    B, _, H, W = (int(v) for v in dims)
    nby, nbx, ncs = -(-H // 16), -(-W // 32), c // 32
    wd = bits.view(torch.int32)[:B * nby * nbx * ncs * 512].view(B, nby, nbx, ncs, 2, 4, 2, 2, 4, 2, 2)      # [B, by, bx, cs, yh, rp, etr, kql, qm, qih, qil]
    sh = torch.arange(32, device=bits.device, dtype=torch.int32).view(2, 4, 4)                                # [nb, e, cc]
    m = ((wd[..., None, None, None] >> sh) & 1).bool()
    #   0  1   2   3   4   5   6    7    8   9    10   11  12  13
    #  [B, by, bx, cs, yh, rp, etr, kql, qm, qih, qil, nb, e, cc]  ->  (B | by rp etr qih | bx kql e yh qil | cs nb qm cc)
    m = m.permute(0, 1, 5, 6, 9, 2, 7, 12, 4, 10, 3, 11, 8, 13).reshape(B, nby * 16, nbx * 32, c)
    return m[:, :H, :W].contiguous()


def sign_bits_to_mask(bits, dims, c):
    """Decode the sign words of ``df_wino_conv_fwd_bits`` / ``_addup_bits`` / ``df_wino_upconv_fwd_bits`` (conv_wino.hip, kSignBits) into
    a bool tensor ``[B, D, H, W, c]`` = (activation > 0).  Layout: one byte per (tile block, cout slice, wave = (z-row th, xi_z), cout
    16-block nb, lane = (kq, tl)); bit s = (dz, dy, dx) of the lane's 2x2x2 outputs at (4 bz + 2 th + dz, 8 by + 2 kq + dy,
    8 bx + 2 xi_z + dx), channel 32 cs + 16 nb + tl.  The fetch-list counterpart for layers whose fp32 activation is never written."""
    B, D, H, W = (int(v) for v in dims)
    nbz, nby, nbx, ncs = -(-D // 4), -(-H // 8), -(-W // 8), c // 32
    by = bits.view(torch.uint8)[:B * nbz * nby * nbx * ncs * 1024].view(B, nbz, nby, nbx, ncs, 2, 4, 2, 4, 16)
    sh = torch.arange(8, device=bits.device, dtype=torch.uint8).view(2, 2, 2)
    m = ((by[..., None, None, None] >> sh) & 1).bool()      # [B, bz, by, bx, cs, th, xz, nb, kq, tl, dz, dy, dx]
    m = m.permute(0, 1, 5, 10, 2, 8, 11, 3, 6, 12, 4, 7, 9).reshape(B, nbz * 4, nby * 8, nbx * 8, c)
    return m[:, :D, :H, :W].contiguous()


# Fetch of the block-tail sign words (see ACTIVATION_FETCH below): when set to a list, every up-sampling block on the production tail
# (df_wino_conv_fwd_addup_bits: the last conv's activation is never written) appends ``(bits, fdims, cout)``; tests decode them with
# sign_bits_to_mask and compare with the activations of the fp32-mask path.
SIGN_BITS_FETCH = None


def _conv_raw(x, wp, bias, residual, mask_src, dims, cin, cout, kz, flags, leak, sign_bits=None, mask_bits=None):
    """`wp` must come from ``_pack(..., dims)`` with the same dims AND mode: both ask `_conv_kernel` (every forward call carries DF_CONV_BIAS,
    no dgrad call does -- that is how the pack mode is recognised here)."""
    mode = 0 if (flags & DF_CONV_BIAS) else 1
    B, D, H, W = dims
    y = torch.empty((B, D, H, W, cout), dtype=torch.float32, device=x.device)
    k = _conv_kernel(cin, cout, dims, kz, mode)
    if DISPATCH_COUNTS is not None:
        _count("conv", k.form, dims, cin, cout)
    words = sign_bits is not None or mask_bits is not None
    if k.kind == "wino43":
        call("df_wino43_conv", _ptr(x), _ptr(wp), _ptr(bias), _ptr(residual), _ptr(mask_src), _ptr(mask_bits), _ptr(y), None, _ptr(sign_bits),
             B, D, H, W, cin, cout, flags, float(leak), _stream())
    elif k.kind == "wino" and words:
        call("df_wino_conv_fwd_bits", _ptr(x), _ptr(wp), _ptr(bias), _ptr(mask_bits), _ptr(y), _ptr(sign_bits), B, D, H, W, cin, cout,
             flags, float(leak), _stream())
    elif k.kind == "wino":
        call("df_wino_conv_fwd", _ptr(x), _ptr(wp), _ptr(bias), _ptr(residual), _ptr(mask_src), _ptr(y), B, D, H, W, cin, cout,
             flags, float(leak), _stream())
    elif k.kind == "wino2d43" and words:
        call("df_wino2d43_conv_bits", _ptr(x), _ptr(wp), _ptr(bias), _ptr(mask_bits), _ptr(y), _ptr(sign_bits), B, H, W, cin, cout, flags, float(leak),
             _stream())
    elif words:
        raise _lib.DeepFluidsHipError("sign-bit masks exist for the 3-D Winograd kernels and the 2-D F(2,3) x F(4,3) kernel only")
    elif k.kind == "wino2d43":
        call("df_wino2d43_conv", _ptr(x), _ptr(wp), _ptr(bias), _ptr(residual), _ptr(mask_src), _ptr(y), B, H, W, cin, cout, flags, float(leak),
             _stream())
    elif k.kind == "wino2d":
        call("df_wino2d_conv_fwd", _ptr(x), _ptr(wp), _ptr(bias), _ptr(residual), _ptr(mask_src), _ptr(y), B, H, W, cin, cout,
             flags, float(leak), _stream())
    else:
        if THIN_VALU_ONLY and not k.sfx:      # (df_conv_fwd_bf16x3 has no thin layers and refuses the flag)
            flags |= _lib.DF_CONV_VALU_ONLY
        call("df_conv_fwd" + k.sfx, _ptr(x), _ptr(wp), _ptr(bias), _ptr(residual), _ptr(mask_src), _ptr(y), B, D, H, W,
             cin, cout, kz, flags, float(leak), _stream())
    return y


def _geom(x, ws, who):
    """``(kz, taps, dims)`` of the k=3 convs with weights `ws` applied in a row to the channels-last `x` ([B, (D,) H, W, C]); raises where a
    weight is not [3, (3,) 3, Cin, Cout] with Cin the channel count that reaches it.  `who` names the caller in the error."""
    nd = x.dim() - 2
    c = x.shape[-1]
    for w in ws:
        if tuple(w.shape[:-2]) != (3,) * nd or w.shape[-2] != c:
            raise ValueError("%s: weights %s do not match input %s (k=3 only)" % (who, tuple(w.shape), tuple(x.shape[:-1]) + (c,)))
        c = w.shape[-1]
    dims = (x.shape[0], x.shape[1] if nd == 3 else 1, x.shape[-3], x.shape[-2])
    return (3, 27, dims) if nd == 3 else (1, 9, dims)


def _conv_bwd_prologue(gy, y, leak, w, bptr):
    """What the backward of a single conv starts with: the gradient through the fused lrelu (if any) and the outputs of the weight / bias
    gradient kernels -> ``(dp, gw, rw, gb, rb)`` (rw, rb: what backward returns for them, see `_grad_out`)."""
    gy = _prep(gy, "grad")
    if leak is not None:
        dp = torch.empty_like(gy)
        call("df_lrelu_bwd", _ptr(gy), _ptr(y), _ptr(dp), float(leak), gy.numel(), _stream())
    else:
        dp = gy
    gw, rw = _grad_out(w.data_ptr(), w.shape, w.device)
    gb, rb = _grad_out(bptr, (w.shape[-1],), w.device)
    return dp, gw, rw, gb, rb


class _ConvSame3(torch.autograd.Function):
    """k=3, stride-1, SAME conv (+bias, + optional fused lrelu) on the fp32 MFMA kernels."""

    @staticmethod
    def forward(ctx, x, w, b, leak):
        x = _prep(x, "x"); w = _prep(w, "weights"); b = _prep(b, "biases")
        kz, taps, dims = _geom(x, [w], "conv")
        cin, cout = w.shape[-2], w.shape[-1]
        wp = _pack(w, taps, cin, cout, 0, dims)
        flags = DF_CONV_BIAS | (DF_CONV_LRELU if leak is not None else 0)
        y = _conv_raw(x, wp, b, None, None, dims, cin, cout, kz, flags, leak if leak is not None else 0.0)
        y = y.view(x.shape[:-1] + (cout,))
        if ACTIVATION_FETCH is not None and leak is not None:
            ACTIVATION_FETCH.append(y)
        ctx.save_for_backward(x, w, y if leak is not None else None)
        ctx.leak = leak
        ctx.geom = (dims, cin, cout, kz, taps)
        ctx.bptr = b.data_ptr()
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        dims, cin, cout, kz, taps = ctx.geom
        B, D, H, W = dims
        dp, gw, rw, gb, rb = _conv_bwd_prologue(gy, y, ctx.leak, w, ctx.bptr)
        _wgrad(x, dp, gw, gb, B, D, H, W, cin, cout, kz, _sfx(cin, cout))
        gx = None
        if ctx.needs_input_grad[0]:
            wpd = _pack(w, taps, cin, cout, 1, dims)
            gx = _conv_raw(dp, wpd, None, None, None, dims, cout, cin, kz, 0, 0.0).view(x.shape)
        return gx, rw, rb, None


# The per-layer steps the fused nodes (_ConvStack, _UpGenBlock) share.
def _layer_fwd(x, w, b, dims, kz, taps, leak, want_bits):
    """conv k3 s1 + bias + lrelu -> (activation, its sign words or None).  `want_bits`: the activation only serves as the lrelu mask of the
    dgrad of the layer above -- emit the mask as sign words too, where this layer's kernel can."""
    cin, cout = w.shape[-2], w.shape[-1]
    wp = _pack(w, taps, cin, cout, 0, dims)
    bk = _bits_kind(cin, cout, dims, kz) if want_bits else 0
    sb = _new_bits(dims, cout, x, bk) if bk else None
    y = _conv_raw(x, wp, b, None, None, dims, cin, cout, kz, DF_CONV_BIAS | DF_CONV_LRELU, leak, sign_bits=sb)
    return y.view(x.shape[:-1] + (cout,)), sb


def _layer_wgrad(lane, x, dp, w, bptr, dims, kz):
    """Weight and bias gradient of the layer with input `x` and masked output gradient `dp`, on the lane -> what backward returns for (w, b)."""
    cin, cout = w.shape[-2], w.shape[-1]
    B, D, H, W = dims
    gw, rw = _grad_out(w.data_ptr(), w.shape, dp.device)
    gb, rb = _grad_out(bptr, (cout,), dp.device)
    lane.run(lambda: _wgrad(x, dp, gw, gb, B, D, H, W, cin, cout, kz, _sfx(cin, cout)), dp, gw, gb)
    return rw, rb


def _layer_dgrad_masked(dp, w, dims, kz, taps, leak, act, bits):
    """dgrad of a layer times the lrelu slope of the layer below -- from that layer's sign words `bits` if its forward emitted them, else from
    its fp32 activation `act`: directly the next dp."""
    cin, cout = w.shape[-2], w.shape[-1]
    wpd = _pack(w, taps, cin, cout, 1, dims)
    return _conv_raw(dp, wpd, None, None, None if bits is not None else act, dims, cout, cin, kz, DF_CONV_MASK, leak, mask_bits=bits).view(act.shape)


class _ConvStack(torch.autograd.Function):
    """n x [conv k3 s1 + bias + lrelu] in a row as ONE autograd node, with (``skip``) or without the residual add of the input at the end:
    a generator block (model.py:24-40 / 66-82) or the per-level conv stack of the encoder (model.py:131-136 / 167-172; its first conv may
    change the channel count).  Forward = the same kernels as the layer-by-layer path; the hand-written reverse chain uses the fused
    epilogues of the conv kernels: each dgrad multiplies by the lrelu slope of the layer below (DF_CONV_MASK; sign words where the Winograd
    forward emits them) and with ``skip`` the first layer's dgrad adds the skip gradient (DF_CONV_RESIDUAL) -- per block three element-wise
    passes and one gradient-accumulation pass over the activations less; only the LAST layer's element-wise lrelu-backward pass remains."""

    @staticmethod
    def forward(ctx, x0, leak, skip, *wb):
        who = "gen_block" if skip else "conv_chain"
        x0 = _prep(x0, "x")
        n = len(wb) // 2
        ws = [_prep(w, "weights") for w in wb[0::2]]
        bs = [_prep(b, "biases") for b in wb[1::2]]
        kz, taps, dims = _geom(x0, ws, who)
        xs = [x0]
        bits = []
        for i in range(n):
            # outputs of convs 1 .. n-1 are the masks of the dgrads of convs 2 .. n
            x, sb = _layer_fwd(xs[i], ws[i], bs[i], dims, kz, taps, leak, i < n - 1)
            xs.append(x)
            bits.append(sb)
        y = xs[n]
        if skip:
            if y.shape != x0.shape:
                raise ValueError("gen_block: residual add needs Cout == Cin of the block")
            y = torch.empty_like(y)
            call("df_add", _ptr(xs[n]), _ptr(x0), _ptr(y), y.numel(), _stream())
        if ACTIVATION_FETCH is not None:
            ACTIVATION_FETCH.extend(xs[1:])
        ctx.save_for_backward(*(xs + list(wb[0::2])))
        ctx.geom = (n, dims, kz, taps, float(leak), skip)
        ctx.bits = bits
        ctx.bptrs = [b.data_ptr() for b in wb[1::2]]
        return y

    @staticmethod
    def backward(ctx, dy):
        n, dims, kz, taps, leak, skip = ctx.geom
        saved = ctx.saved_tensors
        xs, ws = saved[:n + 1], saved[n + 1:]
        dy = _prep(dy, "grad")
        dp = torch.empty_like(dy)
        call("df_lrelu_bwd", _ptr(dy), _ptr(xs[n]), _ptr(dp), leak, dy.numel(), _stream())
        grads = [None] * (2 * n)
        dx0 = None
        lane = _WgradLane(dims, dy, taps)
        for i in range(n, 0, -1):
            w = ws[i - 1]
            grads[2 * i - 2], grads[2 * i - 1] = _layer_wgrad(lane, xs[i - 1], dp, w, ctx.bptrs[i - 1], dims, kz)
            if i > 1:
                dp = _layer_dgrad_masked(dp, w, dims, kz, taps, leak, xs[i - 1], ctx.bits[i - 2])
            elif ctx.needs_input_grad[0]:   # dgrad of the first layer, + the skip gradient in its epilogue
                cin, cout = w.shape[-2], w.shape[-1]
                wpd = _pack(w, taps, cin, cout, 1, dims)
                dx0 = _conv_raw(dp, wpd, None, dy if skip else None, None, dims, cout, cin, kz, DF_CONV_RESIDUAL if skip else 0, 0.0).view(xs[0].shape)
        lane.join()
        return (dx0, None, None) + tuple(grads)


class _GenBlock(object):
    """One generator block as a single autograd node: ``_GenBlock.apply(x, leak, w1, b1, ..., wn, bn)`` = `_ConvStack` with the skip."""

    @staticmethod
    def apply(x, leak, *wb):
        return _ConvStack.apply(x, leak, True, *wb)


class _ConvChain(object):
    """The encoder's per-level conv stack as a single autograd node: `_ConvStack` without the skip."""

    @staticmethod
    def apply(x, leak, *wb):
        return _ConvStack.apply(x, leak, False, *wb)


_UP_FORMS = {"wino": "winograd-27pt", "wino2d": "winograd2d-9pt"}      # DISPATCH_COUNTS labels of the up-sampling-aware Winograd forms, by kernel kind


def _fused_tail(k, x, w, b, xc, fdims, taps, leak):
    """The last conv of an up-sampling block on kernel `k` with the block-end skip add fused into its epilogue: ``y = lrelu(conv(x)) +
    upscale(xc)`` -> ``(activation, y, tail_bits)``, or None where `k` has no such epilogue (the caller then runs conv and add apart).
    With sign-bit masks on and nobody fetching activations, of the conv's own activation only the sign words are kept (``tail_bits``: all
    the backward tail needs of it) and the activation is None; otherwise (3-D only) the fp32 activation is a second output."""
    is3d = k.kind in ("wino43", "wino")
    words = bool(k.bits) and ACTIVATION_FETCH is None
    if not (is3d or words):
        return None
    cin, cout = w.shape[-2], w.shape[-1]
    B, D, H, W = fdims
    wp = _pack(w, taps, cin, cout, 0, fdims)
    _count("conv", k.form + ("+addup+signwords" if words else "+addup"), fdims, cin, cout)
    tail_bits = _new_bits(fdims, cout, xc, k.bits) if words else None
    act = None if words else torch.empty_like(x)
    y = torch.empty_like(x)
    if k.kind == "wino43":
        call("df_wino43_conv", _ptr(x), _ptr(wp), _ptr(b), _ptr(xc), None, None, _ptr(act), _ptr(y), _ptr(tail_bits), B, D, H, W, cin, cout,
             DF_CONV_BIAS | DF_CONV_LRELU | _lib.DF_CONV_ADDUP, float(leak), _stream())
    elif k.kind == "wino" and words:
        call("df_wino_conv_fwd_addup_bits", _ptr(x), _ptr(wp), _ptr(b), _ptr(xc), _ptr(y), _ptr(tail_bits), B, D, H, W, cin, cout, float(leak), _stream())
    elif k.kind == "wino":
        call("df_wino_conv_fwd_addup", _ptr(x), _ptr(wp), _ptr(b), _ptr(xc), _ptr(act), _ptr(y), B, D, H, W, cin, cout, float(leak), _stream())
    else:
        call("df_wino2d43_conv_addup_bits", _ptr(x), _ptr(wp), _ptr(b), _ptr(xc), _ptr(y), _ptr(tail_bits), B, H, W, cin, cout, float(leak), _stream())
    if words and is3d and SIGN_BITS_FETCH is not None:
        SIGN_BITS_FETCH.append((tail_bits, fdims, cout))
    return act, y, tail_bits


class _UpGenBlock(torch.autograd.Function):
    """``x0 = upscale(xc, 2)`` followed by one generator block (model.py:36-40 / 78-82) as a single autograd node that
    never materialises ``x0``: the block's first conv runs on the coarse input -- as the up-sampling-aware form of the fine grid's
    Winograd kernel (27 of the 64 / 9 of the 16 products: F(2,3)^3 / F(2,3)^2 only) or as parity-class 2x2(x2)-tap convs
    (``df_upconv_*``: 3.4x fewer FLOPs forward, dgrad and 2.25x fewer in wgrad) --, the block-end residual add reads the coarse tensor
    (the last conv's epilogue, or ``df_add_up2x``) and the skip gradient is the 2x2(x2) sum-pool of dy."""

    @staticmethod
    def forward(ctx, xc, leak, *wb):
        xc = _prep(xc, "x")
        n = len(wb) // 2
        ws = [_prep(w, "weights") for w in wb[0::2]]
        bs = [_prep(b, "biases") for b in wb[1::2]]
        C = int(xc.shape[-1])
        kz, taps, cdims = _geom(xc, ws, "up_gen_block")
        for w in ws:
            if w.shape[-1] != C:
                raise ValueError("up_gen_block: weights %s do not match %d channels" % (tuple(w.shape), C))
        is3d = kz == 3
        fdims = (cdims[0], 2 * cdims[1] if is3d else 1, 2 * cdims[2], 2 * cdims[3])
        fshape = (xc.shape[0],) + tuple(2 * int(d) for d in xc.shape[1:-1]) + (C,)
        Bc, Dc, Hc, Wc = cdims
        fam = "f222" if is3d else "f22"       # the up-sampling-aware forms exist in these families only
        first = _conv_kernel(C, C, fdims, kz, 0, family=fam)
        last = _conv_kernel(C, C, fdims, kz, 0)
        xs = []
        bits = []
        y = None
        tail_bits = None
        for i in range(n):
            # (2-D: the block's first conv runs the 9-point F(2,3)^2 form, which has no sign words -- the dgrad above it reads its fp32 activation)
            want_bits = i < n - 1 and (is3d or i > 0)
            if i == 0:
                sb = _new_bits(fdims, C, xc, first.bits) if (want_bits and first.bits) else None
                _count("upconv", _UP_FORMS.get(first.kind, "parity-class" + first.sfx), fdims, C, C)
                x = torch.empty(fshape, dtype=torch.float32, device=xc.device)
                if first.kind == "direct":
                    wp = _upconv_pack(ws[0], C, C, kz, 0, first.sfx)
                    call("df_upconv_fwd" + first.sfx, _ptr(xc), _ptr(wp), _ptr(bs[0]), _ptr(x), Bc, Dc, Hc, Wc, C, C, kz, DF_CONV_BIAS | DF_CONV_LRELU,
                         float(leak), _stream())
                else:
                    wp = _pack(ws[0], taps, C, C, 0, fdims, family=fam)      # the operand of a plain conv of that family
                    if first.kind == "wino2d":      # 9 of the 16 Winograd products (conv_wino2d.hip, UP variant)
                        call("df_wino2d_upconv_fwd", _ptr(xc), _ptr(wp), _ptr(bs[0]), _ptr(x), Bc, Hc, Wc, C, C, DF_CONV_BIAS | DF_CONV_LRELU, float(leak),
                             _stream())
                    elif sb is not None:            # 27-point form (conv_wino.hip, UP variant)
                        call("df_wino_upconv_fwd_bits", _ptr(xc), _ptr(wp), _ptr(bs[0]), _ptr(x), _ptr(sb), Bc, Dc, Hc, Wc, C, C, float(leak), _stream())
                    else:
                        call("df_wino_upconv_fwd", _ptr(xc), _ptr(wp), _ptr(bs[0]), _ptr(x), Bc, Dc, Hc, Wc, C, C, DF_CONV_BIAS | DF_CONV_LRELU,
                             float(leak), _stream())
            else:
                tail = _fused_tail(last, x, ws[i], bs[i], xc, fdims, taps, leak) if i == n - 1 else None
                if tail is not None:
                    (x, y, tail_bits), sb = tail, None
                else:
                    x, sb = _layer_fwd(x, ws[i], bs[i], fdims, kz, taps, leak, want_bits)
            bits.append(sb)
            xs.append(x)
        if y is None:
            y = torch.empty_like(x)
            call("df_add_up2x", _ptr(x), _ptr(xc), _ptr(y), Bc, Dc, Hc, Wc, C, int(is3d), _stream())
        if ACTIVATION_FETCH is not None:
            ACTIVATION_FETCH.extend(xs)
        ctx.save_for_backward(*([xc] + xs + list(wb[0::2])))
        ctx.geom = (n, cdims, fdims, kz, taps, float(leak), C, is3d)
        ctx.bits = bits
        ctx.tail_bits = tail_bits
        ctx.bptrs = [b.data_ptr() for b in wb[1::2]]
        return y

    @staticmethod
    def backward(ctx, dy):
        n, cdims, fdims, kz, taps, leak, C, is3d = ctx.geom
        saved = ctx.saved_tensors
        xc, xs, ws = saved[0], saved[1:n + 1], saved[n + 1:]
        Bc, Dc, Hc, Wc = cdims
        dy = _prep(dy, "grad")
        dp = torch.empty_like(dy)
        dxc = None
        if ctx.tail_bits is not None:
            # the lrelu mask of the last conv from its sign bits (its fp32 activation was never written): 6.9 GB moved at the cfg3 top
            # level instead of 12.9; the pooled skip gradient comes with it (dropped below if xc needs no gradient)
            dxc = torch.empty_like(xc)
            if is3d:
                call("df_lrelu_bits_bwd_pool2x", _ptr(dy), _ptr(ctx.tail_bits), _ptr(dp), _ptr(dxc), leak, Bc, Dc, Hc, Wc, C, _stream())
            else:
                call("df_lrelu_words2d_bwd_pool2x", _ptr(dy), _ptr(ctx.tail_bits), _ptr(dp), _ptr(dxc), leak, Bc, Hc, Wc, C, _stream())
        elif ctx.needs_input_grad[0]:
            # both consumers of dy in one pass: the masked gradient entering the last conv and the skip path's 2x2(x2) sum-pool
            dxc = torch.empty_like(xc)
            call("df_lrelu_bwd_pool2x", _ptr(dy), _ptr(xs[n - 1]), _ptr(dp), _ptr(dxc), leak, Bc, Dc, Hc, Wc, C, int(is3d), _stream())
        else:
            call("df_lrelu_bwd", _ptr(dy), _ptr(xs[n - 1]), _ptr(dp), leak, dy.numel(), _stream())
        grads = [None] * (2 * n)
        lane = _WgradLane(fdims, dy, taps)
        for i in range(n, 1, -1):      # sign bits of conv i-1's output (xs[i-2]), if its forward emitted them
            grads[2 * i - 2], grads[2 * i - 1] = _layer_wgrad(lane, xs[i - 2], dp, ws[i - 1], ctx.bptrs[i - 1], fdims, kz)
            dp = _layer_dgrad_masked(dp, ws[i - 1], fdims, kz, taps, leak, xs[i - 2], ctx.bits[i - 2])
        # the first conv, on the coarse input
        w = ws[0]
        sfx = _sfx(C, C)
        gw, grads[0] = _grad_out(w.data_ptr(), w.shape, dy.device)
        gb, grads[1] = _grad_out(ctx.bptrs[0], (C,), dy.device)
        nbytes = query("df_upconv_wgrad_workspace_bytes", Bc, Dc, Hc, Wc, C, C, kz)
        wsb = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dy.device)

        def up_wgrad():
            if sfx:
                call("df_upconv_wgrad" + sfx, _ptr(xc), _ptr(dp), _ptr(gw), _ptr(gb), Bc, Dc, Hc, Wc, C, C, kz, _ptr(wsb), nbytes, _stream())
            else:
                if DISPATCH_COUNTS is not None:
                    f = query("df_upconv_wgrad_form", Bc, Dc, Hc, Wc, C, C, kz, int(WGRAD_ALGO))
                    _count("upconv-wgrad", "winograd-xyz-27pt" if f == 3 else "parity-class", fdims, C, C)
                call("df_upconv_wgrad_algo", _ptr(xc), _ptr(dp), _ptr(gw), _ptr(gb), Bc, Dc, Hc, Wc, C, C, kz, _ptr(wsb), nbytes, int(WGRAD_ALGO),
                     _stream())
        lane.run(up_wgrad, dp, gw, gb, wsb)
        if ctx.needs_input_grad[0]:
            # dxc holds the skip path's sum-pool of dy (the prologue above); += the conv path
            fam = "f222" if is3d else "f22"
            first = _conv_kernel(C, C, fdims, kz, 1, family=fam)
            _count("upconv-dgrad", _UP_FORMS[first.kind] + "-pooled" if first.kind in _UP_FORMS else "parity-class" + first.sfx, fdims, C, C)
            if first.kind == "direct":      # per parity class
                wpd = _upconv_pack(w, C, C, kz, 1, first.sfx)
                call("df_upconv_dgrad" + first.sfx, _ptr(dp), _ptr(wpd), _ptr(dxc), Bc, Dc, Hc, Wc, C, C, kz, _stream())
            else:
                wpd = _pack(w, taps, C, C, 1, fdims, family=fam)
                if first.kind == "wino":    # pooled-output Winograd form (conv_wino.hip, POOL variant): 27 of the 64 products, coarse stores
                    call("df_wino_upconv_dgrad", _ptr(dp), _ptr(wpd), _ptr(dxc), Bc, Dc, Hc, Wc, C, C, _stream())
                else:
                    call("df_wino2d_upconv_dgrad", _ptr(dp), _ptr(wpd), _ptr(dxc), Bc, Hc, Wc, C, C, _stream())
        lane.join()
        return (dxc if ctx.needs_input_grad[0] else None, None) + tuple(grads)


class _ConvSame3S2(torch.autograd.Function):
    """k=3, stride-2, TF-'SAME' conv on even extents (pad 0 before / 1 after): the encoder's
    down-sampling layers (model.py:141-143, 177-179).  Forward is a dedicated MFMA kernel; the backward has native forms on the output
    grid and, for the shapes those are not instantiated for, re-uses the stride-1 dgrad / wgrad kernels on the zero-inserted gradient
    (out[2o+1] = g[o]), which reproduces the stride-2 adjoints exactly (at 4x / 8x the minimal FLOPs)."""

    @staticmethod
    def forward(ctx, x, w, b, leak):
        x = _prep(x, "x"); w = _prep(w, "weights"); b = _prep(b, "biases")
        kz, taps, idims = _geom(x, [w], "conv")
        cin, cout = w.shape[-2], w.shape[-1]
        if any(int(d) % 2 for d in x.shape[1:-1]):
            raise NotImplementedError("stride-2 conv: even spatial extents only (the encoder asserts them, model.py:125,161)")
        odims = (idims[0], idims[1] // 2 if kz == 3 else 1, idims[2] // 2, idims[3] // 2)
        wp = _pack(w, taps, cin, cout, 0, fp32=True)       # df_conv_s2_fwd has no bf16x3 variant: always the fp32 operand
        flags = DF_CONV_BIAS | (DF_CONV_LRELU if leak is not None else 0)
        y = torch.empty(odims + (cout,), dtype=torch.float32, device=x.device)
        call("df_conv_s2_fwd", _ptr(x), _ptr(wp), _ptr(b), _ptr(y), odims[0], odims[1], odims[2], odims[3], cin, cout, kz,
             flags, float(leak if leak is not None else 0.0), _stream())
        y = y.view((x.shape[0],) + tuple(int(d) // 2 for d in x.shape[1:-1]) + (cout,))
        if ACTIVATION_FETCH is not None and leak is not None:
            ACTIVATION_FETCH.append(y)
        ctx.save_for_backward(x, w, y if leak is not None else None)
        ctx.leak = leak
        ctx.geom = (idims, odims, cin, cout, kz, taps)
        ctx.bptr = b.data_ptr()
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        idims, odims, cin, cout, kz, taps = ctx.geom
        B, D, H, W = idims
        dp, gw, rw, gb, rb = _conv_bwd_prologue(gy, y, ctx.leak, w, ctx.bptr)
        up = []

        def zero_inserted():      # out[2o+1] = g[o] on the input grid: built once, where it is first needed
            if not up:
                up.append(torch.empty((B, D, H, W, cout), dtype=torch.float32, device=x.device))
                call("df_dilate2_odd", _ptr(dp), _ptr(up[0]), odims[0], odims[1], odims[2], odims[3], cout, int(kz == 3), _stream())
            return up[0]
        nbytes = query("df_conv_s2_wgrad_workspace_bytes", odims[0], odims[1], odims[2], odims[3], cin, cout, kz)
        if nbytes > 0 and WGRAD_ALGO == 0:
            # native form on the output grid: x[2o + t] * g[o] (conv_wgrad.hip::wgrad_s2_kernel) -- no zero-inserted gradient
            _count("wgrad-s2", "native-direct-mfma", odims, cin, cout)
            ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
            call("df_conv_s2_wgrad", _ptr(x), _ptr(dp), _ptr(gw), _ptr(gb), odims[0], odims[1], odims[2], odims[3], cin, cout, kz, _ptr(ws),
                 nbytes, _stream())
        else:
            # shapes the native kernel is not instantiated for: the stride-1 kernels on the zero-inserted gradient
            _wgrad(x, zero_inserted(), gw, gb, B, D, H, W, cin, cout, kz)
        gx = None
        if ctx.needs_input_grad[0]:
            if cin > 4 and cout > 4:
                # adjoint as 8 (4) parity-class 2x2(x2)-tap convs from the coarse gradient straight to the fine grid: the
                # up-sampling-aware forward kernel with the stride-2 dgrad operand (pack mode 2) -- 3.4x fewer FLOPs than the
                # stride-1 dgrad on the zero-inserted gradient, which stays as the thin-channel fallback below
                wpd = _upconv_pack(w, cin, cout, kz, 2)
                gx = torch.empty((B, D, H, W, cin), dtype=torch.float32, device=x.device)
                # [r5] df_conv_s2_dgrad: the same parity classes, each on a kernel specialised on its LIVE taps (27 of the 64 the generic
                # 2x2x2-tap parity-class kernel df_upconv_fwd multiplies -- half of the mode-2 operand is structural zeros)
                if DISPATCH_COUNTS is not None:      # (the library falls back to the generic class kernel on other channel counts / an unaligned gradient)
                    _count("dgrad-s2", "parity-class-live-taps" if query("df_conv_s2_dgrad_form", _ptr(dp), cin, cout) == 1 else
                           "parity-class-generic", odims, cin, cout)
                call("df_conv_s2_dgrad", _ptr(dp), _ptr(wpd), _ptr(gx), odims[0], odims[1], odims[2], odims[3], cin, cout, kz, _stream())
                gx = gx.view(x.shape)
            else:
                g = zero_inserted()
                wpd = _pack(w, taps, cin, cout, 1, idims)
                gx = _conv_raw(g, wpd, None, None, None, idims, cout, cin, kz, 0, 0.0).view(x.shape)
        return gx, rw, rb, None



class _Concat2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = _prep(a, "a"); b = _prep(b, "b")
        if a.shape[:-1] != b.shape[:-1]:
            raise ValueError("concat: leading shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        ca, cb = a.shape[-1], b.shape[-1]
        rows = a.numel() // ca
        y = _empty(tuple(a.shape[:-1]) + (ca + cb,), a)
        call("df_concat2_fwd", _ptr(a), _ptr(b), _ptr(y), rows, ca, cb, _stream())
        ctx.geom = (rows, ca, cb, tuple(a.shape), tuple(b.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        rows, ca, cb, sa, sb = ctx.geom
        gy = _prep(gy, "grad")
        ga, gb = _empty(sa, gy), _empty(sb, gy)
        call("df_concat2_bwd", _ptr(gy), _ptr(ga), _ptr(gb), rows, ca, cb, _stream())
        return ga, gb


class _Sigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _prep(x, "x")
        y = torch.empty_like(x)
        call("df_sigmoid_fwd", _ptr(x), _ptr(y), x.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = _prep(gy, "grad")
        gx = torch.empty_like(gy)
        call("df_sigmoid_bwd", _ptr(gy), _ptr(y), _ptr(gx), gy.numel(), _stream())
        return gx


class _KlBernoulli(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, n, rho):
        z = _prep(z, "z")
        if z.dim() != 2 or not 0 <= n <= z.shape[1]:
            raise ValueError("kl_bernoulli: z must be [B, ncol] with n <= ncol")
        out = torch.empty((), dtype=torch.float32, device=z.device)
        call("df_kl_bernoulli_fwd", _ptr(z), z.shape[0], z.shape[1], int(n), float(rho), _ptr(out), _stream())
        ctx.save_for_backward(z)
        ctx.geom = (int(n), float(rho))
        return out

    @staticmethod
    def backward(ctx, gout):
        (z,) = ctx.saved_tensors
        n, rho = ctx.geom
        gout = _prep(gout, "grad")
        gz = torch.empty_like(z)
        call("df_kl_bernoulli_bwd", _ptr(z), _ptr(gout), 1.0, _ptr(gz), z.shape[0], z.shape[1], n, rho, _stream())
        return gz, None, None


class _MseMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = _prep(a, "a"); b = _prep(b, "b")
        if a.shape != b.shape:
            raise ValueError("mse_mean: shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        n = a.numel()
        out = _empty((), a)
        nbytes = query("df_l1_mean_workspace_bytes", n)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
        call("df_mse_mean_fwd", _ptr(a), _ptr(b), n, _ptr(out), _ptr(ws), nbytes, _stream())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        gout = _prep(gout, "grad")
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = torch.empty_like(a)
            call("df_mse_mean_bwd", _ptr(a), _ptr(b), _ptr(gout), 1.0, _ptr(ga), a.numel(), _stream())
        if ctx.needs_input_grad[1]:
            gb = torch.empty_like(b)
            call("df_mse_mean_bwd", _ptr(a), _ptr(b), _ptr(gout), -1.0, _ptr(gb), a.numel(), _stream())
        return ga, gb


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = _prep(x, "x"); w = _prep(w, "weights"); b = _prep(b, "biases")
        B, K = x.shape
        N = w.shape[1]
        if w.shape[0] != K:
            raise ValueError("linear: weights %s do not match input %s" % (tuple(w.shape), tuple(x.shape)))
        y = _empty((B, N), x)
        nbytes = query("df_linear_workspace_bytes", B, K, N)
        ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device)
        call("df_linear_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, K, N, _ptr(ws), nbytes, _stream())
        ctx.save_for_backward(x, w)
        ctx.bptr = b.data_ptr()
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _prep(gy, "grad")
        B, K = x.shape
        N = w.shape[1]
        gw, rw = _grad_out(w.data_ptr(), w.shape, x.device)
        gb, rb = _grad_out(ctx.bptr, (N,), x.device)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        call("df_linear_bwd", _ptr(x), _ptr(w), _ptr(gy), _ptr(gx), _ptr(gw), _ptr(gb), B, K, N, _stream())
        return gx, rw, rb


class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _prep(x, "x")
        is3d = x.dim() == 5
        B = x.shape[0]
        D = x.shape[1] if is3d else 1
        H, W, C = x.shape[-3], x.shape[-2], x.shape[-1]
        out_shape = (B, 2 * D, 2 * H, 2 * W, C) if is3d else (B, 2 * H, 2 * W, C)
        y = _empty(out_shape, x)
        call("df_upsample2x_fwd", _ptr(x), _ptr(y), B, D, H, W, C, int(is3d), _stream())
        ctx.geom = (B, D, H, W, C, is3d, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        B, D, H, W, C, is3d, shp = ctx.geom
        gy = _prep(gy, "grad")
        gx = _empty(shp, gy)
        call("df_upsample2x_bwd", _ptr(gy), _ptr(gx), B, D, H, W, C, int(is3d), _stream())
        return gx


class _ConvGeneral(torch.autograd.Function):
    """slim.conv2d / conv3d with ANY cubic kernel and stride, TF 'SAME' on any extents (ops.py:12-16: the wrappers' own defaults are
    k=4, s=2) -- the general-shape vector-ALU kernels of conv_general.hip.  The call sites of the reference's trainers (k=3, s=1|2, even
    extents) never come here: they run on the matrix-core kernels (_ConvSame3 / _ConvSame3S2)."""

    @staticmethod
    def forward(ctx, x, w, b, leak, k, s):
        x = _prep(x, "x"); w = _prep(w, "weights"); b = _prep(b, "biases")
        nd = x.dim() - 2
        kz = k if nd == 3 else 1
        cin, cout = int(w.shape[-2]), int(w.shape[-1])
        if tuple(w.shape[:-2]) != (k,) * nd or x.shape[-1] != cin:
            raise ValueError("conv: weights %s do not match input %s / k=%d" % (tuple(w.shape), tuple(x.shape), k))
        B = int(x.shape[0])
        D = int(x.shape[1]) if nd == 3 else 1
        H, W = int(x.shape[-3]), int(x.shape[-2])
        od = [-(-D // s) if nd == 3 else 1, -(-H // s), -(-W // s)]
        y = torch.empty((B,) + tuple(od[3 - nd:]) + (cout,), dtype=torch.float32, device=x.device)
        flags = DF_CONV_BIAS | (DF_CONV_LRELU if leak is not None else 0)
        _count("conv", "general-valu k%d s%d" % (k, s), (B, D, H, W), cin, cout)
        call("df_conv_general_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, D, H, W, cin, cout, kz, k, s, flags,
             float(leak if leak is not None else 0.0), _stream())
        if ACTIVATION_FETCH is not None and leak is not None:
            ACTIVATION_FETCH.append(y)
        ctx.save_for_backward(x, w, y if leak is not None else None)
        ctx.leak = leak
        ctx.geom = (B, D, H, W, cin, cout, kz, k, s)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        B, D, H, W, cin, cout, kz, k, s = ctx.geom
        gy = _prep(gy, "grad")
        if ctx.leak is not None:
            dp = torch.empty_like(gy)
            call("df_lrelu_bwd", _ptr(gy), _ptr(y), _ptr(dp), float(ctx.leak), gy.numel(), _stream())
        else:
            dp = gy
        gw = torch.empty_like(w)
        gb = torch.empty(cout, dtype=torch.float32, device=x.device)
        call("df_conv_general_wgrad", _ptr(x), _ptr(dp), _ptr(gw), _ptr(gb), B, D, H, W, cin, cout, kz, k, s, _stream())
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            call("df_conv_general_dgrad", _ptr(dp), _ptr(w), _ptr(gx), B, D, H, W, cin, cout, kz, k, s, _stream())
        return gx, gw, gb, None, None, None


class _ResizeNN(torch.autograd.Function):
    """tf.image.resize_nearest_neighbor(align_corners=False) to ANY size per spatial axis (ops.py:66-73): src = min(floor(dst in / out), in - 1)."""

    @staticmethod
    def forward(ctx, x, new_size):
        x = _prep(x, "x")
        is3d = x.dim() == 5
        B, C = int(x.shape[0]), int(x.shape[-1])
        D = int(x.shape[1]) if is3d else 1
        H, W = int(x.shape[-3]), int(x.shape[-2])
        ns = [int(v) for v in new_size]
        if len(ns) != (3 if is3d else 2) or min(ns) <= 0:
            raise ValueError("resize: new_size %r does not match a %d-D tensor" % (new_size, x.dim()))
        Do, Ho, Wo = (ns[0], ns[1], ns[2]) if is3d else (1, ns[0], ns[1])
        y = _empty(((B, Do, Ho, Wo, C) if is3d else (B, Ho, Wo, C)), x)
        call("df_resize_nn_fwd", _ptr(x), _ptr(y), B, D, H, W, C, Do, Ho, Wo, _stream())
        ctx.geom = (B, D, H, W, C, Do, Ho, Wo, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        B, D, H, W, C, Do, Ho, Wo, shp = ctx.geom
        gy = _prep(gy, "grad")
        gx = _empty(shp, gy)
        call("df_resize_nn_bwd", _ptr(gy), _ptr(gx), B, D, H, W, C, Do, Ho, Wo, _stream())
        return gx, None


class _Curl2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, psi):
        psi = _prep(psi, "x")
        B, Y, X, C = psi.shape
        if C != 1:
            raise ValueError("curl kernel expects the 1-channel stream function [B,Y,X,1], got %s" % (tuple(psi.shape),))
        u = _empty((B, Y, X, 2), psi)
        call("df_curl2d_fwd", _ptr(psi), _ptr(u), B, Y, X, _stream())
        ctx.geom = (B, Y, X)
        return u

    @staticmethod
    def backward(ctx, gu):
        B, Y, X = ctx.geom
        gu = _prep(gu, "grad")
        g = _empty((B, Y, X, 1), gu)
        call("df_curl2d_bwd", _ptr(gu), _ptr(g), B, Y, X, _stream())
        return g


class _Jacobian2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _prep(x, "x")
        B, Y, X, C = x.shape
        if C != 2:
            raise ValueError("jacobian expects a 2-channel field [B,Y,X,2], got %s" % (tuple(x.shape),))
        j = _empty((B, Y, X, 4), x); w = _empty((B, Y, X, 1), x)
        call("df_jacobian2d_fwd", _ptr(x), _ptr(j), _ptr(w), B, Y, X, _stream())
        ctx.geom = (B, Y, X)
        ctx.set_materialize_grads(False)
        return j, w

    @staticmethod
    def backward(ctx, gj, gw):
        B, Y, X = ctx.geom
        if gj is None and gw is None:
            return None
        gj = None if gj is None else _prep(gj, "grad")
        gw = None if gw is None else _prep(gw, "grad")
        ref = gj if gj is not None else gw
        gx = _empty((B, Y, X, 2), ref)
        call("df_jacobian2d_bwd", _ptr(gj), _ptr(gw), _ptr(gx), B, Y, X, _stream())
        return gx


class _Jacobian3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, want_j, want_c):
        x = _prep(x, "x")
        B, Z, Y, X, C = x.shape
        if C != 3:
            raise ValueError("jacobian3 expects a 3-channel field [B,Z,Y,X,3], got %s" % (tuple(x.shape),))
        j = _empty((B, Z, Y, X, 9), x) if want_j else None
        c = _empty((B, Z, Y, X, 3), x) if want_c else None
        call("df_jacobian3d_fwd", _ptr(x), _ptr(j), _ptr(c), B, Z, Y, X, _stream())
        ctx.geom = (B, Z, Y, X)
        ctx.set_materialize_grads(False)
        if want_j and want_c:
            return j, c
        return j if want_j else c

    @staticmethod
    def backward(ctx, *grads):
        B, Z, Y, X = ctx.geom
        if len(grads) == 2:
            gj, gc = grads
        else:
            gj, gc = (grads[0], None) if grads[0] is not None and grads[0].shape[-1] == 9 else (None, grads[0])
        if gj is None and gc is None:
            return None, None, None
        gj = None if gj is None else _prep(gj, "grad")
        gc = None if gc is None else _prep(gc, "grad")
        ref = gj if gj is not None else gc
        gx = _empty((B, Z, Y, X, 3), ref)
        call("df_jacobian3d_bwd", _ptr(gj), _ptr(gc), _ptr(gx), B, Z, Y, X, _stream())
        return gx, None, None


class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = _prep(a, "a"); b = _prep(b, "b")
        if a.shape != b.shape:
            raise ValueError("l1_mean: shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        n = a.numel()
        out = _empty((), a)
        nbytes = query("df_l1_mean_workspace_bytes", n)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
        call("df_l1_mean_fwd", _ptr(a), _ptr(b), n, _ptr(out), _ptr(ws), nbytes, _stream())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        gout = _prep(gout, "grad")
        ga = gb = None
        if ctx.needs_input_grad[0]:
            ga = torch.empty_like(a)
            call("df_l1_mean_bwd", _ptr(a), _ptr(b), _ptr(gout), 1.0, _ptr(ga), a.numel(), _stream())
        if ctx.needs_input_grad[1]:
            gb = torch.empty_like(b)
            call("df_l1_mean_bwd", _ptr(a), _ptr(b), _ptr(gout), -1.0, _ptr(gb), a.numel(), _stream())
        return ga, gb


class _VelocityLoss(torch.autograd.Function):
    """Fused tail: (psi, x) -> (l1, jl1, u) with u = curl(psi) | jacobian3(psi)[1], l1 = mean|u - x|, jl1 = mean|J(u) - J(x)|
    (velocity_loss.hip).  x is data: no gradient."""

    @staticmethod
    def forward(ctx, psi, x):
        psi = _prep(psi, "psi"); x = _prep(x, "x")
        is3d = psi.dim() == 5
        if is3d:
            B, Z, Y, X, C = psi.shape
            if C != 3 or tuple(x.shape) != (B, Z, Y, X, 3):
                raise ValueError("velocity_loss: psi [B,Z,Y,X,3] and x [B,Z,Y,X,3] expected, got %s / %s" % (tuple(psi.shape), tuple(x.shape)))
            geom = (B, Z, Y, X)
            u = _empty((B, Z, Y, X, 3), psi)
        else:
            B, Y, X, C = psi.shape
            if C != 1 or tuple(x.shape) != (B, Y, X, 2):
                raise ValueError("velocity_loss: psi [B,Y,X,1] and x [B,Y,X,2] expected, got %s / %s" % (tuple(psi.shape), tuple(x.shape)))
            geom = (B, Y, X)
            u = _empty((B, Y, X, 2), psi)
        fn = "df_velocity_loss3d" if is3d else "df_velocity_loss2d"
        nbytes = query(fn + "_workspace_bytes", *geom)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=psi.device)
        l1, jl1 = _empty((), psi), _empty((), psi)
        call(fn + "_fwd", _ptr(psi), _ptr(x), _ptr(u), _ptr(l1), _ptr(jl1), *geom, _ptr(ws), nbytes, _stream())
        ctx.save_for_backward(u, x)
        ctx.geom = (fn, geom, nbytes, tuple(psi.shape))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(u)          # u is handed out for logging / metrics; differentiate through curl()/curl3() instead
        return l1, jl1, u

    @staticmethod
    def backward(ctx, g1, g9, _gu):
        u, x = ctx.saved_tensors
        fn, geom, nbytes, pshape = ctx.geom
        if g1 is None and g9 is None:
            return None, None
        zero = None
        if g1 is None or g9 is None:
            zero = torch.zeros((), dtype=torch.float32, device=u.device)
        g1 = _prep(g1, "grad") if g1 is not None else zero
        g9 = _prep(g9, "grad") if g9 is not None else zero
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=u.device)
        gpsi = _empty(pshape, u)
        call(fn + "_bwd", _ptr(u), _ptr(x), _ptr(g1), _ptr(g9), _ptr(gpsi), *geom, _ptr(ws), nbytes, _stream())
        return gpsi, None


# --------------------------------------------------------------------------------------------------
# the reference's call surface
# --------------------------------------------------------------------------------------------------
def lrelu(x, leak=0.2):
    """ops.py:9-10  ``tf.maximum(x, leak*x)``."""
    return _Lrelu.apply(x, leak)


def add(a, b):
    """The residual ``x += x0`` of model.py:35,40,77,82 as a HIP kernel."""
    return _Add.apply(a, b)


def concat(values, axis=-1):
    """``tf.concat([x, x0], axis=-1)`` (model.py:138,174): channel concat of two channels-last tensors."""
    if len(values) != 2 or axis not in (-1, values[0].dim() - 1):
        raise NotImplementedError("concat: two tensors along the channel axis (the encoder's skip connection)")
    return _Concat2.apply(values[0], values[1])


def sigmoid(x):
    """``tf.sigmoid`` (model.py:196,210)."""
    return _Sigmoid.apply(x)


def kl_bernoulli(z, n, rho):
    """``tf.reduce_sum(ds.kl_divergence(ds.Bernoulli(probs=rho), ds.Bernoulli(probs=tf.reduce_mean(z[:, :n], axis=0))))``
    (trainer3.py:272-277)."""
    return _KlBernoulli.apply(z, n, rho)


def mse_mean(a, b):
    """``tf.reduce_mean(tf.squared_difference(a, b))`` (trainer3.py:270)."""
    return _MseMean.apply(a, b)


FUSED_BLOCKS = True     # GeneratorBE(3) uses one fused autograd node per block (same kernels, fused backward epilogues)

# Fetch of intermediate tensors (the counterpart of adding a tensor to ``sess.run``'s fetch list): when set to a list, every
# fused generator block and every layer-by-layer conv with an lrelu appends its post-lrelu conv outputs (execution order) to it.  Used by the full-size parity tests to hand the
# oracle the lrelu sign pattern the GPU actually took.  None (default) = no fetch, no cost.
ACTIVATION_FETCH = None


# The switches above are process-wide module attributes (like the reference's single global `config`).  `options` is the one supported way
# to change them temporarily: it sets them, restores the previous values on exit -- also when the body raises, so a failing test cannot
# leak its mode into the next one -- and holds a re-entrant lock for the duration of the block, so two threads cannot interleave
# different option sets (a second thread entering `options` waits until the first leaves).
_OPTION_ATTRS = {"conv_precision": "CONV_PRECISION", "conv_algo": "CONV_ALGO", "wino3d_family": "WINO3D_FAMILY", "wino2d_family": "WINO2D_FAMILY", "wgrad_algo": "WGRAD_ALGO",
                 "thin_valu_only": "THIN_VALU_ONLY", "sign_bit_masks": "SIGN_BIT_MASKS", "fused_blocks": "FUSED_BLOCKS",
                 "dispatch_counts": "DISPATCH_COUNTS", "concurrent_wgrad_work": "CONCURRENT_WGRAD_WORK", "activation_fetch": "ACTIVATION_FETCH", "sign_bits_fetch": "SIGN_BITS_FETCH"}
_OPTION_CHOICES = {"conv_precision": ("fp32", "bf16x3"), "conv_algo": ("auto", "direct", "winograd"), "wino3d_family": ("f224", "f222"), "wino2d_family": ("auto", "f24", "f22"), "wgrad_algo": (0, 1, 2, 3, 4)}
_OPTION_LOCK = _threading.RLock()


@contextlib.contextmanager
def options(**kw):
    """``with ops.options(conv_precision="bf16x3", conv_algo="direct", wgrad_algo=1, activation_fetch=[]): ...``
    Keys: conv_precision, conv_algo, wino3d_family ("f224" | "f222"), wino2d_family ("auto" | "f24" | "f22"), wgrad_algo, thin_valu_only, sign_bit_masks, fused_blocks, dispatch_counts (a dict to count into),
    concurrent_wgrad_work (weight gradients of levels up to that many B x voxels x taps run on a second stream; 0 = serial),
    activation_fetch / sign_bits_fetch (a list to append to).  Unknown keys and out-of-range values raise before anything changes."""
    for k, v in kw.items():
        if k not in _OPTION_ATTRS:
            raise TypeError("ops.options: unknown option %r (known: %s)" % (k, ", ".join(sorted(_OPTION_ATTRS))))
        if k in _OPTION_CHOICES and v not in _OPTION_CHOICES[k]:
            raise ValueError("ops.options: %s=%r not in %r" % (k, v, _OPTION_CHOICES[k]))
    g = globals()
    with _OPTION_LOCK:
        old = {k: g[_OPTION_ATTRS[k]] for k in kw}
        try:
            for k, v in kw.items():
                g[_OPTION_ATTRS[k]] = v
            yield
        finally:
            for k, v in old.items():
                g[_OPTION_ATTRS[k]] = v


def _stack_variables(names, nd, cin, filters, device):
    """The slim variables ``names`` of a row of k=3 convs cin -> filters -> ... -> filters: [w1, b1, w2, b2, ...]."""
    wb = []
    for name in names:
        wb.append(get_variable(name + "/weights", (3,) * nd + (int(cin), int(filters)), "xavier", device))
        wb.append(get_variable(name + "/biases", (int(filters),), "zeros", device))
        cin = filters
    return wb


def gen_block(x, filters, names, nd, leak=0.2):
    """``num_conv`` x conv(k=3,s=1,act=lrelu) + ``x += x0`` (model.py:24-40 / 66-82) with slim variables ``names``."""
    return _GenBlock.apply(x, leak, *_stack_variables(names, nd, x.shape[-1], filters, x.device))


def conv_chain(x, filters, names, nd, leak=0.2):
    """``len(names)`` x conv(k=3,s=1,act=lrelu) (the encoder's per-level stack, model.py:131-136 / 167-172) as one autograd node."""
    return _ConvChain.apply(x, leak, *_stack_variables(names, nd, x.shape[-1], filters, x.device))


def up_gen_block(xc, filters, names, nd, leak=0.2):
    """``upscale(xc, 2)`` + one generator block on the up-sampled tensor (model.py:36-40 / 78-82), fused."""
    return _UpGenBlock.apply(xc, leak, *_stack_variables(names, nd, filters, filters, xc.device))


def nchw_to_nhwc(x):
    """ops.py:108-109."""
    return x.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(x):
    """ops.py:111-112."""
    return x.permute(0, 3, 1, 2).contiguous()


def int_shape(tensor):
    """ops.py:96-98."""
    return [int(s) for s in tensor.shape]


def get_conv_shape(tensor, data_format="NHWC"):
    """ops.py:100-106: always returns [N,H,W,C] (for 5-D NDHWC input: the shape itself)."""
    shape = int_shape(tensor)
    if data_format == "NCHW":
        return [shape[0], shape[2], shape[3], shape[1]]
    elif data_format == "NHWC":
        return shape


def reshape(x, h, w, c, data_format="NHWC"):
    """ops.py:198-203."""
    if data_format == "NCHW":
        return x.reshape(-1, c, h, w)
    return x.reshape(-1, h, w, c)


def _act_leak(act):
    """Map the reference's ``act`` argument onto the fused epilogue: None -> linear, lrelu -> leak 0.2."""
    if act is None:
        return None, None
    if act is lrelu:
        return 0.2, None
    return None, act          # any other callable is applied after the conv, un-fused


def _conv(x, o_dim, nd, data_format, name, k, s, act):
    k, s = int(k), int(s)
    if not (1 <= k <= 7 and 1 <= s <= 4):
        raise ValueError("conv: kernel size 1..7 and stride 1..4 (got k=%d s=%d)" % (k, s))
    if nd == 2 and data_format == "NCHW":
        x = nchw_to_nhwc(x)
    cin = int(x.shape[-1])
    lname = _layer_name(name, "Conv")
    w = get_variable(lname + "/weights", (k,) * nd + (cin, int(o_dim)), "xavier", x.device)
    b = get_variable(lname + "/biases", (int(o_dim),), "zeros", x.device)
    leak, post = _act_leak(act)
    # the reference's own call sites (k=3; s=1, or s=2 on even extents: model.py:26,42,68,84,127-143,163-179) run on the matrix cores;
    # every other (k, s, extent) of the wrapper (its defaults are k=4, s=2, ops.py:12-16) on the general-shape kernels
    fast = k == 3 and (s == 1 or (s == 2 and not any(int(d) % 2 for d in x.shape[1:-1])))
    if fast:
        y = (_ConvSame3 if s == 1 else _ConvSame3S2).apply(x, w, b, leak)
    else:
        y = _ConvGeneral.apply(x, w, b, leak, k, s)
    if post is not None:
        y = post(y)
    if nd == 2 and data_format == "NCHW":
        y = nhwc_to_nchw(y)
    return y


def conv2d(x, o_dim, data_format="NHWC", name=None, k=4, s=2, act=None):
    """ops.py:12-13 (slim.conv2d, SAME; the wrapper's defaults k=4, s=2 included)."""
    return _conv(x, o_dim, 2, data_format, name, k, s, act)


def conv3d(x, o_dim, data_format="NDHWC", name=None, k=4, s=2, act=None):
    """ops.py:15-16 (slim.conv3d, SAME)."""
    if data_format != "NDHWC":
        raise NotImplementedError("conv3d: NDHWC only (the reference never uses NCDHW)")
    return _conv(x, o_dim, 3, data_format, name, k, s, act)


def linear(x, o_dim, name=None, act=None):
    """ops.py:23-24 (slim.fully_connected)."""
    lname = _layer_name(name, "fully_connected")
    w = get_variable(lname + "/weights", (int(x.shape[-1]), int(o_dim)), "xavier", x.device)
    b = get_variable(lname + "/biases", (int(o_dim),), "zeros", x.device)
    y = _Linear.apply(x, w, b)
    return act(y) if act is not None else y


def resize_nearest_neighbor(x, new_size, data_format="NHWC"):
    """ops.py:66-73 (tf.image.resize_nearest_neighbor, align_corners=False): any target size; the exact 2x of the reference's call sites
    takes the vectorised kernel."""
    if data_format == "NCHW":
        x = nchw_to_nhwc(x)
    if tuple(int(v) for v in new_size) == (2 * x.shape[1], 2 * x.shape[2]) and x.shape[-1] % 4 == 0:
        y = _Upsample2x.apply(x)
    else:
        y = _ResizeNN.apply(x, tuple(int(v) for v in new_size))
    return nhwc_to_nchw(y) if data_format == "NCHW" else y


def upscale(x, scale, data_format="NHWC"):
    """ops.py:75-77."""
    _, h, w, _ = get_conv_shape(x, data_format)
    return resize_nearest_neighbor(x, (h * scale, w * scale), data_format)


def upscale3(x, scale):
    """ops.py:79-91: two 2-D nearest resizes == one 3-D nearest resize by `scale` (src = dst // scale); scale 2 (model.py:78) takes the
    vectorised kernel."""
    scale = int(scale)
    if scale == 2 and x.shape[-1] % 4 == 0:
        return _Upsample2x.apply(x)
    if scale < 1:
        raise ValueError("upscale3: scale must be a positive integer")
    return _ResizeNN.apply(x, tuple(int(d) * scale for d in x.shape[1:4]))


def jacobian(x, data_format="NHCW"):
    """ops.py:205-225 -> (j [..,4], w [..,1]).  (The reference default 'NHCW' is a typo that behaves as NHWC.)"""
    if data_format == "NCHW":
        x = nchw_to_nhwc(x)
    j, w = _Jacobian2d.apply(x)
    if data_format == "NCHW":
        j, w = nhwc_to_nchw(j), nhwc_to_nchw(w)
    return j, w


def jacobian3(x):
    """ops.py:227-262 -> (j [..,9], c [..,3]);  call-site idiom ``_, G_ = jacobian3(G_s)`` (trainer3.py:18)."""
    return _Jacobian3d.apply(x, True, True)


def curl3(x):
    """North-star alias for ``jacobian3(x)[1]`` that skips the unused 9-channel output (24 B/voxel, not 60)."""
    return _Jacobian3d.apply(x, False, True)


def curl(x, data_format="NHWC"):
    """ops.py:264-274."""
    if data_format == "NCHW":
        x = nchw_to_nhwc(x)
    if x.shape[-1] != 1:
        x = x[..., :1]          # the reference reads channel 0 only (x[:,1:,:,0]); e.g. the 2-channel AE output, trainer.py:361
    c = _Curl2d.apply(x)
    return nhwc_to_nchw(c) if data_format == "NCHW" else c


def divergence(x, data_format="NHWC"):
    """ops.py:276-284 (no gradient: used as a diagnostic only)."""
    if data_format == "NCHW":
        x = nchw_to_nhwc(x)
    x = _prep(x.detach(), "x")
    B, Y, X, _ = x.shape
    d = _empty((B, Y - 1, X - 1, 1), x)
    call("df_divergence2d", _ptr(x), _ptr(d), B, Y, X, _stream())
    return nhwc_to_nchw(d) if data_format == "NCHW" else d


def divergence3(x):
    """ops.py:286-290."""
    x = _prep(x.detach(), "x")
    B, Z, Y, X, _ = x.shape
    d = _empty((B, Z - 1, Y - 1, X - 1, 1), x)
    call("df_divergence3d", _ptr(x), _ptr(d), B, Z, Y, X, _stream())
    return d


def pgrad(x, data_format):
    """ops.py:292-303: pressure gradient ``(D_x p, D_y p)`` of channel 0 with the last difference replicated.  The two
    differences are exactly the curl kernel's outputs re-ordered -- ``curl(p) = (D_y p, -D_x p)`` (ops.py:267-271) and negation
    is exact -- so the stencil runs on ``df_curl2d_fwd`` / ``_bwd``; only the channel swap is a tensor view op."""
    if data_format == "NCHW":
        x = nchw_to_nhwc(x)
    c = _Curl2d.apply(x[..., :1].contiguous())
    g = torch.stack([-c[..., 1], c[..., 0]], dim=-1)
    return nhwc_to_nchw(g) if data_format == "NCHW" else g


def l1_mean(a, b):
    """``tf.reduce_mean(tf.abs(a - b))`` (trainer.py:170-171) as one fused reduction."""
    return _L1Mean.apply(a, b)


def velocity_loss(psi, x):
    """The tail of ``build_model`` as ONE fused op (SURVEY 8(b) ``velocity_loss2d/3d``; trainer.py:140-146,170-172 and the
    ground-truth Jacobian of trainer.py:29-32 / trainer3.py:18-24,49-51):  returns ``(l1, j_l1, u)`` with
    ``u = curl(psi) | jacobian3(psi)[1]``, ``l1 = reduce_mean(abs(u - x))``, ``j_l1 = reduce_mean(abs(jacobian(u)[0] - jacobian(x)[0]))``.
    Gradients flow to ``psi`` through ``l1`` and ``j_l1``; ``u`` is returned detached (for metrics / summaries)."""
    return _VelocityLoss.apply(psi, x)


# ---- fused field metrics (include/deepfluids_hip_metrics.h; csrc/metrics.hip): evaluation only, no autograd ----
class FieldMetrics(object):
    """The result of ``field_metrics``: per batch entry, over its counted cells.  ``raw`` is the int32 tensor [B, DF_FM_WORDS] the kernel
    wrote; every quantity is a view [B] of it (int32: ``count``, ``div_count``, ``argmax``; float32: the rest), on the device of the
    fields:
      ``count``          the counted cells;  ``div_count``: those of them that hold a divergence (x < X-1, y < Y-1 (, z < Z-1))
      ``sum_abs``, ``sum_sq``, ``max_abs``, ``argmax``    sum |g-x| and sum (g-x)^2 over cells and components, max |g-x| and the flat
                         cell index of it (the lowest on a tie, -1 when nothing is counted)
      ``sum_abs_x``, ``sum_sq_x``                         the same two sums of x alone
      ``sum_abs_jac``    sum |J(g)-J(x)| over cells and the D*D components of ``jacobian`` / ``jacobian3`` (what g_loss_j_l1 averages)
      ``sum_abs_div_g``, ``max_abs_div_g``, ``sum_abs_div_x``, ``max_abs_div_x``   of ``divergence`` / ``divergence3`` of g and of x
    The derived properties are float64 [B], computed from these without another pass: ``l1`` = sum_abs / (count D), ``rmse`` =
    sqrt(sum_sq / (count D)), ``rel_l1`` = sum_abs / sum_abs_x, ``rel_l2`` = sqrt(sum_sq / sum_sq_x), ``jacobian_l1`` = sum_abs_jac /
    (count D D), ``div_l1_g`` / ``div_l1_x`` = sum_abs_div_* / div_count.  An entry with nothing counted has zero sums and ``nan`` means;
    ``rel_*`` of an entry whose x sums are 0 are ``nan``."""
    INTS = ("count", "div_count", "argmax")
    FLOATS = ("sum_abs", "sum_sq", "max_abs", "sum_abs_x", "sum_sq_x", "sum_abs_jac", "sum_abs_div_g", "max_abs_div_g", "sum_abs_div_x",
              "max_abs_div_x")
    QUANTITIES = INTS + FLOATS
    DERIVED = ("l1", "rmse", "rel_l1", "rel_l2", "jacobian_l1", "div_l1_g", "div_l1_x")
    LINEAR = ("max_abs", "max_abs_div_g", "max_abs_div_x", "l1", "rmse", "jacobian_l1", "div_l1_g", "div_l1_x")   # scale with the velocity unit

    def __init__(self, raw, dim):
        if raw.dtype != torch.int32 or raw.dim() != 2 or raw.shape[1] != _lib.DF_FM_WORDS or dim not in (2, 3):
            raise ValueError("FieldMetrics: raw must be int32 [B, %d] and dim 2 or 3" % _lib.DF_FM_WORDS)
        self.raw, self.dim = raw, dim

    def __getattr__(self, name):
        if name in FieldMetrics.QUANTITIES:
            word = getattr(_lib, "DF_FM_" + name.upper())
            return (self.raw if name in FieldMetrics.INTS else self.raw.view(torch.float32))[:, word]
        raise AttributeError(name)

    @property
    def batch(self):
        return self.raw.shape[0]

    def cpu(self):
        return FieldMetrics(self.raw.cpu(), self.dim)

    @staticmethod
    def cat(parts):
        """the entries of several results in one (still on the device)"""
        return FieldMetrics(torch.cat([p.raw for p in parts], dim=0), parts[0].dim)

    def _n(self, power):
        return self.count.double() * float(self.dim ** power)

    @staticmethod
    def _rel(num, den):
        return torch.where(den == 0, torch.full_like(num, float("nan")), num / den)

    @property
    def l1(self):
        return self.sum_abs.double() / self._n(1)

    @property
    def rmse(self):
        return torch.sqrt(self.sum_sq.double() / self._n(1))

    @property
    def rel_l1(self):
        return self._rel(self.sum_abs.double(), self.sum_abs_x.double())

    @property
    def rel_l2(self):
        return torch.sqrt(self._rel(self.sum_sq.double(), self.sum_sq_x.double()))

    @property
    def jacobian_l1(self):
        return self.sum_abs_jac.double() / self._n(2)

    @property
    def div_l1_g(self):
        return self.sum_abs_div_g.double() / self.div_count.double()

    @property
    def div_l1_x(self):
        return self.sum_abs_div_x.double() / self.div_count.double()


def _field_metrics_args(g, x, mask, workspace):
    """the checks of ``field_metrics`` that need no device: ``(dim, extents [B,Z,Y,X], mask as uint8 | None, mask_per_entry, workspace bytes)``"""
    who = "field_metrics"
    for t, name in ((g, "g"), (x, "x")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor on the MI355X (got %r)" % (who, name, type(t)))
    if g.dim() not in (4, 5) or g.shape[-1] != g.dim() - 2:
        raise ValueError("%s expects velocity fields [B,Y,X,2] or [B,Z,Y,X,3], got g %s" % (who, tuple(g.shape)))
    if tuple(x.shape) != tuple(g.shape):
        raise ValueError("%s: g %s and x %s disagree in shape" % (who, tuple(g.shape), tuple(x.shape)))
    for t, name in ((g, "g"), (x, "x")):
        if t.dtype != torch.float32:
            raise ValueError("%s: %s must be float32 (g and x in the same dtype), got %s" % (who, name, t.dtype))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous (strides %s for shape %s)" % (who, name, tuple(t.stride()), tuple(t.shape)))
    dim = g.dim() - 2
    spatial = tuple(int(n) for n in g.shape[1:-1])
    B = int(g.shape[0])
    if B < 1 or min(spatial) < 2:
        raise ValueError("%s: the forward differences need every extent >= 2 (and B >= 1), got %s" % (who, tuple(g.shape)))
    ext = [B] + ([1] if dim == 2 else []) + list(spatial)
    need = query("df_field_metrics_workspace_bytes", dim, *ext)
    if need < 0:
        raise ValueError("%s: %s cells per entry do not fit the int32 cell index" % (who, " x ".join(str(n) for n in spatial)))
    per_entry = 0
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError("%s: mask must be a uint8 (or bool) tensor, got %s" % (who, getattr(mask, "dtype", type(mask))))
        if tuple(mask.shape) not in (spatial, (B,) + spatial):
            raise ValueError("%s: mask must be [(Z,)Y,X] = %s (shared by the batch) or [B,(Z,)Y,X], got %s" % (who, spatial, tuple(mask.shape)))
        if not mask.is_contiguous():
            raise ValueError("%s: mask must be contiguous" % who)
        # ([B,..] with B = 1 and the shared form hold the same bytes)
        per_entry = 1 if mask.dim() == dim + 1 else 0
        mask = mask.view(torch.uint8)
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
            raise ValueError("%s: workspace must be a contiguous tensor of >= %d bytes (field_metrics_workspace)" % (who, need))
    return dim, ext, mask, per_entry, need


def field_metrics_workspace(g):
    """The scratch ``field_metrics`` needs for fields of the shape of ``g`` (80 bytes per 1024 cells); reusable across calls."""
    dim = g.dim() - 2
    ext = [int(g.shape[0])] + ([1] if dim == 2 else []) + [int(n) for n in g.shape[1:-1]]
    need = query("df_field_metrics_workspace_bytes", dim, *ext)
    if need < 0:
        raise ValueError("field_metrics_workspace: no workspace for fields of shape %s" % (tuple(g.shape),))
    return torch.empty((need // 8,), dtype=torch.float64, device=g.device)


def field_metrics(g, x, mask=None, workspace=None):
    """How well a generated velocity field ``g`` reproduces the ground truth ``x`` ([B,Y,X,2] or [B,Z,Y,X,3], float32, contiguous), per
    batch entry, as ONE fused pass: each field is read once, nothing the size of a field is allocated.  Returns a ``FieldMetrics``:
    the counted cells, sum |g-x|, sum (g-x)^2, max |g-x| and its cell, sum |x|, sum x^2, sum |J(g)-J(x)| with the forward-difference
    Jacobian of ``jacobian`` / ``jacobian3`` (the quantity g_loss_j_l1 averages), and the sum and max of |div g| and |div x| with the
    divergence of ``divergence`` / ``divergence3`` -- and, derived from them, ``l1``, ``rmse``, ``rel_l1``, ``rel_l2``,
    ``jacobian_l1``, ``div_l1_g``, ``div_l1_x``.
    ``mask``: uint8 (or bool) [(Z,)Y,X], shared by the batch, or [B,(Z,)Y,X]; a cell is counted where it is non-zero (everywhere without
    a mask).  A stencil value belongs to the cell where the stencil ops store it and is counted with that cell, whatever the mask says
    about the neighbours it reads.
    include/deepfluids_hip_metrics.h fixes the arithmetic and the order of every sum (fp32 per thread, fp64 across threads and
    workgroups, no atomics): two calls give the same bits, an entry's numbers do not depend on the rest of the batch, and
    tests/field_metrics_ref.py restates it in NumPy.  ``workspace``: see ``field_metrics_workspace``.  No autograd."""
    dim, ext, mask, per_entry, need = _field_metrics_args(g, x, mask, workspace)
    with torch.no_grad():
        g, x = _prep(g.detach(), "g"), _prep(x.detach(), "x")
        if x.device != g.device or (mask is not None and mask.device != g.device) or (workspace is not None and workspace.device != g.device):
            raise ValueError("field_metrics: g, x, mask and workspace must be on one device")
        ws = workspace if workspace is not None else field_metrics_workspace(g)
        if ws.data_ptr() % 8:
            raise ValueError("field_metrics: workspace must be 8-byte aligned")
        raw = torch.empty((ext[0], _lib.DF_FM_WORDS), dtype=torch.int32, device=g.device)
        call("df_field_metrics%dd" % dim, _ptr(g), _ptr(x), _ptr(mask), per_entry, _ptr(raw), _ptr(ws), ws.numel() * ws.element_size(),
             *(ext[:1] + ext[-dim:] + [_stream()]))
        return FieldMetrics(raw, dim)


# ---- SSIM / MS-SSIM (include/deepfluids_hip_ssim.h; csrc/ssim.hip; ops.py:382-501): evaluation only, no autograd ----
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # ops.py:467
_SSIM_TAPS = {}
_SSIM_WEIGHTS = {}


def _ssim_taps(size, sigma):
    """the normalised 1-D factor of ``fspecial_gauss(size, sigma, .)`` as the header defines it: fp64, rounded to fp32 once.
    ``(float32 array [size], the same as a ctypes array)``"""
    key = (int(size), float(sigma))
    if key not in _SSIM_TAPS:
        u = np.arange(size, dtype=np.float64) - size // 2 + (0.5 if size % 2 == 0 else 0.0)
        e = np.exp(-(u * u) / (2.0 * float(sigma) ** 2))
        t = (e / e.sum()).astype(np.float32)
        if not np.isfinite(t).all():
            raise ValueError("ssim: a window of %d taps with sigma %r is not finite" % (size, sigma))
        _SSIM_TAPS[key] = (t, (ctypes.c_float * int(size))(*[float(v) for v in t]))
    return _SSIM_TAPS[key]


def fspecial_gauss(size, sigma, channels):
    """ops.py:382-407: the Gaussian window [size,size,C,C], normalised over ALL its entries (so every channel pair holds the 2-D
    window over C^2), with the half-cell offset of an even ``size``.  Computed in fp64 on the host, float32 CPU tensor."""
    size, channels = int(size), int(channels)
    if size < 1 or channels < 1 or not float(sigma) > 0:
        raise ValueError("fspecial_gauss: size and channels must be >= 1 and sigma > 0, got %r, %r, %r" % (size, sigma, channels))
    u = np.arange(size, dtype=np.float64) - size // 2 + (0.5 if size % 2 == 0 else 0.0)
    g = np.exp(-(u[:, None] ** 2 + u[None, :] ** 2) / (2.0 * float(sigma) ** 2))
    g = np.broadcast_to(g[:, :, None, None], (size, size, channels, channels))
    return torch.from_numpy((g / g.sum()).astype(np.float32))


def _ssim_args(who, img1, img2, filter_size, filter_sigma, min_val, max_val):
    """the checks of the SSIM entry points that need no device: ``(N, H, W, C, size, sigma)``"""
    for t, name in ((img1, "img1"), (img2, "img2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor on the MI355X (got %r)" % (who, name, type(t)))
    if img1.dim() != 4 or not 1 <= img1.shape[-1] <= _lib.DF_SSIM_MAX_CHANNELS or min(img1.shape) < 1:
        raise ValueError("%s expects images [N,H,W,C] with C in 1..%d, got img1 %s" % (who, _lib.DF_SSIM_MAX_CHANNELS, tuple(img1.shape)))
    if tuple(img2.shape) != tuple(img1.shape):
        raise ValueError("%s: img1 %s and img2 %s disagree in shape" % (who, tuple(img1.shape), tuple(img2.shape)))
    for t, name in ((img1, "img1"), (img2, "img2")):
        if t.dtype != torch.float32:
            raise ValueError("%s: %s must be float32 (both images in the same dtype), got %s" % (who, name, t.dtype))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous (strides %s for shape %s)" % (who, name, tuple(t.stride()), tuple(t.shape)))
        if t.requires_grad:
            raise NotImplementedError("%s: %s requires grad; SSIM has no backward here (detach it: evaluation only)" % (who, name))
    if int(filter_size) != filter_size or filter_size < 1:
        # the reference's filter_size = 0 branch does not run (`mu1 = img1, mu2 = img2` unpacks a tensor into two names)
        raise ValueError("%s: filter_size must be an integer >= 1, got %r" % (who, filter_size))
    if not float(filter_sigma) > 0:
        raise ValueError("%s: filter_sigma must be > 0, got %r" % (who, filter_sigma))
    if not (math.isfinite(min_val) and math.isfinite(max_val)) or np.float32(max_val) == np.float32(min_val):
        raise ValueError("%s: min_val and max_val must be finite and differ, got %r, %r" % (who, min_val, max_val))
    N, H, W, C = (int(n) for n in img1.shape)
    size = min(int(filter_size), H, W)
    if size > _lib.DF_SSIM_MAX_SIZE:
        raise ValueError("%s: a window of %d taps; the kernel's staged tile holds at most %d" % (who, size, _lib.DF_SSIM_MAX_SIZE))
    if query("df_ssim_workspace_bytes", N, H, W, int(filter_size)) < 0:
        raise ValueError("%s: images of shape %s do not fit the int32 index of the kernel" % (who, tuple(img1.shape)))
    return N, H, W, C, size, float(filter_sigma) * size / int(filter_size)


class SSIMWorkspace(object):
    """What repeated SSIM calls on images of one shape need (``ssim_workspace``): per level the tile sums, the output rows, the two
    map planes when asked for and the pooled pair that is the next level's input, and the fp64 means [levels, groups, 2]."""

    def __init__(self, shape, device, levels, filter_size, groups, maps=False):
        N, H, W, C = (int(n) for n in shape)
        self.shape, self.levels, self.filter_size, self.groups, self.device = (N, H, W, C), int(levels), int(filter_size), int(groups), torch.device(device)
        if N % self.groups:
            raise ValueError("ssim_workspace: %d images are not %d groups" % (N, self.groups))
        self.level = []
        for k in range(self.levels):
            need = query("df_ssim_workspace_bytes", N, H, W, self.filter_size)
            if need < 0:
                raise ValueError("ssim_workspace: no workspace for images of shape %s" % ((N, H, W, C),))
            size = min(self.filter_size, H, W)
            lv = {"shape": (N, H, W, C), "ws": torch.empty((need // 8,), dtype=torch.float64, device=device),
                  "out": torch.empty((N, _lib.DF_SSIM_WORDS), dtype=torch.int32, device=device), "maps": None, "pool": None}
            if maps:
                lv["maps"] = (torch.empty((N, H - size + 1, W - size + 1), dtype=torch.float32, device=device),
                              torch.empty((N, H - size + 1, W - size + 1), dtype=torch.float32, device=device))
            H, W = (H + 1) // 2, (W + 1) // 2
            if k < self.levels - 1:
                lv["pool"] = (torch.empty((N, H, W, C), dtype=torch.float32, device=device), torch.empty((N, H, W, C), dtype=torch.float32, device=device))
            self.level.append(lv)
        self.mean = torch.empty((self.levels, self.groups, 2), dtype=torch.float64, device=device)


def ssim_workspace(x, multiscale=False, filter_size=11):
    """The buffers ``field_ssim(g, x, multiscale=...)`` needs for fields of the shape of ``x`` ([B,Y,X,C] or [B,Z,Y,X,C]); reusable
    across calls, so that a sweep allocates nothing per batch."""
    if x.dim() not in (4, 5):
        raise ValueError("ssim_workspace expects fields [B,Y,X,C] or [B,Z,Y,X,C], got %s" % (tuple(x.shape),))
    B = int(x.shape[0])
    shape = (B * int(np.prod(x.shape[1:-3])),) + tuple(int(n) for n in x.shape[-3:])
    return SSIMWorkspace(shape, x.device, len(MS_SSIM_WEIGHTS) if multiscale else 1, 11 if multiscale else filter_size, B)


def _ssim_run(who, a, b, ws, filter_sigma, k1, k2, min_val, max_val):
    """the levels of ``ws`` on the images a, b: one fused launch (and its small second one) per level, each but the last also
    writing the next level's images; then the group means of every level.  Nothing is read back."""
    a, b = _prep(a, "img1"), _prep(b, "img2")
    if b.device != a.device or ws.device != a.device:
        raise ValueError("%s: the images and the workspace must be on one device" % who)
    if tuple(a.shape) != ws.shape:
        raise ValueError("%s: the workspace is for images %s, got %s" % (who, ws.shape, tuple(a.shape)))
    s = _stream()
    for k, lv in enumerate(ws.level):
        N, H, W, C = lv["shape"]
        size = min(ws.filter_size, H, W)
        taps = _ssim_taps(size, float(filter_sigma) * size / ws.filter_size)[1]
        maps, pool = lv["maps"] or (None, None), lv["pool"] or (None, None)
        call("df_ssim", _ptr(a), _ptr(b), taps, _ptr(maps[0]), _ptr(maps[1]), _ptr(pool[0]), _ptr(pool[1]), _ptr(lv["out"]), _ptr(lv["ws"]),
             lv["ws"].numel() * 8, N, H, W, C, ws.filter_size, float(k1), float(k2), float(min_val), float(max_val), s)
        call("df_ssim_group_mean", _ptr(lv["out"]), _ptr(ws.mean[k]), ws.groups, N // ws.groups, s)
        a, b = pool
    return ws.mean


def _ms_combine(mean):
    """mean [5, G, 2] fp64 (ssim, cs per level) -> [G] fp64: prod(mcs[0:4] ** w[0:4]) * mssim[4] ** w[4], on the device"""
    key = mean.device
    if key not in _SSIM_WEIGHTS:
        _SSIM_WEIGHTS[key] = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64, device=mean.device)
    w = _SSIM_WEIGHTS[key]
    return torch.prod(mean[:-1, :, 1] ** w[:-1, None], dim=0) * mean[-1, :, 0] ** w[-1]


def ssim(img1, img2, mean_metric=True, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, min_val=-1.0, max_val=1.0):
    """ops.py:410-462: the structural similarity of two image batches [N,H,W,C] (float32, contiguous, C in 1..4, values in
    [min_val, max_val]) as ONE fused pass (include/deepfluids_hip_ssim.h fixes every operation and the order of every sum;
    tests/ssim_ref.py restates it).  The window shrinks to ``min(filter_size, H, W)`` taps (at most 11 here) and sigma with it.
    ``mean_metric=True``: a 0-d float32 tensor on the device, the mean over the whole batch: the images' fp64 totals added and
    divided by N H' W', rounded once.  ``mean_metric=False``: the reference's dict, ``ssim_map`` and ``cs_map`` [N,H',W',C] (the
    reference's C channels are equal: an expanded view of the one plane) and ``g``, the window [size,size,C,C].
    As in the reference every output channel is 1/C^2 times the sum over the input channels (the window is normalised over all its
    C^2 channel pairs).  No autograd: inputs that require grad are refused."""
    N, H, W, C, size, sigma = _ssim_args("ssim", img1, img2, filter_size, filter_sigma, min_val, max_val)
    with torch.no_grad():
        _prep(img1, "img1"), _prep(img2, "img2")
        ws = SSIMWorkspace((N, H, W, C), img1.device, 1, filter_size, 1, maps=not mean_metric)
        mean = _ssim_run("ssim", img1, img2, ws, filter_sigma, k1, k2, min_val, max_val)
        if mean_metric:
            return mean[0, 0, 0].float()
        sm, cm = ws.level[0]["maps"]
        return {"ssim_map": sm.unsqueeze(-1).expand(-1, -1, -1, C), "cs_map": cm.unsqueeze(-1).expand(-1, -1, -1, C),
                "g": fspecial_gauss(size, sigma, C).to(img1.device)}


def ms_ssim(img1, img2, mean_metric=True, min_val=-1.0, max_val=1.0):
    """ops.py:465-501: multi-scale SSIM with the reference's five weights.  Each level is one fused launch that also writes the 2x2
    average-pooled images ('SAME': ceil(H/2) x ceil(W/2), an edge cell averages what exists) the next level reads; the last writes
    none.  The levels' batch means (fp64) are combined on the device, prod(mcs[0:4] ** w[0:4]) * mssim[4] ** w[4], without a host
    read; a 0-d float32 tensor either way (the reference's ``mean_metric`` averages a scalar).  NaN where the reference gives NaN:
    a non-positive level mean (cs of levels 0..3, ssim of level 4) under a fractional power."""
    N, H, W, C, _, _ = _ssim_args("ms_ssim", img1, img2, 11, 1.5, min_val, max_val)
    with torch.no_grad():
        _prep(img1, "img1"), _prep(img2, "img2")
        ws = SSIMWorkspace((N, H, W, C), img1.device, len(MS_SSIM_WEIGHTS), 11, 1)
        return _ms_combine(_ssim_run("ms_ssim", img1, img2, ws, 1.5, 0.01, 0.03, min_val, max_val))[0].float()


def field_ssim(g, x, multiscale=False, workspace=None, **ssim_kwargs):
    """SSIM (``multiscale``: MS-SSIM) of a generated field ``g`` against the ground truth ``x``, per batch ENTRY: float64 [B] on the
    device.  Fields are [B,Y,X,C] or [B,Z,Y,X,C]; a 3-D field is taken as its B Z slices [Y,X,C] (a view; window and pooling stay
    in-plane), and an entry's mean is over the pixels of all its slices: the slices' fp64 totals added, divided by Z H' W'
    (``df_ssim_group_mean``).  ``ssim_kwargs``: ``filter_size, filter_sigma, k1, k2, min_val, max_val`` of ``ssim`` (``multiscale``:
    ``min_val, max_val`` only).  ``workspace``: see ``ssim_workspace``.  No autograd."""
    who = "field_ssim"
    allowed = ("min_val", "max_val") if multiscale else ("filter_size", "filter_sigma", "k1", "k2", "min_val", "max_val")
    for k in ssim_kwargs:
        if k not in allowed:
            raise TypeError("%s: unexpected argument %r (multiscale=%s takes %s)" % (who, k, bool(multiscale), ", ".join(allowed)))
    kw = dict(filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, min_val=-1.0, max_val=1.0)
    kw.update(ssim_kwargs)
    for t, name in ((g, "g"), (x, "x")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor on the MI355X (got %r)" % (who, name, type(t)))
    if g.dim() not in (4, 5):
        raise ValueError("%s expects fields [B,Y,X,C] or [B,Z,Y,X,C], got g %s" % (who, tuple(g.shape)))
    if tuple(x.shape) != tuple(g.shape):
        raise ValueError("%s: g %s and x %s disagree in shape" % (who, tuple(g.shape), tuple(x.shape)))
    for t, name in ((g, "g"), (x, "x")):
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous (strides %s for shape %s)" % (who, name, tuple(t.stride()), tuple(t.shape)))
    B = int(g.shape[0])
    a, b = g.reshape((-1,) + tuple(g.shape[-3:])), x.reshape((-1,) + tuple(x.shape[-3:]))      # views: both are contiguous
    _ssim_args(who, a, b, kw["filter_size"], kw["filter_sigma"], kw["min_val"], kw["max_val"])
    with torch.no_grad():
        _prep(a, "g"), _prep(b, "x")
        ws = workspace if workspace is not None else ssim_workspace(g, multiscale, kw["filter_size"])
        if not isinstance(ws, SSIMWorkspace) or ws.groups != B or ws.levels != (len(MS_SSIM_WEIGHTS) if multiscale else 1) or \
                ws.filter_size != int(kw["filter_size"]):
            raise ValueError("%s: the workspace was made for another call (ssim_workspace(x, multiscale, filter_size))" % who)
        mean = _ssim_run(who, a, b, ws, kw["filter_sigma"], kw["k1"], kw["k2"], kw["min_val"], kw["max_val"])
        return _ms_combine(mean) if multiscale else mean[0, :, 0].clone()


# ---- uint8 image views (ops.py:138-188): inference only, no autograd, torch.uint8 out ----
def add_channels(x, num_ch=1, data_format="NHWC"):
    """ops.py:138-144: append ``num_ch`` zero channels."""
    b, h, w, _ = get_conv_shape(x, data_format)
    if data_format == "NCHW":
        return torch.cat([x, torch.zeros((b, num_ch, h, w), dtype=x.dtype, device=x.device)], dim=1)
    return torch.cat([x, torch.zeros((b, h, w, num_ch), dtype=x.dtype, device=x.device)], dim=-1)


def remove_channels(x, data_format="NHWC"):
    """ops.py:146-152: keep the first three channels."""
    return x[:, :3] if data_format == "NCHW" else x[..., :3]


def _u8(shape, like):
    return torch.empty(shape, dtype=torch.uint8, device=like.device)


def denorm_img(norm, data_format="NHWC"):
    """ops.py:154-161: [-1,1] -> uint8 [B,H,W,1|3] (always channels-last); 2 channels get a zero third one, more than 3 lose the rest --
    folded into the one kernel together with the layout change."""
    x = _prep(norm.detach(), "norm")
    if x.dim() != 4:
        raise ValueError("denorm_img expects a 4-D tensor, got %s" % (tuple(x.shape),))
    B, H, W, C = get_conv_shape(x, data_format)
    out = _u8((B, H, W, 3 if (C == 2 or C > 3) else C), x)
    call("df_denorm_img2d", _ptr(x), _ptr(out), B, H, W, C, 1 if data_format == "NCHW" else 0, _stream())
    return out


_VIEW_KEYS = ("xy", "zy", "xym", "zym")


def _views3(x, keys):
    x = _prep(x.detach(), "x")
    if x.dim() != 5:
        raise ValueError("plane views expect [B,Z,Y,X,C], got %s" % (tuple(x.shape),))
    B, Z, Y, X, C = x.shape
    out = {k: _u8((B, Y, X if k[0] == "x" else Z, C), x) for k in keys}
    call("df_plane_views3d", _ptr(x), *([_ptr(out.get(k)) for k in _VIEW_KEYS] + [B, Z, Y, X, C, _stream()]))
    return out


def plane_view(x, xy_plane=True, project=True):
    """ops.py:163-181: one uint8 view of x [B,Z,Y,X,C] -- the z mean / the Z//2 slice [B,Y,X,C], or the x mean / the X//2 slice with y as
    the row [B,Y,Z,C]."""
    k = ("xy" if xy_plane else "zy") + ("" if project else "m")
    return _views3(x, (k,))[k]


def denorm_img3(x):
    """ops.py:183-188: {'xy', 'zy', 'xym', 'zym'} from ONE pass over x."""
    return _views3(x, _VIEW_KEYS)


def velocity_views3(u):
    """(denorm_img3(u), denorm_img3(curl3(u))) -- the reference's ``G`` and ``G_vort`` (trainer3.py:22-25) -- from one pass over u, the
    curl never written; bit-identical to the composition.  (No reference name: TF fuses nothing here.)"""
    u = _prep(u.detach(), "u")
    if u.dim() != 5 or u.shape[-1] != 3:
        raise ValueError("velocity_views3 expects a 3-channel field [B,Z,Y,X,3], got %s" % (tuple(u.shape),))
    B, Z, Y, X, _ = u.shape
    ou = {k: _u8((B, Y, X if k[0] == "x" else Z, 3), u) for k in _VIEW_KEYS}
    oc = {k: _u8((B, Y, X if k[0] == "x" else Z, 3), u) for k in _VIEW_KEYS}
    call("df_velocity_views3d", _ptr(u), *([_ptr(ou[k]) for k in _VIEW_KEYS] + [_ptr(oc[k]) for k in _VIEW_KEYS] + [B, Z, Y, X, _stream()]))
    return ou, oc


# ---- density advection through a velocity field (the advect() mode of the reference's scene scripts, scene/smoke_pos_size.py:45-109):
#      inference only, no autograd.  The step is defined in include/deepfluids_hip.h; mantaflow, which the reference calls for it, cannot
#      be run here, so bit parity with it is not claimed ----
def _advect_dims(density, vel):
    d = _prep(density.detach(), "density")
    v = _prep(vel.detach(), "vel")
    if d.dim() not in (3, 4):
        raise ValueError("advect expects a density [B,(Z,)Y,X], got %s" % (tuple(d.shape),))
    nd = d.dim() - 1
    if tuple(v.shape) != tuple(d.shape) + (nd,):
        raise ValueError("advect expects a velocity %s for a density %s, got %s" % (tuple(d.shape) + (nd,), tuple(d.shape), tuple(v.shape)))
    return d, v, nd


def _source_mask(source, like):
    m = source if isinstance(source, torch.Tensor) else torch.as_tensor(np.asarray(source))
    if not m.is_cuda:
        m = m.to(like.device)
    if m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8)
    if tuple(m.shape) != tuple(like.shape):
        m = m.expand(like.shape)
    return m.contiguous()


class SphereSource(object):
    """A sphere source whose centre is read from device memory: ``centers`` [B,D] in cell units (x, y[, z]), one sphere per batch entry,
    or [T,B,D] for the sequence forms (``advect_sequence``, ``simulate_smoke``: frame t stamps ``centers[t]``); ``radius`` in cells.  A
    tensor, or anything ``torch.as_tensor`` converts -- once, here.  ``source=`` of ``advect``, ``advect_sequence``, ``smoke_step`` and
    ``simulate_smoke`` accepts it beside a mask; it goes through ``df_density_sphere_source*``, no mask is built on the host."""

    def __init__(self, centers, radius):
        c = centers if isinstance(centers, torch.Tensor) else torch.as_tensor(np.asarray(centers, dtype=np.float32))
        if c.dim() not in (2, 3) or c.shape[-1] not in (2, 3):
            raise ValueError("SphereSource: centers must be [B,D] or [T,B,D] with D = 2 | 3, got %s" % (tuple(c.shape),))
        self.centers = c.detach().to(dtype=torch.float32)
        self.radius = float(radius)

    def frame(self, t):
        """the source of frame ``t``: [T,B,D] centres are indexed, [B,D] centres serve every frame"""
        if self.centers.dim() == 2:
            return self
        if not 0 <= t < self.centers.shape[0]:
            raise ValueError("SphereSource: frame %d of %d" % (t, self.centers.shape[0]))
        return SphereSource(self.centers[t], self.radius)

    def on(self, like):
        """centres [B,D] on ``like``'s device, contiguous, checked against its shape [B,(Z,)Y,X]"""
        c = self.centers
        if c.dim() != 2 or tuple(c.shape) != (like.shape[0], like.dim() - 1):
            raise ValueError("SphereSource: centres %s do not fit a density %s (one step takes [B,D])" % (tuple(c.shape), tuple(like.shape)))
        return c.to(like.device).contiguous()


class CylinderShape(object):
    """mantaflow's ``Cylinder(center, radius, z)``, one per batch entry, packed for the kernels: ``centers`` and ``z`` (the HALF-axis
    vector) are [B,D] or [D] (then shared by the batch) in cell units, xyz order; ``radius`` a float or [B].  Holds ``packed``
    [B | 1, 2D+1] = (centre, z, radius) float32, moved to the device of the grid it is used on.  A zero-length ``z`` is refused here
    when the numbers are on the host; on the device such an entry, like one that holds a NaN, stamps nothing."""

    def __init__(self, centers, z, radius):
        def as_t(x):
            return x.detach().to(dtype=torch.float32) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
        c, zz, r = as_t(centers), as_t(z), as_t(radius)
        D = c.shape[-1] if c.dim() else 0
        if c.dim() not in (1, 2) or D not in (2, 3) or zz.dim() not in (1, 2) or zz.shape[-1] != D or r.dim() > 1:
            raise ValueError("CylinderShape: centers and z must be [B,D] or [D] with D = 2 | 3 and radius a float or [B], got %s, %s, %s" %
                             (tuple(c.shape), tuple(zz.shape), tuple(r.shape)))
        Bs = set([c.shape[0]] if c.dim() == 2 else []) | set([zz.shape[0]] if zz.dim() == 2 else []) | set([r.shape[0]] if r.dim() == 1 else [])
        if len(Bs - {1}) > 1:
            raise ValueError("CylinderShape: centers, z and radius disagree about the batch: %s" % sorted(Bs))
        B = max(Bs) if Bs else 1
        dev = next((t.device for t in (c, zz, r) if t.is_cuda), c.device)
        c, zz, r = c.to(dev).reshape(-1, D).expand(B, D), zz.to(dev).reshape(-1, D).expand(B, D), r.to(dev).reshape(-1, 1).expand(B, 1)
        if not zz.is_cuda and bool((zz == 0).all(dim=-1).any()):
            raise ValueError("CylinderShape: a half-axis z of length zero")
        self.packed = torch.cat([c, zz, r], dim=-1).contiguous()
        self._on = None

    @property
    def dim(self):
        return (self.packed.shape[-1] - 1) // 2

    def entry(self, b):
        """the cylinder of batch entry ``b`` alone ([1, 2D+1])"""
        out = CylinderShape.__new__(CylinderShape)
        out.packed = self.packed if self.packed.shape[0] == 1 else self.packed[b:b + 1].contiguous()
        out._on = None
        return out

    def on(self, like):
        """``packed`` [B, 2D+1] on ``like``'s device, contiguous, for a grid ``like`` [B,(Z,)Y,X,...] of D axes"""
        B, dev = like.shape[0], like.device
        if self._on is not None and self._on.shape[0] == B and self._on.device == dev:
            return self._on
        if self.packed.shape[0] not in (1, B):
            raise ValueError("CylinderShape: %d cylinders do not fit a batch of %d" % (self.packed.shape[0], B))
        self._on = self.packed.to(dev).expand(B, self.packed.shape[-1]).contiguous()
        return self._on


class NoiseField(object):
    """The parameters of mantaflow's ``NoiseField`` as scene/smoke3_vel_buo.py:185-191 sets them (the defaults here), for THIS
    project's seeded lattice value noise (include/deepfluids_hip.h) -- NOT mantaflow's wavelet noise, which is read from a tile file and
    cannot be restated.  ``pos_scale`` / ``pos_offset``: a number or D numbers (xyz).  A plain holder."""

    def __init__(self, pos_scale=45, val_offset=0.75, val_scale=1, time_anim=0.2, clamp=True, clamp_neg=0, clamp_pos=1, pos_offset=0,
                 seed=0x9E3779B9):
        self.pos_scale, self.pos_offset = pos_scale, pos_offset
        self.val_offset, self.val_scale, self.time_anim = float(val_offset), float(val_scale), float(time_anim)
        self.clamp, self.clamp_neg, self.clamp_pos = bool(clamp), float(clamp_neg), float(clamp_pos)
        self.seed = int(seed) & 0xFFFFFFFF

    def vec(self, name, dim):
        v = np.asarray(getattr(self, name), dtype=np.float32).reshape(-1)
        if v.size not in (1, dim):
            raise ValueError("NoiseField: %s must be a number or %d numbers, got %r" % (name, dim, getattr(self, name)))
        return [float(x) for x in np.broadcast_to(v, (dim,))]

    def params(self, dim, extent_x):
        """the ``df_noise_params`` of a grid of ``dim`` axes whose x extent is ``extent_x``"""
        from ._lib import NoiseParams
        q = NoiseParams()
        for a, (sc, of) in enumerate(zip(self.vec("pos_scale", dim), self.vec("pos_offset", dim))):
            q.pos_scale[a], q.pos_offset[a] = sc, of
        q.time_anim, q.val_offset, q.val_scale = self.time_anim, self.val_offset, self.val_scale
        q.clamp, q.clamp_neg, q.clamp_pos = int(self.clamp), self.clamp_neg, self.clamp_pos
        q.seed = self.seed
        q.inv_extent = float(np.float32(1.0) / np.float32(extent_x))
        return q


class NoiseInflow(object):
    """``densityInflow(flags, density, noise, shape, scale, sigma)`` of scene/smoke3_vel_buo.py:222 as a source: ``shape`` a
    ``CylinderShape``, ``noise`` a ``NoiseField``.  ``source=`` of ``advect``, ``advect_sequence``, ``smoke_step`` and ``simulate_smoke``
    accepts it beside a mask and a ``SphereSource``; ``source_value`` does not apply to it (``scale`` does).  Frame t of the sequence forms
    evaluates the noise at ``time = t * time_step`` (the ``dt`` of the call when ``time_step`` is None), as the script's ``s.step()``
    advances the solver time; the single-step forms take ``time=``.  The noise is this project's own, NOT mantaflow's."""

    def __init__(self, shape, noise, scale=1.0, sigma=0.5, time_step=None):
        if not isinstance(shape, CylinderShape) or not isinstance(noise, NoiseField):
            raise ValueError("NoiseInflow expects a CylinderShape and a NoiseField, got %r, %r" % (type(shape).__name__, type(noise).__name__))
        if not float(sigma) > 0:
            raise ValueError("NoiseInflow: sigma must be > 0, got %r" % (sigma,))
        self.shape, self.noise, self.scale, self.sigma = shape, noise, float(scale), float(sigma)
        self.time_step = None if time_step is None else float(time_step)

    def entry(self, b):
        return NoiseInflow(self.shape.entry(b), self.noise, self.scale, self.sigma, self.time_step)

    def time(self, t, dt):
        return t * (float(dt) if self.time_step is None else self.time_step)


def density_inflow(density, inflow, time=0.0, bnd=1, out=None):
    """``inflow`` (a ``NoiseInflow``) applied to ``density`` [B,(Z,)Y,X] at solver time ``time``: inside the cylinder, and up to ``sigma``
    outside it, interior cells become ``max(density, noise * scale * factor)``, factor falling from 1 at ``-sigma`` to 0 at ``sigma``
    (include/deepfluids_hip.h has the definition).  Returns ``out`` (new unless given; it may be ``density``)."""
    with torch.no_grad():
        d = _prep(density.detach(), "density")
        if d.dim() not in (3, 4) or not isinstance(inflow, NoiseInflow) or inflow.shape.dim != d.dim() - 1:
            raise ValueError("density_inflow expects a density [B,(Z,)Y,X] and a NoiseInflow of as many axes, got %s" % (tuple(d.shape),))
        if int(bnd) != bnd or bnd < 0:
            raise ValueError("density_inflow: bnd must be an integer >= 0, got %r" % (bnd,))
        if out is None:
            out = torch.empty_like(d)
        elif tuple(out.shape) != tuple(d.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("density_inflow: out must be a contiguous float32 GPU tensor of the density's shape")
        nd = d.dim() - 1
        q = inflow.noise.params(nd, d.shape[-1])
        call("df_density_noise_inflow%dd" % nd, _ptr(d), _ptr(out), _ptr(inflow.shape.on(d)), ctypes.addressof(q), float(time), inflow.scale,
             inflow.sigma, *(list(d.shape) + [int(bnd), _stream()]))
        return out


def _stamp(d, source, value, out, time=0.0, bnd=1):
    """``source`` (a mask, a SphereSource or a NoiseInflow) stamped into ``d`` -> ``out`` (which may be ``d``)"""
    if isinstance(source, NoiseInflow):
        density_inflow(d, source, time, bnd, out)
    elif isinstance(source, SphereSource):
        call("df_density_sphere_source%dd" % (d.dim() - 1), _ptr(d), _ptr(source.on(d)), source.radius, float(value), _ptr(out),
             *(list(d.shape) + [_stream()]))
    else:
        call("df_density_source", _ptr(d), _ptr(_source_mask(source, d)), float(value), _ptr(out), d.numel(), _stream())


def _source_arg(source, like):
    """what the sequence forms hold: a mask on the device, packed once, the SphereSource with its centres on the device, or the
    NoiseInflow (its cylinders move to the device at the first stamp, once)"""
    if source is None:
        return None
    if isinstance(source, NoiseInflow):
        return source
    if isinstance(source, SphereSource):
        return SphereSource(source.centers.to(like.device), source.radius)
    return _source_mask(source, like)


def _source_frame(source, t):
    return source.frame(t) if isinstance(source, SphereSource) else source


def _source_time(source, t, dt):
    return source.time(t, dt) if isinstance(source, NoiseInflow) else 0.0


def open_sides(spec, dim):
    """The ``open_sides`` bits of include/deepfluids_hip.h (bit 0..5: x-, x+, y-, y+, z-, z+) from what the reference's scene scripts
    pass to ``setOpenBound``: a string of ``xXyYzZ`` (lower case: the low side, upper case: the high side), ``True`` (every side of the
    grid's ``dim`` axes), ``False`` / ``None`` / ``''`` (closed), or the bits themselves."""
    if dim not in (2, 3):
        raise ValueError("open_sides: dim must be 2 or 3, got %r" % (dim,))
    if spec is None or spec is False or (isinstance(spec, str) and spec == ""):
        return 0
    if spec is True:
        return (1 << (2 * dim)) - 1
    if isinstance(spec, str):
        bits = 0
        for ch in spec:
            at = "xXyYzZ".find(ch)
            if at < 0:
                raise ValueError("open_sides: %r is not one of xXyYzZ (in %r)" % (ch, spec))
            bits |= 1 << at
    elif isinstance(spec, (int, np.integer)):
        bits = int(spec)
        if not 0 <= bits <= 63:
            raise ValueError("open_sides: bits must be in 0..63, got %r" % (spec,))
    else:
        raise ValueError("open_sides: expected a string of xXyYzZ, a bool, None or the bits, got %r" % (spec,))
    if dim == 2 and bits >= 16:
        raise ValueError("open_sides: %r opens a z side of a 2-D grid" % (spec,))
    return bits


def _fill_open(v, nd, bnd, osd):
    call("df_open_extrapolate%dd" % nd, _ptr(v), *(list(v.shape[:-1]) + [int(bnd), osd, _stream()]))


# Obstacles: a uint8 / bool mask [B,(Z,)Y,X] (nonzero = solid; [(Z,)Y,X] is shared by the batch) is packed once into the flags of
# include/deepfluids_hip.h (one byte per cell: the cell is fluid, each of its six neighbours is fluid), which every `_flags` kernel reads.
class ObstacleFlags(torch.Tensor):
    """What ``obstacle_flags`` returns: a uint8 tensor whose TYPE says that it holds flags, not a mask, and that carries the boundary
    width it was packed for.  Slices along the batch, clones and copies to another device stay ``ObstacleFlags`` and keep ``bnd``, so
    ``flags[e:e + 1]`` is still taken for flags.  Anything COMPUTED from flags (``flags & 1``, ``flags != 0``) is an ordinary tensor again,
    as is what ``as_subclass(torch.Tensor)`` or a trip through NumPy returns: a plain array is taken for a mask."""
    bnd = None
    _KEEP = frozenset(["__getitem__", "clone", "contiguous", "detach", "to", "cuda", "cpu", "expand", "unsqueeze", "squeeze", "pin_memory"])

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        out = super().__torch_function__(func, types, args, kwargs or {})
        if isinstance(out, ObstacleFlags):
            src = args[0] if args and isinstance(args[0], ObstacleFlags) else None
            if src is not None and getattr(func, "__name__", None) in cls._KEEP and out.dtype == torch.uint8:
                out.bnd = src.bnd                       # the same bytes, seen or copied: still flags
            else:
                out = out.as_subclass(torch.Tensor)     # computed from flags: an ordinary tensor
        return out


def obstacle_flags(obstacle, bnd=1, dim=None):
    """The flags tensor (``ObstacleFlags``, uint8 [B,(Z,)Y,X]) of an obstacle mask for boundary width ``bnd``: bit 0 = the cell is fluid
    (interior and not solid), bits 1-6 = its x-, x+, y-, y+, z-, z+ neighbour is.  ``obstacle``: bool / uint8 [B,(Z,)Y,X] or [(Z,)Y,X]
    (then B = 1, and every op broadcasts it over its batch).  A 3-dimensional mask is [B,Y,X] unless ``dim=3`` says it is [Z,Y,X].
    Build it once per sequence and hand it to the ``obstacle=`` keyword of the ops below; the tensor remembers ``bnd``."""
    with torch.no_grad():
        if int(bnd) != bnd or bnd < 1:
            raise ValueError("obstacle_flags: bnd must be an integer >= 1, got %r" % (bnd,))
        if isinstance(obstacle, ObstacleFlags):
            raise ValueError("obstacle_flags expects a mask of solid cells, got flags that are packed already")
        m = obstacle if isinstance(obstacle, torch.Tensor) else torch.as_tensor(np.asarray(obstacle))
        if not m.is_cuda:
            m = m.cuda()
        if m.dtype != torch.uint8:
            m = (m != 0).to(torch.uint8)
        if dim is None:
            dim = 3 if m.dim() == 4 else 2
        if dim not in (2, 3) or m.dim() not in (dim, dim + 1):
            raise ValueError("obstacle_flags expects a mask [B,(Z,)Y,X] or [(Z,)Y,X], got %s (dim=%r)" % (tuple(m.shape), dim))
        if m.dim() == dim:
            m = m[None]
        m = m.contiguous()
        flags = torch.empty_like(m).as_subclass(ObstacleFlags)
        flags.bnd = int(bnd)
        call("df_obstacle_flags%dd" % dim, _ptr(m), _ptr(flags), *(list(m.shape) + [int(bnd), _stream()]))
        return flags


def _obstacle_arg(obstacle, shape, bnd, who):
    """flags [B,(Z,)Y,X] for a field of ``shape`` from the ``obstacle=`` keyword: a flags tensor of ``obstacle_flags`` or a mask"""
    shape = tuple(shape)
    nd = len(shape) - 1
    if isinstance(obstacle, ObstacleFlags):
        if obstacle.dtype != torch.uint8 or obstacle.bnd is None:
            raise ValueError("%s: obstacle was derived from flags by an operation that does not keep them flags (dtype %s); pass the "
                             "flags of obstacle_flags, or a mask" % (who, obstacle.dtype))
        if obstacle.bnd != int(bnd):
            raise ValueError("%s: the obstacle flags were built for bnd=%d, the step uses bnd=%d" % (who, obstacle.bnd, int(bnd)))
    else:
        m = obstacle if isinstance(obstacle, torch.Tensor) else torch.as_tensor(np.asarray(obstacle))
        if tuple(m.shape) not in (shape, shape[1:], (1,) + shape[1:]):
            raise ValueError("%s: obstacle must be a mask %s or %s, got %s" % (who, shape, shape[1:], tuple(m.shape)))
        obstacle = obstacle_flags(m, bnd, dim=nd)
    if tuple(obstacle.shape) == shape:
        return obstacle if obstacle.is_contiguous() else obstacle.contiguous()
    if tuple(obstacle.shape) != (1,) + shape[1:]:
        raise ValueError("%s: obstacle flags %s do not fit a field %s" % (who, tuple(obstacle.shape), shape))
    return obstacle.expand(shape).contiguous()


def advect_workspace(density, order=2, source=False):
    """The scratch ``advect`` needs for one step on ``density``: one grid for the source-stamped density, one for the forward pass of
    order 2.  Reusable across calls of the same shape."""
    n = density.numel() * ((1 if source else 0) + (1 if order == 2 else 0))
    return torch.empty((max(n, 1),), dtype=torch.float32, device=density.device)


def _advect_step(d, v, nd, out, fwd, dt, order, clamp_mode, bnd, vel_scale, flags=None):
    sfx = "%dd" % nd
    dims = list(d.shape)
    if order == 1:                                      # the first-order value ignores obstacles
        call("df_advect_sl" + sfx, _ptr(d), _ptr(v), _ptr(out), *(dims + [dt, vel_scale, bnd, _stream()]))
    else:
        call("df_advect_sl" + sfx, _ptr(d), _ptr(v), _ptr(fwd), *(dims + [dt, vel_scale, bnd, _stream()]))
        if flags is None:
            call("df_advect_mc" + sfx, _ptr(d), _ptr(fwd), _ptr(v), _ptr(out), *(dims + [dt, vel_scale, bnd, clamp_mode, _stream()]))
        else:
            call("df_advect_mc" + sfx + "_flags", _ptr(d), _ptr(fwd), _ptr(v), _ptr(out), _ptr(flags),
                 *(dims + [dt, vel_scale, bnd, clamp_mode, _stream()]))


def _advect_args(order, clamp_mode, bnd):
    if order not in (1, 2):
        raise ValueError("advect: order must be 1 (semi-Lagrangian) or 2 (MacCormack), got %r" % (order,))
    if clamp_mode not in (1, 2):
        raise ValueError("advect: clamp_mode must be 1 or 2, got %r" % (clamp_mode,))
    if int(bnd) != bnd or bnd < 1:
        raise ValueError("advect: bnd must be an integer >= 1, got %r" % (bnd,))


def advect(density, vel, dt, order=2, clamp_mode=2, bnd=1, vel_scale=1.0, source=None, source_value=1.0, out=None, workspace=None,
           obstacle=None, time=0.0):
    """One advection step of ``density`` [B,(Z,)Y,X] through ``vel`` [B,(Z,)Y,X,C] (MAC face values, C = 2 | 3), modelled on mantaflow's
    ``advectSemiLagrange(order, boundaryWidth=bnd, clampMode=clamp_mode)`` as the reference's scene scripts call it
    (scene/smoke_pos_size.py:99-101) -- NOT bit-identical to mantaflow, which cannot be run here; include/deepfluids_hip.h holds the
    definition that is tested.  ``vel_scale`` multiplies the velocities inside the kernel (``x_range`` for a generator's normalised
    output); ``source`` is an optional mask [B,(Z,)Y,X] (or one broadcastable to it) of cells set to ``source_value`` before the step,
    or a ``SphereSource`` (one sphere per batch entry, centres on the device), or a ``NoiseInflow`` (evaluated at solver time ``time``).
    Returns a new density (``out`` if given; it must not be ``density``).  ``workspace``: see ``advect_workspace``.  ``obstacle``: a
    mask of solid cells or the flags of ``obstacle_flags``; the MacCormack correction and its clamp then run over fluid cells only (the
    first-order value and the source stamp ignore obstacles, as mantaflow's do)."""
    with torch.no_grad():
        _advect_args(order, clamp_mode, bnd)
        d, v, nd = _advect_dims(density, vel)
        flags = _obstacle_arg(obstacle, d.shape, bnd, "advect") if obstacle is not None else None
        n = d.numel()
        need = n * ((1 if source is not None else 0) + (1 if order == 2 else 0))
        ws = workspace if workspace is not None else advect_workspace(d, order, source is not None)
        if ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < need:
            raise ValueError("advect: workspace must be a contiguous float32 GPU tensor of >= %d elements" % need)
        ws = ws.view(-1)
        if out is None:
            out = _empty(d.shape, d)
        elif out.data_ptr() == d.data_ptr() or tuple(out.shape) != tuple(d.shape) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("advect: out must be a contiguous float32 tensor of the density's shape, and not the density itself")
        off = 0
        if source is not None:
            stamped = ws[:n].view(d.shape)
            _stamp(d, source, source_value, stamped, time, bnd)
            d, off = stamped, n
        fwd = ws[off:off + n] if order == 2 else None
        _advect_step(d, v, nd, out, fwd, float(dt), order, clamp_mode, int(bnd), float(vel_scale), flags)
        return out


def density_image(d, out=None):
    """The ``d_adv`` frame of density [B,(Z,)Y,X] (scene/smoke_pos_size.py:105-106): uint8 [B,Y,X], rows flipped in y, of
    ``clip(255 * d, 0, 255)`` (3-D: of the z mean).  The reference casts without clipping, so values outside [0,1] wrap there."""
    with torch.no_grad():
        d = _prep(d.detach(), "density")
        if d.dim() not in (3, 4):
            raise ValueError("density_image expects [B,(Z,)Y,X], got %s" % (tuple(d.shape),))
        shape = (d.shape[0], d.shape[-2], d.shape[-1])
        if out is None:
            out = _u8(shape, d)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("density_image: out must be a contiguous uint8 tensor %s" % (shape,))
        call("df_density_image%dd" % (d.dim() - 1), _ptr(d), _ptr(out), *(list(d.shape) + [_stream()]))
        return out


def advect_sequence(density0, vels, dt, order=2, clamp_mode=2, bnd=1, vel_scale=1.0, source=None, source_value=1.0, images=False,
                    obstacle=None):
    """``T`` chained ``advect`` steps over ``vels`` [T,B,(Z,)Y,X,C] (a tensor or a sequence of T tensors), the source stamped before
    every step, ping-ponging two density buffers (``density0`` is left untouched).  Returns the final density, and with ``images`` also
    the uint8 frames [T,B,Y,X] of ``density_image`` after each step, produced on the device and copied to the host once (a NumPy
    array).  ``obstacle``: as for ``advect``; its flags are built once for the sequence.  A ``NoiseInflow`` source is evaluated at
    ``t * dt`` (its own ``time_step`` if it has one) before step t."""
    with torch.no_grad():
        _advect_args(order, clamp_mode, bnd)
        T = len(vels)
        if T < 1:
            raise ValueError("advect_sequence: no velocity frames")
        cur, _, nd = _advect_dims(density0, vels[0])
        cur = cur.clone()
        nxt = torch.empty_like(cur)
        fwd = torch.empty_like(cur) if order == 2 else None
        mask = _source_arg(source, cur)                    # a SphereSource [T,B,D] stamps centers[t] before step t
        flags = _obstacle_arg(obstacle, cur.shape, bnd, "advect_sequence") if obstacle is not None else None
        imgs = _u8((T, cur.shape[0], cur.shape[-2], cur.shape[-1]), cur) if images else None
        for t in range(T):
            _, v, _ = _advect_dims(cur, vels[t])
            if mask is not None:
                _stamp(cur, _source_frame(mask, t), source_value, cur, _source_time(mask, t, dt), bnd)
            _advect_step(cur, v, nd, nxt, fwd, float(dt), order, clamp_mode, int(bnd), float(vel_scale), flags)
            cur, nxt = nxt, cur
            if images:
                density_image(cur, out=imgs[t])
        if images:
            return cur, imgs.cpu().numpy()
        return cur


def sphere_mask(shape, center, radius, device=None):
    """mantaflow's ``Sphere.applyToGrid`` as a mask: uint8 [(Z,)Y,X], 1 where the cell centre (i+.5, j+.5[, k+.5]) lies within ``radius``
    of ``center`` (cell units, xyz order).  Built on the host (it is made once per sweep); ``device=None`` keeps it there."""
    shape = tuple(int(n) for n in shape)
    if len(shape) not in (2, 3) or len(center) != len(shape):
        raise ValueError("sphere_mask expects a 2-D or 3-D shape and a centre of as many coordinates, got %s, %s" % (shape, tuple(center)))
    r2 = np.zeros(shape, np.float64)
    for a, c in enumerate(center):                      # a = 0 is x: the last array axis
        ax = len(shape) - 1 - a
        sh = [1] * len(shape)
        sh[ax] = shape[ax]
        r2 = r2 + ((np.arange(shape[ax]) + 0.5 - float(c)) ** 2).reshape(sh)
    m = torch.from_numpy((r2 <= float(radius) * float(radius)).astype(np.uint8))
    return m if device is None else m.to(device)


def cylinder_mask(shape, center, z, radius, device=None):
    """The host-side twin of ``sphere_mask`` for mantaflow's ``Cylinder``: uint8 [(Z,)Y,X], 1 where the cell centre (i+.5, j+.5[, k+.5])
    lies inside the cylinder around ``center`` with HALF-axis vector ``z`` and ``radius`` (cell units, xyz order): with a = z/|z| and
    d = centre - center, ``|d.a| <= |z|`` and ``|d|^2 - (d.a)^2 < radius^2`` (the test of ``stamp_velocity``, at cell centres)."""
    shape = tuple(int(n) for n in shape)
    if len(shape) not in (2, 3) or len(center) != len(shape) or len(z) != len(shape):
        raise ValueError("cylinder_mask expects a 2-D or 3-D shape, a centre and an axis of as many coordinates, got %s, %s, %s" %
                         (shape, tuple(center), tuple(z)))
    zl = math.sqrt(sum(float(v) ** 2 for v in z))
    if not zl > 0:
        raise ValueError("cylinder_mask: a half-axis z of length zero")
    h = np.zeros(shape, np.float64)
    d2 = np.zeros(shape, np.float64)
    for a in range(len(shape)):
        d = _centres(shape, a) - float(center[a])
        h = h + d * (float(z[a]) / zl)
        d2 = d2 + d * d
    m = torch.from_numpy(((np.abs(h) <= zl) & (np.maximum(d2 - h * h, 0.0) < float(radius) * float(radius))).astype(np.uint8))
    return m if device is None else m.to(device)


def stamp_velocity(vel, shape, values, out=None):
    """mantaflow's ``Cylinder.applyToGrid(grid=vel, value=...)`` on the MAC velocity ``vel`` [B,(Z,)Y,X,D]: component a of a cell becomes
    ``values[b][a]`` where the position of that FACE lies inside entry b's cylinder (``shape``, a ``CylinderShape``); faces are tested
    one by one, obstacles and the band are ignored.  ``values``: [B,D] or [D].  Returns ``out`` (new unless given; it may be ``vel``)."""
    with torch.no_grad():
        v, nd = _smoke_vel(vel, "stamp_velocity")
        if not isinstance(shape, CylinderShape) or shape.dim != nd:
            raise ValueError("stamp_velocity expects a CylinderShape of %d axes" % nd)
        vals = _entry_rows(values, v, nd, "stamp_velocity: values")
        out = _smoke_out(out, v, "stamp_velocity")
        call("df_mac_cylinder_stamp%dd" % nd, _ptr(v), _ptr(shape.on(v)), _ptr(vals), _ptr(out), *(list(v.shape[:-1]) + [_stream()]))
        return out


def _entry_rows(x, v, nd, what):
    """[B,D] float32 on ``v``'s device from [B,D] or [D] (a tensor, or anything NumPy converts)"""
    t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
    if t.dim() not in (1, 2) or t.shape[-1] != nd or (t.dim() == 2 and t.shape[0] not in (1, v.shape[0])):
        raise ValueError("%s must be [%d,%d] or [%d], got %s" % (what, v.shape[0], nd, nd, tuple(t.shape)))
    return t.to(device=v.device, dtype=torch.float32).reshape(-1, nd).expand(v.shape[0], nd).contiguous()


# ---- the smoke solver step (the main() loop of the reference's scene/smoke_pos_size.py:186-195, a closed box): MAC self-advection, walls
#      and buoyancy, a conjugate-gradient pressure projection.  Inference only, no autograd.  The step is defined in
#      include/deepfluids_hip.h; parity is with the fp64 restatement of tests/smoke_ref.py, NOT with mantaflow, which cannot be run here.
#      Obstacles (the reference's scene/smoke3_obs_buo.py) enter through the ``obstacle=`` keyword: "interior" then reads "fluid".
#      Open sides (scene/smoke3_rot.py, smoke3_mov.py, smoke3_vel_buo.py, the open_bound option of smoke_pos_size.py) enter through
#      ``open_bound=`` (``open_sides`` parses it) and combine with obstacles; a moving source is a ``SphereSource``.  Parity is with
#      tests/smoke_open_ref.py, NOT with mantaflow.
#      The inflow of scene/smoke3_vel_buo.py enters through a ``NoiseInflow`` source (a seeded lattice noise of this project's own, NOT
#      mantaflow's wavelet noise), ``inflow_velocity=`` (the cylinder stamp) and a ``force`` tensor [B,D] (one buoyancy per batch entry);
#      parity is with tests/smoke_inflow_ref.py, NOT with mantaflow.
#      Left out: mantaflow's convective outflow extrapolation (a zero-gradient fill stands in for it), the MIC(0) preconditioner ----
DEFAULT_CHECK_EVERY = 16      # iterations between two looks at the active count; the sweep over 1, 4, 16, 64 is in profiles/smoke.md


def _smoke_vel(vel, who):
    v = _prep(vel.detach(), "vel")
    if v.dim() not in (4, 5) or v.shape[-1] != v.dim() - 2:
        raise ValueError("%s expects a velocity [B,(Z,)Y,X,D] with D = 2 | 3 matching the grid, got %s" % (who, tuple(v.shape)))
    return v, v.dim() - 2


def _smoke_out(out, like, who):
    if out is None:
        return torch.empty_like(like)
    if tuple(out.shape) != tuple(like.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous float32 GPU tensor of shape %s" % (who, tuple(like.shape)))
    return out


def advect_velocity(vel, dt, order=2, clamp_mode=2, bnd=1, out=None, workspace=None, obstacle=None, open_bound=None):
    """The MAC velocity ``vel`` [B,(Z,)Y,X,D] carried through itself for ``dt`` (cells per unit time), modelled on mantaflow's
    ``advectSemiLagrange(vel, vel, order, boundaryWidth=bnd, clampMode=clamp_mode)``; include/deepfluids_hip.h holds the definition
    that is tested.  Returns a new velocity (``out`` if given; not ``vel`` itself).  ``workspace``: a float32 GPU tensor of
    ``vel.numel()`` elements for order 2.  ``obstacle``: a mask or the flags of ``obstacle_flags``; component a is then corrected and
    clamped only where c and c - e_a are fluid, over fluid corners (the first-order value ignores obstacles).  ``open_bound``: the open
    sides (see ``open_sides``); the high-side boundary faces are then advected too, faces between a fluid and an open cell are corrected,
    and the open cells are filled (zero gradient) before returning, so the result is complete."""
    with torch.no_grad():
        _advect_args(order, clamp_mode, bnd)
        v, nd = _smoke_vel(vel, "advect_velocity")
        osd = open_sides(open_bound, nd)
        flags = _obstacle_arg(obstacle, v.shape[:-1], bnd, "advect_velocity") if obstacle is not None else None
        out = _smoke_out(out, v, "advect_velocity")
        if out.data_ptr() == v.data_ptr():
            raise ValueError("advect_velocity: out must not be the velocity itself (the step gathers)")
        dims = list(v.shape[:-1])
        sfx = "%dd" % nd
        osa = [osd] if osd else []                          # the `_open` twins: open_sides right after bnd, flags nullable
        slx = sfx + ("_open" if osd else "")
        if order == 1:
            call("df_mac_advect_sl" + slx, _ptr(v), _ptr(out), *(dims + [float(dt), int(bnd)] + osa + [_stream()]))
            if osd:
                _fill_open(out, nd, bnd, osd)
            return out
        ws = workspace if workspace is not None else torch.empty((v.numel(),), dtype=torch.float32, device=v.device)
        if ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < v.numel():
            raise ValueError("advect_velocity: workspace must be a contiguous float32 GPU tensor of >= %d elements" % v.numel())
        call("df_mac_advect_sl" + slx, _ptr(v), _ptr(ws), *(dims + [float(dt), int(bnd)] + osa + [_stream()]))
        if osd:
            call("df_mac_advect_mc" + sfx + "_open", _ptr(v), _ptr(ws), _ptr(out), None if flags is None else _ptr(flags),
                 *(dims + [float(dt), int(bnd), osd, int(clamp_mode), _stream()]))
            _fill_open(out, nd, bnd, osd)
        elif flags is None:
            call("df_mac_advect_mc" + sfx, _ptr(v), _ptr(ws), _ptr(out), *(dims + [float(dt), int(bnd), int(clamp_mode), _stream()]))
        else:
            call("df_mac_advect_mc" + sfx + "_flags", _ptr(v), _ptr(ws), _ptr(out), _ptr(flags),
                 *(dims + [float(dt), int(bnd), int(clamp_mode), _stream()]))
        return out


def wall_buoyancy(vel, density, force, bnd=1, out=None, obstacle=None, open_bound=None):
    """``setWallBcs`` of a closed box and ``addBuoyancy`` in one element-wise pass: component a of cell c is 0 unless c and c - e_a are
    both interior; kept components get ``+ (0.5 * force[a]) * (density[c] + density[c-e_a])``.  ``force``: D numbers (x, y[, z]), or a
    tensor [B,D]: one force per batch entry, read on the device (equal rows give the bits of the D numbers).
    ``out`` may be ``vel`` (in place).  ``obstacle``: a mask or the flags of ``obstacle_flags``; "interior" then reads "fluid", so the
    faces of solid cells are 0 as well.  ``open_bound``: the open sides (see ``open_sides``); a face between a fluid and an open cell is
    then kept, without the buoyancy term, and open cells keep all their components."""
    with torch.no_grad():
        v, nd = _smoke_vel(vel, "wall_buoyancy")
        osd = open_sides(open_bound, nd)
        d = _prep(density.detach(), "density")
        if tuple(d.shape) != tuple(v.shape[:-1]):
            raise ValueError("wall_buoyancy expects a density %s for a velocity %s, got %s" % (tuple(v.shape[:-1]), tuple(v.shape), tuple(d.shape)))
        if int(bnd) != bnd or bnd < 1:
            raise ValueError("wall_buoyancy: bnd must be an integer >= 1, got %r" % (bnd,))
        if isinstance(force, torch.Tensor):
            if force.dim() != 2:
                raise ValueError("wall_buoyancy: a force tensor must be [B,D], got %s" % (tuple(force.shape),))
            rows = _entry_rows(force, v, nd, "wall_buoyancy: force")
            out = _smoke_out(out, v, "wall_buoyancy")
            flags = None if obstacle is None else _obstacle_arg(obstacle, d.shape, bnd, "wall_buoyancy")
            call("df_wall_buoyancy%dd_open_dev" % nd, _ptr(v), _ptr(d), _ptr(out), None if flags is None else _ptr(flags), _ptr(rows),
                 *(list(d.shape) + [int(bnd), osd, _stream()]))
            return out
        f = [float(x) for x in force]
        if len(f) != nd:
            raise ValueError("wall_buoyancy: force must have %d components, got %r" % (nd, force))
        out = _smoke_out(out, v, "wall_buoyancy")
        if osd:
            flags = None if obstacle is None else _obstacle_arg(obstacle, d.shape, bnd, "wall_buoyancy")
            call("df_wall_buoyancy%dd_open" % nd, _ptr(v), _ptr(d), _ptr(out), None if flags is None else _ptr(flags),
                 *(list(d.shape) + f + [int(bnd), osd, _stream()]))
        elif obstacle is None:
            call("df_wall_buoyancy%dd" % nd, _ptr(v), _ptr(d), _ptr(out), *(list(d.shape) + f + [int(bnd), _stream()]))
        else:
            flags = _obstacle_arg(obstacle, d.shape, bnd, "wall_buoyancy")
            call("df_wall_buoyancy%dd_flags" % nd, _ptr(v), _ptr(d), _ptr(out), _ptr(flags), *(list(d.shape) + f + [int(bnd), _stream()]))
        return out


def _read_word(t):
    """the one word the host reads during a solve: the number of batch entries still iterating (a device-to-host copy that waits for
    the stream); tools/smoke_probe.py times it"""
    return int(t.item())


def _pressure_dims(v, nd):
    dims = list(v.shape[:-1])
    return dims, (dims if nd == 3 else [dims[0], 1] + dims[1:])


def pressure_workspace(vel, ghost_fluid=False):
    """The scratch ``solve_pressure`` needs for ``vel`` [B,(Z,)Y,X,D] (residual, two directions, A p, partial sums, per-entry scalars): a
    float32 GPU tensor, reusable across calls of the same shape.  ``ghost_fluid=True`` adds the two arrays (diagonal, preconditioned
    residual) that ``solve_pressure_liquid(phi=...)`` needs; such a workspace serves the plain solves too."""
    v, nd = _smoke_vel(vel, "pressure_workspace")
    nbytes = query("df_pressure_workspace_bytes_gf" if ghost_fluid else "df_pressure_workspace_bytes", *[int(x) for x in _pressure_dims(v, nd)[1]])
    if nbytes < 0:
        raise ValueError("pressure_workspace: unsupported extents %s" % (tuple(v.shape),))
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=v.device)


def default_max_iter(shape):
    """mantaflow's ``cgMaxIterFac=10``: ``int(10 * max(extent))``, times 4 in 2-D."""
    return int(10 * max(shape)) * (1 if len(shape) == 3 else 4)


# ---- multigrid preconditioner of the smoke pressure solve: the V-cycle defined in include/deepfluids_hip.h ----
DEFAULT_MG_ALPHA = 1.8        # the over-correction of the coarse-grid step; the table it was chosen from is in profiles/smoke_mg.md
DEFAULT_MG_CHECK_EVERY = 4    # a preconditioned solve takes 6-12 iterations: a look every 16 would launch up to 10 idle cycles after the last


class Multigrid(object):
    """The settings of ``preconditioner=`` on every solve of the library: ``alpha`` in [1, 2), the over-correction of the coarse-grid
    step, and ``diffusion``: whether ``liquid_step`` / ``simulate_liquid`` with ``viscosity_alpha=`` precondition the diffusion solve as
    well as the projection (a diffusion of small ``viscosity_alpha`` takes few plain iterations, and a cycle costs more than it saves:
    profiles/liquid_mg.md).  On the smoke calls it means ``"mg"`` with that ``alpha``."""

    def __init__(self, alpha=DEFAULT_MG_ALPHA, diffusion=True):
        if not isinstance(diffusion, (bool, np.bool_)):
            raise ValueError("Multigrid: diffusion must be True or False, got %r" % (diffusion,))
        self.alpha, self.diffusion = _mg_alpha_arg(alpha, "Multigrid"), bool(diffusion)


MG_SYSTEMS = ("smoke", "liquid", "gf", "diffusion")


class MultigridHierarchy(object):
    """What ``multigrid_hierarchy`` (and ``multigrid_hierarchy_liquid`` / ``_diffusion``) returns: one float32 GPU block that holds, per
    batch entry and level, the face weights, ``dir``, ``diag``, the level's right-hand side and x scratch, and ``z`` -- and the geometry it
    was built for (``shape`` [(Z,)Y,X], ``batch``, ``bnd``, ``open_sides`` bits) and the ``system`` whose matrix level 0 is: ``"smoke"``,
    ``"liquid"`` (free surface), ``"gf"`` (ghost fluid) or ``"diffusion"`` (``batch`` then counts the B*D (entry, component) systems).
    Reusable across solves of the same geometry; a solve writes its scratch, so one hierarchy serves one stream at a time."""

    def __init__(self, block, shape, batch, bnd, osd, alpha, system="smoke"):
        self.block, self.shape, self.batch, self.bnd, self.open_sides, self.alpha = block, tuple(shape), int(batch), int(bnd), int(osd), float(alpha)
        self.system = system
        self.dim = len(self.shape)
        self.dims4 = [self.batch] + ([1] if self.dim == 2 else []) + list(self.shape)
        self.nbytes = block.numel() * 4
        self.levels = query("df_mg_levels", self.dim, *self.dims4[1:])

    @property
    def device(self):
        return self.block.device

    def level_shape(self, level):
        s = self.shape
        for _ in range(level):
            s = tuple((n + 1) // 2 for n in s)
        return s

    def _array(self, level, array):
        off = query("df_mg_level_offset", self.dim, *(self.dims4 + [int(level), int(array)]))
        if off < 0:
            raise ValueError("MultigridHierarchy: no array %d on level %d of %d" % (array, level, self.levels))
        shape = (self.batch,) + self.level_shape(level)
        return self.block[off:off + int(np.prod(shape))].view(shape)

    def weights(self, level):
        """``(w, dir, diag)`` of a level: ``w`` a tuple of D tensors [B,(Z,)Y,X of the level] (axis x, y[, z]); views of the block"""
        return tuple(self._array(level, a) for a in range(self.dim)), self._array(level, self.dim), self._array(level, self.dim + 1)

    @property
    def z(self):
        return self._array(0, self.dim + 2)


def multigrid_hierarchy(vel_or_shape, bnd=1, obstacle=None, open_bound=None, batch=None, alpha=DEFAULT_MG_ALPHA, device=None):
    """The multigrid hierarchy of the smoke pressure matrix (include/deepfluids_hip.h, "multigrid preconditioner") for a velocity
    [B,(Z,)Y,X,D] or a grid shape [(Z,)Y,X] with ``batch`` entries (default: those of a per-entry ``obstacle``, else 1): level 0 is the matrix ``solve_pressure`` uses for ``bnd``,
    ``obstacle`` (a mask or flags, per entry or shared) and ``open_bound``; the coarser levels are its Galerkin products over aggregates of
    2^D cells.  Build it once per geometry and pass it as ``preconditioner=``; the solve it is passed to must use the same ``obstacle``,
    which cannot be checked there.  ``alpha`` in [1, 2) scales the coarse-grid correction."""
    with torch.no_grad():
        if isinstance(vel_or_shape, torch.Tensor):
            v, nd = _smoke_vel(vel_or_shape, "multigrid_hierarchy")
            shape, B, device = tuple(v.shape[1:-1]), v.shape[0], v.device
            if batch is not None and int(batch) != B:
                raise ValueError("multigrid_hierarchy: batch=%r beside a velocity of %d entries" % (batch, B))
        else:
            shape = tuple(int(n) for n in vel_or_shape)
            nd = len(shape)
            if batch is None:                                  # a per-entry obstacle says how many entries there are
                batch = obstacle.shape[0] if isinstance(obstacle, torch.Tensor) and obstacle.dim() == nd + 1 else 1
            B = int(batch)
            if nd not in (2, 3) or B < 1:
                raise ValueError("multigrid_hierarchy expects a velocity or a grid shape [(Z,)Y,X] and batch >= 1, got %r, batch=%r" % (vel_or_shape, batch))
            if device is None:
                device = obstacle.device if isinstance(obstacle, torch.Tensor) and obstacle.is_cuda else torch.device("cuda", torch.cuda.current_device())
        if int(bnd) != bnd or bnd < 1:
            raise ValueError("multigrid_hierarchy: bnd must be an integer >= 1, got %r" % (bnd,))
        if not 1.0 <= alpha < 2.0:
            raise ValueError("multigrid_hierarchy: alpha must lie in [1, 2), got %r" % (alpha,))
        osd = open_sides(open_bound, nd)
        dims = [B] + list(shape)
        flags = None if obstacle is None else _obstacle_arg(obstacle, dims, int(bnd), "multigrid_hierarchy")
        if flags is not None and flags.device != torch.device(device):
            raise ValueError("multigrid_hierarchy: the obstacle is on %s, the hierarchy on %s" % (flags.device, device))
        dims4 = [B] + ([1] if nd == 2 else []) + list(shape)
        nbytes = query("df_mg_hierarchy_bytes", nd, *dims4)
        if nbytes < 0:
            raise ValueError("multigrid_hierarchy: unsupported extents %s" % (tuple(dims),))
        h = MultigridHierarchy(torch.empty((nbytes // 4,), dtype=torch.float32, device=device), shape, B, bnd, osd, alpha)
        call("df_mg_build", _ptr(h.block), h.nbytes, _ptr(flags), nd, *(dims4 + [int(bnd), osd, _stream()]))
        return h


def multigrid_apply(hierarchy, r):
    """``z = M r``: one V-cycle of ``hierarchy`` on ``r`` [B,(Z,)Y,X] (float32, on the hierarchy's device).  Returns ``hierarchy.z``, a
    view of the hierarchy's block that the next cycle overwrites.  The bare op; ``solve_pressure(preconditioner=...)`` is its user."""
    with torch.no_grad():
        if not isinstance(hierarchy, MultigridHierarchy):
            raise ValueError("multigrid_apply expects the hierarchy of multigrid_hierarchy, got %r" % (type(hierarchy),))
        want = (hierarchy.batch,) + hierarchy.shape
        if (not isinstance(r, torch.Tensor) or r.dtype != torch.float32 or tuple(r.shape) != want or r.device != hierarchy.device
                or not r.is_contiguous()):
            raise ValueError("multigrid_apply: r must be a contiguous float32 tensor %s on %s" % (want, hierarchy.device))
        call("df_mg_apply", _ptr(hierarchy.block), hierarchy.nbytes, _ptr(r.detach()), hierarchy.dim, *(hierarchy.dims4 + [hierarchy.alpha, _stream()]))
        return hierarchy.z


def _mg_alpha_arg(alpha, who):
    """a real number (Python's or NumPy's, not a bool) in [1, 2), as a float"""
    if isinstance(alpha, (bool, np.bool_)) or not isinstance(alpha, numbers.Real) or not 1.0 <= alpha < 2.0:
        raise ValueError("%s: alpha must be a number in [1, 2), got %r" % (who, alpha))
    return float(alpha)


def _hierarchy_block(who, nd, systems, shape, device, out, bnd, alpha, system):
    """a new hierarchy of ``systems`` entries for ``system``, or the caller's ``out`` -- which must be one of the same system, geometry,
    ``bnd`` and device, and takes the call's ``alpha``: nothing is allocated then"""
    dims4 = [systems] + ([1] if nd == 2 else []) + list(shape)
    if out is not None:
        if (not isinstance(out, MultigridHierarchy) or out.system != system or out.shape != tuple(shape) or out.batch != systems or out.bnd != bnd
                or out.device != torch.device(device)):
            raise ValueError("%s: out must be a %r hierarchy of shape %s, %d systems, bnd %d on %s" % (who, system, tuple(shape), systems, bnd, device))
        out.alpha = alpha
        return out
    nbytes = query("df_mg_hierarchy_bytes", nd, *dims4)
    if nbytes < 0:
        raise ValueError("%s: unsupported extents %s" % (who, tuple(dims4)))
    return MultigridHierarchy(torch.empty((nbytes // 4,), dtype=torch.float32, device=device), shape, systems, bnd, 0, alpha, system)


def multigrid_hierarchy_liquid(vel_or_shape, flags, bnd=1, phi=None, gf_clamp=1e-4, alpha=DEFAULT_MG_ALPHA, batch=None, out=None):
    """The multigrid hierarchy of the free-surface pressure matrix of ``solve_pressure_liquid`` (include/deepfluids_hip_liquid_mg.h) for
    ``flags`` [B,(Z,)Y,X] (``liquid_flags``) on the grid of a velocity [B,(Z,)Y,X,D] or a shape [(Z,)Y,X]: level 0 has weight 1 between two
    liquid cells and counts the air neighbours (p = 0 there) on the diagonal; with ``phi`` (and ``gf_clamp``) it is the ghost-fluid
    matrix, 1 / theta per air neighbour.  The hierarchy's ``system`` is ``"liquid"`` or ``"gf"``.  The liquid moves every step:
    ``out=`` rebuilds a hierarchy of the same geometry in place, with no allocation."""
    who = "multigrid_hierarchy_liquid"
    with torch.no_grad():
        if not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda or not flags.is_contiguous() or flags.dim() not in (3, 4):
            raise ValueError("%s: flags must be the uint8 GPU tensor [B,(Z,)Y,X] of liquid_flags" % who)
        if isinstance(vel_or_shape, torch.Tensor):
            v, nd = _smoke_vel(vel_or_shape, who)
            shape, B = tuple(v.shape[1:-1]), v.shape[0]
            if v.device != flags.device:
                raise ValueError("%s: the velocity is on %s, the flags on %s" % (who, v.device, flags.device))
        else:
            shape, B = tuple(int(n) for n in vel_or_shape), flags.shape[0]
            nd = len(shape)
        if batch is not None and int(batch) != B:
            raise ValueError("%s: batch=%r beside %d entries" % (who, batch, B))
        if nd not in (2, 3) or tuple(flags.shape) != (B,) + shape:
            raise ValueError("%s: flags %s for a grid %s of %d entries" % (who, tuple(flags.shape), shape, B))
        bnd, alpha = _liquid_bnd(bnd, who), _mg_alpha_arg(alpha, who)
        gfc = 0.0
        if phi is not None:
            gfc = _gf_clamp_arg(gf_clamp, who)
            if (not isinstance(phi, torch.Tensor) or phi.dtype != torch.float32 or tuple(phi.shape) != tuple(flags.shape) or phi.device != flags.device
                    or not phi.is_contiguous()):
                raise ValueError("%s: phi must be a contiguous float32 GPU tensor %s on the flags' device" % (who, tuple(flags.shape)))
            phi = phi.detach()
        h = _hierarchy_block(who, nd, B, shape, flags.device, out, bnd, alpha, "liquid" if phi is None else "gf")
        call("df_mg_build_liquid", _ptr(h.block), h.nbytes, _ptr(flags), _ptr(phi), nd, *(h.dims4 + [bnd, gfc, _stream()]))
        return h


def multigrid_hierarchy_diffusion(vel, alpha_v, bnd=1, alpha=DEFAULT_MG_ALPHA, out=None):
    """The multigrid hierarchy of ``(I - alpha_v * Laplacian)`` of ``diffuse_velocity`` (include/deepfluids_hip_liquid_mg.h) on the grid of
    ``vel`` [B,(Z,)Y,X,D]: one system per (entry, component) pair, so ``batch`` is B*D; ``alpha_v`` a number or B numbers as in
    ``diffuse_velocity`` (or the [B] float32 device tensor a caller already holds).  ``system`` is ``"diffusion"``.  ``alpha`` in [1, 2)
    scales the coarse-grid correction.  ``out=``: rebuild in place, no allocation beside the [B] numbers."""
    who = "multigrid_hierarchy_diffusion"
    with torch.no_grad():
        v, nd = _smoke_vel(vel, who)
        bnd, alpha = _liquid_bnd(bnd, who), _mg_alpha_arg(alpha, who)
        B = v.shape[0]
        if isinstance(alpha_v, torch.Tensor) and alpha_v.is_cuda:
            if alpha_v.dtype != torch.float32 or tuple(alpha_v.shape) != (B,) or alpha_v.device != v.device or not alpha_v.is_contiguous():
                raise ValueError("%s: a device alpha_v must be a contiguous float32 tensor [%d] on the velocity's device" % (who, B))
            al = alpha_v
        else:
            al = torch.from_numpy(_diffusion_alpha_arg(alpha_v, B, who)).to(v.device)
        h = _hierarchy_block(who, nd, B * nd, tuple(v.shape[1:-1]), v.device, out, bnd, alpha, "diffusion")
        call("df_mg_build_diffusion", _ptr(h.block), h.nbytes, _ptr(al), nd, B, *(h.dims4[1:] + [bnd, _stream()]))
        return h


def _preconditioner_arg(preconditioner, who):
    """``None``, ``"mg"``, a ``Multigrid`` or a ``MultigridHierarchy``; checked before anything touches a GPU"""
    if (preconditioner is None or isinstance(preconditioner, (MultigridHierarchy, Multigrid))
            or (isinstance(preconditioner, str) and preconditioner == "mg")):
        return preconditioner
    raise ValueError("%s: preconditioner must be None, 'mg', an ops.Multigrid or the hierarchy of multigrid_hierarchy, got %r" % (who, preconditioner))


def _liquid_preconditioner_arg(preconditioner, who):
    """the ``preconditioner=`` of the liquid calls: ``None``, an ``ops.Multigrid`` or a ``MultigridHierarchy``; the string ``"mg"`` belongs
    to the smoke calls and stays refused here.  Checked before anything else is looked at."""
    if preconditioner is None or isinstance(preconditioner, (MultigridHierarchy, Multigrid)):
        return preconditioner
    raise ValueError("%s: preconditioner must be None, an ops.Multigrid(...) or a fitting hierarchy (multigrid_hierarchy_liquid / "
                     "multigrid_hierarchy_diffusion), got preconditioner=%r; the string 'mg' serves the smoke projections (solve_pressure, "
                     "smoke_step, simulate_smoke) only" % (who, preconditioner))


def _hierarchy_for(preconditioner, v, bnd, flags, osd, who, system="smoke", systems=None):
    """the hierarchy a smoke solve on ``v`` uses: built here for ``"mg"`` or a ``Multigrid``, or the caller's, which must fit the call --
    its ``system`` too (``systems``: the number of systems of the call, default the entries of ``v``)"""
    if not isinstance(preconditioner, MultigridHierarchy):
        return multigrid_hierarchy(v, bnd, flags, osd, alpha=preconditioner.alpha if isinstance(preconditioner, Multigrid) else DEFAULT_MG_ALPHA)
    h = preconditioner
    systems = v.shape[0] if systems is None else systems
    if h.system != system:
        raise ValueError("%s: the hierarchy holds the %r system, the call solves the %r system" % (who, h.system, system))
    if h.shape != tuple(v.shape[1:-1]) or h.batch != systems or h.bnd != int(bnd) or h.device != v.device or h.open_sides != osd:
        raise ValueError("%s: the hierarchy was built for shape %s, batch %d, bnd %d, open sides %d on %s; the call has shape %s, batch %d, "
                         "bnd %d, open sides %d on %s" % (who, h.shape, h.batch, h.bnd, h.open_sides, h.device, tuple(v.shape[1:-1]),
                                                          systems, int(bnd), osd, v.device))
    return h


def solve_pressure(vel, bnd=1, accuracy=1e-4, max_iter=None, check_every=None, out=None, workspace=None, obstacle=None, open_bound=None,
                   preconditioner=None):
    """Make ``vel`` [B,(Z,)Y,X,D] divergence free inside a closed box: plain conjugate gradients on the Neumann Laplacian of the interior
    cells from p = 0, every batch entry on its own until its ``max|r| <= accuracy`` or ``max_iter`` iterations (default
    ``int(10*max(extent))``, times 4 in 2-D), then ``vel -= grad p`` with the wall faces 0.  The wall faces of ``vel`` must be 0 already
    (``wall_buoyancy``).  All scalars of the iteration stay on the device; the host reads one word, the number of entries still
    iterating, every ``check_every`` iterations (the result does not depend on it).  mantaflow preconditions with MIC(0), this solver
    does not: both stop at the same criterion, so the fields agree to the solve's accuracy and not beyond.
    Returns ``(vel_projected, pressure, iterations)``; ``iterations`` is an int32 tensor [B].  ``out`` may be ``vel``.
    ``obstacle``: a mask or the flags of ``obstacle_flags``; the Laplacian then lives on the fluid cells (every connected fluid region is
    its own singular system), the solid faces of ``vel`` must be 0 already and stay 0, and the pressure is 0 outside the fluid.
    ``open_bound``: the open sides (see ``open_sides``); p = 0 in open cells (Dirichlet), so a fluid region that touches one is a
    non-singular system, the faces between fluid and open cells are corrected too (every fluid cell ends divergence free -- mantaflow,
    as far as can be recalled, leaves those faces alone), and the open cells are filled (zero gradient) before returning.
    ``preconditioner``: ``"mg"``, an ``ops.Multigrid`` (``"mg"`` with its ``alpha``) or the hierarchy of ``multigrid_hierarchy`` for this geometry makes it multigrid-preconditioned
    conjugate gradients (one V-cycle per iteration, include/deepfluids_hip.h); it stops on the same unscaled ``max|r|``, so the fields
    agree with the plain solve's to the accuracy and not beyond; ``check_every`` then defaults to 4.  A hierarchy passed in is checked
    for shape, batch, ``bnd``, open sides and device; it must also have been built for the SAME ``obstacle``, which is NOT checked (a
    hierarchy of another obstacle is still a symmetric preconditioner of the wrong matrix: the result stays within the accuracy, the
    solve only takes more iterations).  With ``None`` nothing of it is allocated or launched."""
    pre = _preconditioner_arg(preconditioner, "solve_pressure")
    with torch.no_grad():
        v, nd = _smoke_vel(vel, "solve_pressure")
        osd = open_sides(open_bound, nd)
        if int(bnd) != bnd or bnd < 1:
            raise ValueError("solve_pressure: bnd must be an integer >= 1, got %r" % (bnd,))
        if pre is not None and check_every is None:
            check_every = DEFAULT_MG_CHECK_EVERY
        s = _solve_begin("solve_pressure", v, nd, accuracy, max_iter, check_every, workspace if workspace is not None else pressure_workspace(v))
        out = _smoke_out(out, v, "solve_pressure")
        dims, ws, nbytes, bnd = list(v.shape[:-1]), s.ws, s.nbytes, int(bnd)
        pressure = _empty(dims, v)
        # with obstacles: the `_flags` twin of every launch, the flags pointer right after the array arguments
        flags = None if obstacle is None else _obstacle_arg(obstacle, dims, bnd, "solve_pressure")     # held until the last launch
        fl = [] if flags is None else [_ptr(flags)]
        sfx = "%dd" % nd + ("_flags" if fl else "")
        call("df_pressure_init" + sfx, _ptr(v), _ptr(pressure), _ptr(ws), nbytes, *(fl + dims + [bnd, _stream()]))
        # open sides: only the direction launch (n_c) and the correction differ; their `_open` twins take a nullable flags pointer
        fo = [_ptr(flags) if fl else None]
        if pre is not None:
            # the preconditioned recurrence: z = M r after the init and after every update, r.z in the place of r.r
            h = _hierarchy_for(pre, v, bnd, flags, osd, "solve_pressure")
            mg, hb = [nd] + s.status4, [_ptr(h.block), h.nbytes]

            def direction(k):
                call("df_pressure_cg_direction_mg", _ptr(ws), nbytes, *(hb + fo + mg + [bnd, osd, k, s.acc, s.max_iter, _stream()]))

            def update(k):
                call("df_pressure_cg_update_mg", _ptr(pressure), _ptr(ws), nbytes, *(fo + mg + [bnd, k, _stream()]))
                call("df_pressure_mg_precondition", *(hb + [_ptr(ws), nbytes] + mg + [h.alpha, k, _stream()]))
            call("df_pressure_mg_precondition", *(hb + [_ptr(ws), nbytes] + mg + [h.alpha, -1, _stream()]))
        elif osd:
            def direction(k):
                call("df_pressure_cg_direction%dd_open" % nd, _ptr(ws), nbytes, *(fo + dims + [bnd, osd, k, s.acc, s.max_iter, _stream()]))
        else:
            def direction(k):
                call("df_pressure_cg_direction" + sfx, _ptr(ws), nbytes, *(fl + dims + [bnd, k, s.acc, s.max_iter, _stream()]))
        if pre is None:
            def update(k):
                call("df_pressure_cg_update" + sfx, _ptr(pressure), _ptr(ws), nbytes, *(fl + dims + [bnd, k, _stream()]))
        iters = _cg_loop(direction, update, s)
        if osd:
            call("df_pressure_correct%dd_open" % nd, _ptr(v), _ptr(pressure), _ptr(out), *(fo + dims + [bnd, osd, _stream()]))
            _fill_open(out, nd, bnd, osd)
        else:
            call("df_pressure_correct" + sfx, _ptr(v), _ptr(pressure), _ptr(out), *(fl + dims + [bnd, _stream()]))
        return out, pressure, iters


def default_buoyancy_force(shape, dt, gravity=-4e-3):
    """The ``force`` of ``wall_buoyancy`` for the reference's scene: (0, -gravity * dt * max(extent)[, 0]) -- mantaflow's
    ``-gravity * dt / dx`` with ``dx = 1 / max(gridSize)`` and the scene's ``buoyancy = (0, -4e-3, 0)``.  Restated from memory of
    mantaflow's addBuoyancy; it cannot be checked here."""
    f = [0.0] * len(shape)
    f[1] = -float(gravity) * float(dt) * max(int(n) for n in shape)
    return tuple(f)


def buoyancy_forces(shape, dt, gravities):
    """``default_buoyancy_force`` for one gravity per batch entry: a float32 tensor [B,D] (host), row b =
    ``default_buoyancy_force(shape, dt, gravities[b])``, for the ``force=`` of ``wall_buoyancy``, ``smoke_step`` and ``simulate_smoke``."""
    return torch.tensor([default_buoyancy_force(shape, dt, float(g)) for g in gravities], dtype=torch.float32).reshape(-1, len(shape))


class _SmokeSettings(object):
    """What a smoke step needs besides ``d``, ``v`` (the checked inputs), prepared once per ``smoke_step`` call or ``simulate_smoke``
    sequence of ``steps`` (``who``): the open sides, the force, the source as the sequence forms hold it, the buffers allocated once for
    the shape, the obstacle packed into flags, the velocity stamp, and the scalars of the call."""

    def __init__(self, who, density, vel, steps, dt, source, force, order, clamp_mode, bnd, accuracy, max_iter, check_every, obstacle, open_bound,
                 inflow_velocity, preconditioner=None):
        pre = _preconditioner_arg(preconditioner, who)
        d, v, nd = _advect_dims(density, vel)
        self.d, self.v = d, v
        self.osd = open_sides(open_bound, nd)
        self.force = default_buoyancy_force(d.shape[1:], dt) if force is None else force
        self.mask = mask = _source_arg(source, d)
        if steps is not None and isinstance(mask, SphereSource) and mask.centers.dim() == 3 and mask.centers.shape[0] < int(steps):
            raise ValueError("%s: %d frames of source centres for %d steps" % (who, mask.centers.shape[0], int(steps)))
        self.adv = advect_workspace(d, order, mask is not None)
        self.fwd = torch.empty((v.numel(),), dtype=torch.float32, device=v.device) if order == 2 else None
        self.pws = pressure_workspace(v)
        self.flags = _obstacle_arg(obstacle, d.shape, bnd, who) if obstacle is not None else None
        self.vstamp = _inflow_velocity_arg(inflow_velocity, v, nd)
        self.dt, self.order, self.clamp_mode, self.bnd = dt, order, clamp_mode, bnd
        self.accuracy, self.max_iter, self.check_every = accuracy, max_iter, check_every
        # the multigrid hierarchy, built once per sequence (None: nothing is allocated)
        self.pre = None if pre is None else _hierarchy_for(pre, v, bnd, self.flags, self.osd, who)


def _smoke_step(cfg, d, v, d_out, v_out, mask, time=0.0, v_stamped=None):
    dt, bnd, flags, osd = cfg.dt, cfg.bnd, cfg.flags, cfg.osd
    how = dict(order=cfg.order, clamp_mode=cfg.clamp_mode, bnd=bnd, obstacle=flags)
    if cfg.vstamp is None:
        advect(d, v, dt, source=mask, out=d_out, workspace=cfg.adv, time=time, **how)
    else:
        # the script's order: density inflow, velocity stamp (into ``v_stamped``, which may be ``v``), then both advections through it
        n = d.numel()
        if mask is not None:
            stamped = cfg.adv[:n].view(d.shape)
            _stamp(d, mask, 1.0, stamped, time, bnd)
            d = stamped
        v = stamp_velocity(v, cfg.vstamp[0], cfg.vstamp[1], out=v_stamped)
        advect(d, v, dt, out=d_out, workspace=cfg.adv[n:] if mask is not None else cfg.adv, **how)
    advect_velocity(v, dt, out=v_out, workspace=cfg.fwd, open_bound=osd, **how)
    wall_buoyancy(v_out, d_out, cfg.force, bnd=bnd, out=v_out, obstacle=flags, open_bound=osd)
    _, _, iters = solve_pressure(v_out, bnd=bnd, accuracy=cfg.accuracy, max_iter=cfg.max_iter, check_every=cfg.check_every, out=v_out,
                                 workspace=cfg.pws, obstacle=flags, open_bound=osd, preconditioner=cfg.pre)
    return iters


def smoke_step(density, vel, dt, source=None, force=None, order=2, clamp_mode=2, bnd=1, accuracy=1e-4, max_iter=None, check_every=None,
               obstacle=None, open_bound=None, time=0.0, inflow_velocity=None, preconditioner=None):
    """One frame of the reference's smoke scene (scene/smoke_pos_size.py:187-195) on ``density`` [B,(Z,)Y,X] and the MAC velocity ``vel``
    [B,(Z,)Y,X,D] of a closed box: stamp ``source`` (a mask) with 1, advect the density and the velocity through the OLD velocity, zero
    the wall faces, add buoyancy (``force``; default ``default_buoyancy_force``), project.  Returns new ``(density, vel)``.
    ``obstacle`` (a mask of solid cells or the flags of ``obstacle_flags``) makes it the loop of scene/smoke3_obs_buo.py:211-219: the same
    statements with the obstacle in the flag grid, the solid faces 0 after the walls and after the projection.  ``source`` may be a
    ``SphereSource`` [B,D].  ``open_bound`` (see ``open_sides``) makes it the loop of scene/smoke3_rot.py / smoke3_mov.py: the velocity
    steps treat those sides as open; the density needs nothing, its band is 0 after every advection (``resetOutflow``).
    With a ``NoiseInflow`` source (evaluated at solver time ``time``), ``inflow_velocity=(shape, values)`` (a ``CylinderShape`` and the
    [B,D] or [D] values ``stamp_velocity`` writes) and ``force`` a tensor [B,D] it is the loop of scene/smoke3_vel_buo.py:222-232: density
    inflow, velocity stamp, both advections through the STAMPED velocity, walls, buoyancy, projection.  ``vel`` itself is never written.
    ``preconditioner``: as for ``solve_pressure``."""
    with torch.no_grad():
        cfg = _SmokeSettings("smoke_step", density, vel, None, dt, source, force, order, clamp_mode, bnd, accuracy, max_iter, check_every, obstacle,
                             open_bound, inflow_velocity, preconditioner)
        d_out, v_out = torch.empty_like(cfg.d), torch.empty_like(cfg.v)
        _smoke_step(cfg, cfg.d, cfg.v, d_out, v_out, cfg.mask, time)
        return d_out, v_out


def _inflow_velocity_arg(inflow_velocity, v, nd):
    """``(CylinderShape, values [B,D] on the device)`` from the ``inflow_velocity=`` keyword, or None"""
    if inflow_velocity is None:
        return None
    shape, values = inflow_velocity
    if not isinstance(shape, CylinderShape) or shape.dim != nd:
        raise ValueError("inflow_velocity expects (CylinderShape of %d axes, values)" % nd)
    return shape, _entry_rows(values, v, nd, "inflow_velocity: values")


def _smoke_frames(steps, stats, settings):
    cfg = settings()
    nd, mask = cfg.v.dim() - 2, cfg.mask
    if isinstance(cfg.force, torch.Tensor):
        cfg.force = _entry_rows(cfg.force, cfg.v, nd, "simulate_smoke: force")                             # on the device, once
    d, v = cfg.d.clone(), cfg.v.clone()
    d2, v2 = torch.empty_like(d), torch.empty_like(v)
    for t in range(int(steps)):
        # the working copy ``v`` is stamped in place (v_stamped=v): the caller's vel0 is never written
        iters = _smoke_step(cfg, d, v, d2, v2, _source_frame(mask, t), _source_time(mask, t, cfg.dt), v)
        if stats is not None:
            stats.append(iters)
        d, d2, v, v2 = d2, d, v2, v
        yield d, v


def simulate_smoke(density0, vel0, steps, dt=0.5, source=None, force=None, order=2, clamp_mode=2, bnd=1, accuracy=1e-4, max_iter=None,
                   check_every=None, stack=True, stats=None, obstacle=None, open_bound=None, inflow_velocity=None, preconditioner=None):
    """``steps`` chained ``smoke_step`` frames from ``(density0, vel0)`` (left untouched); every buffer is allocated once.  With
    ``stack`` returns ``(density, vels)``, ``vels`` [steps,B,(Z,)Y,X,D] the velocity after each step; without it returns a generator of
    ``(density, vel)`` per step -- views of buffers the next step overwrites, so copy what is to be kept.  ``stats``: a list that
    receives the iteration counts [B] of every step's solve.  ``obstacle``: as for ``smoke_step``, packed into flags once.  ``source``
    may be a ``SphereSource`` [B,D] or [T,B,D] (step t stamps ``centers[t]``); ``open_bound``: as for ``smoke_step``.  A ``NoiseInflow``
    source is evaluated at ``t * dt`` in step t; ``inflow_velocity`` and a ``force`` tensor [B,D]: as for ``smoke_step`` (the stamp goes
    into the sequence's own working buffer).  ``preconditioner``: as for ``solve_pressure``; ``"mg"`` builds the hierarchy once for the
    sequence."""
    _preconditioner_arg(preconditioner, "simulate_smoke")
    with torch.no_grad():
        gen = _smoke_frames(steps, stats, lambda: _SmokeSettings("simulate_smoke", density0, vel0, steps, dt, source, force, order, clamp_mode, bnd,
                                                                 accuracy, max_iter, check_every, obstacle, open_bound, inflow_velocity,
                                                                 preconditioner))
        if not stack:
            return _no_grad_iter(gen)
        vels = torch.empty((int(steps),) + tuple(vel0.shape), dtype=torch.float32, device=vel0.device)
        d = density0
        for t, (d, v) in enumerate(gen):
            vels[t].copy_(v)
        return (d.clone() if int(steps) > 0 else density0.clone()), vels


def _no_grad_iter(gen):
    while True:
        with torch.no_grad():
            try:
                item = next(gen)
            except StopIteration:
                return
        yield item


# ---- a liquid carried through a velocity field (the advect() mode of the reference's liquid scene scripts, scene/liquid3_vis.py:47-148,
#      scene/liquid_pos_size.py:47-132): marker particles traced with RK4, a union level set rebuilt from them.  Inference only, no
#      autograd.  The step is defined in include/deepfluids_hip.h; mantaflow, which the reference calls for it, cannot be run here, so
#      bit parity with it is not claimed.  Left out: extrapolateMACSimple, markFluidCells, resetOutflow, adjustNumber resampling;
#      meshing is ``extract_surface`` below (this project's own marching tetrahedra); the frame loop uses the union form (the one the 2-D script carries commented out), the averaged form with phi.setBound
#      is ``particle_levelset_averaged`` ----
def _particle_pos(pos, who):
    p = _prep(pos.detach(), "pos")
    if p.dim() != 3 or p.shape[-1] not in (2, 3):
        raise ValueError("%s expects positions [B,N,2|3], got %s" % (who, tuple(p.shape)))
    return p


def _grid_shape(shape, nd, who):
    shape = tuple(int(n) for n in shape)
    if len(shape) != nd:
        raise ValueError("%s: positions of %d coordinates need a grid shape of %d extents, got %s" % (who, nd, nd, shape))
    return shape


def _ragged_arg(pos, entry_start, who):
    """``(pos viewed [B,N,D], entry_start)`` of a ragged batch ``pos`` [P,D], ``entry_start`` [B+1] int32 -- checked before anything
    asks where the tensors live, so a bad argument is refused without a GPU"""
    if not isinstance(entry_start, torch.Tensor) or entry_start.dtype != torch.int32 or entry_start.dim() != 1 or entry_start.numel() < 2:
        raise ValueError("%s: entry_start must be an int32 tensor [B+1], got %s" %
                         (who, "%s %s" % (entry_start.dtype, tuple(entry_start.shape)) if isinstance(entry_start, torch.Tensor) else type(entry_start)))
    if not isinstance(pos, torch.Tensor) or pos.dim() != 2 or pos.shape[-1] not in (2, 3):
        raise ValueError("%s: a ragged batch holds its particles as [P,2|3], got %s" % (who, tuple(pos.shape) if isinstance(pos, torch.Tensor) else type(pos)))
    B = entry_start.numel() - 1
    if pos.shape[0] % B:
        raise ValueError("%s: P = %d rows are not a multiple of B = %d (entry_start has %d elements)" % (who, pos.shape[0], B, B + 1))
    if not pos.is_cuda or not entry_start.is_cuda or entry_start.device != pos.device or not entry_start.is_contiguous():
        raise _lib.DeepFluidsHipError("%s: pos and entry_start must be contiguous tensors on the same GPU" % who)
    return _prep(pos.detach(), "pos").view(B, pos.shape[0] // B, pos.shape[1]), entry_start


def pack_particles(parts, capacity=None):
    """A ragged particle batch from a list of B tensors [N_b,D] (float32, on the GPU): ``(pos [P,D], entry_start [B+1] int32)`` with
    entry b in rows ``entry_start[b] .. entry_start[b+1] - 1`` and the rows from ``entry_start[B]`` on unused (zeros here; they hold no
    meaning).  ``capacity``: P, at least the total and a multiple of B; by default the total rounded up to a multiple of B."""
    parts = list(parts)
    B = len(parts)
    if B < 1:
        raise ValueError("pack_particles: no entries")
    nd = parts[0].shape[-1] if isinstance(parts[0], torch.Tensor) and parts[0].dim() == 2 else 0
    for t in parts:
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[-1] != nd or nd not in (2, 3) or t.dtype != torch.float32:
            raise ValueError("pack_particles expects float32 tensors [N_b,2|3] of one D")
    counts = [int(t.shape[0]) for t in parts]
    total = sum(counts)
    P = -(-total // B) * B if capacity is None else int(capacity)
    if P < total or P % B:
        raise ValueError("pack_particles: capacity %d must be a multiple of B = %d and hold the %d particles" % (P, B, total))
    pos = torch.zeros((P, nd), dtype=torch.float32, device=parts[0].device)
    if total:
        pos[:total] = torch.cat(parts, dim=0)
    es = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(parts[0].device)
    return pos, es


def unpack_particles(pos, entry_start):
    """The list of B tensors [N_b,D] (views of ``pos`` [P,D]) of a ragged batch; reads ``entry_start`` on the host."""
    if not isinstance(entry_start, torch.Tensor) or entry_start.dtype != torch.int32 or entry_start.dim() != 1 or entry_start.numel() < 2:
        raise ValueError("unpack_particles: entry_start must be an int32 tensor [B+1]")
    if not isinstance(pos, torch.Tensor) or pos.dim() != 2:
        raise ValueError("unpack_particles: a ragged batch holds its particles as [P,D]")
    es = [int(x) for x in entry_start.cpu().numpy()]
    if es[0] < 0 or es[-1] > pos.shape[0] or any(b < a for a, b in zip(es, es[1:])):
        raise ValueError("unpack_particles: entry_start %s does not describe %d rows" % (es, pos.shape[0]))
    return [pos[a:b] for a, b in zip(es, es[1:])]


def advect_particles(pos, vel, dt, bnd=1, vel_scale=1.0, out=None, entry_start=None):
    """One RK4 trace of the particles ``pos`` [B,N,D] (cell units, xyz order) through ``vel`` [B,(Z,)Y,X,D] (MAC face values, times
    ``vel_scale``), then clamped to [bnd, extent - bnd - 2^-10] per axis -- modelled on mantaflow's ``pp.advectInGrid(IntRK4,
    deleteInObstacle=False)`` (scene/liquid3_vis.py:134), NOT bit-identical to it; include/deepfluids_hip.h holds the definition that
    is tested.  Returns the new positions (``out`` if given; it may be ``pos`` itself).
    ``entry_start`` [B+1] int32 (``pack_particles``): ``pos`` is a ragged batch [P,D]; unused rows are neither read nor written."""
    with torch.no_grad():
        if entry_start is not None:
            p, es = _ragged_arg(pos, entry_start, "advect_particles")
            v = _liquid_vel(vel, p.shape[0], p.shape[-1], "advect_particles")
            if int(bnd) != bnd or bnd < 0:
                raise ValueError("advect_particles: bnd must be an integer >= 0, got %r" % (bnd,))
            if out is None:
                out = torch.empty_like(pos)
            elif tuple(out.shape) != tuple(pos.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
                raise ValueError("advect_particles: out must be a contiguous float32 GPU tensor of the positions' shape")
            call("df_particles_advect%dd_ragged" % p.shape[-1], _ptr(p), _ptr(out), _ptr(v), _ptr(es), p.shape[0], p.shape[1],
                 *(list(v.shape[1:-1]) + [float(dt), float(vel_scale), int(bnd), _stream()]))
            return out
        p = _particle_pos(pos, "advect_particles")
        v = _prep(vel.detach(), "vel")
        B, N, nd = p.shape
        if v.dim() != nd + 2 or v.shape[0] != B or v.shape[-1] != nd:
            raise ValueError("advect_particles expects a velocity [%d,%s%d] for positions %s, got %s" %
                             (B, "Z,Y,X," if nd == 3 else "Y,X,", nd, tuple(p.shape), tuple(v.shape)))
        if int(bnd) != bnd or bnd < 0:
            raise ValueError("advect_particles: bnd must be an integer >= 0, got %r" % (bnd,))
        if out is None:
            out = torch.empty_like(p)
        elif tuple(out.shape) != tuple(p.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("advect_particles: out must be a contiguous float32 GPU tensor of the positions' shape")
        call("df_particles_advect%dd" % nd, _ptr(p), _ptr(out), _ptr(v), B, N, *(list(v.shape[1:-1]) + [float(dt), float(vel_scale), int(bnd), _stream()]))
        return out


def particle_cells(pos, shape, entry_start=None):
    """The cell index of mantaflow's ``gridParticleIndex``: ``(sorted_pos [B,N,D], cell_start [B*ncell + 1] int32, order [B*N] int64)``
    for positions ``pos`` [B,N,D] on a grid ``shape`` [(Z,)Y,X].  Keys (batch entry, cell) come from a HIP kernel, the stable sort and
    the ranges from torch, the permutation of the positions from a HIP kernel again: ``sorted_pos.view(-1, D) == pos.view(-1, D)[order]``
    and the particles of key c are rows ``cell_start[c] .. cell_start[c+1] - 1``, in their original index order.
    ``entry_start`` [B+1] int32: ``pos`` is a ragged batch [P,D] (and so is ``sorted_pos``).  Unused rows get the key B*ncell and sort
    behind every cell; the stable sort keeps the entries contiguous and in order, so ``entry_start`` describes ``sorted_pos`` too, and
    ``cell_start[-1]`` is the live total."""
    with torch.no_grad():
        if entry_start is not None:
            p, es = _ragged_arg(pos, entry_start, "particle_cells")
        else:
            p = _particle_pos(pos, "particle_cells")
        B, N, nd = p.shape
        shape = _grid_shape(shape, nd, "particle_cells")
        ncell = int(np.prod(shape))
        keys = torch.empty((B * N,), dtype=torch.int32, device=p.device)
        if entry_start is not None:
            call("df_particles_cell_keys%dd_ragged" % nd, _ptr(p), _ptr(keys), _ptr(es), B, N, *(list(shape) + [_stream()]))
        else:
            call("df_particles_cell_keys%dd" % nd, _ptr(p), _ptr(keys), B, N, *(list(shape) + [_stream()]))
        skeys, order = torch.sort(keys, stable=True)
        spos = torch.empty_like(p if entry_start is None else pos)
        call("df_particles_gather", _ptr(p), _ptr(order), _ptr(spos), B * N, nd, _stream())
        edges = torch.arange(B * ncell + 1, dtype=torch.int32, device=p.device)
        cell_start = torch.searchsorted(skeys, edges, out_int32=True)
        return spos, cell_start, order


def particle_levelset(pos, shape, radius_factor=1.0, out=None):
    """The surface level set of the particles ``pos`` [B,N,D] on a grid ``shape``: phi [B,(Z,)Y,X] = min(radius, min over the particles
    within +-((int)radius_factor + 1) cells of |cell centre - p| - radius), radius = 0.5*sqrt(D)*(radius_factor + 0.01) -- modelled on
    mantaflow's ``gridParticleIndex`` + ``unionParticleLevelset`` (scene/liquid3_vis.py:112-113), NOT bit-identical to it.  Negative
    inside the liquid.  No particles: phi = radius everywhere."""
    with torch.no_grad():
        p = _particle_pos(pos, "particle_levelset")
        B, N, nd = p.shape
        shape = _grid_shape(shape, nd, "particle_levelset")
        if out is None:
            out = _empty((B,) + shape, p)
        elif tuple(out.shape) != (B,) + shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("particle_levelset: out must be a contiguous float32 GPU tensor %s" % ((B,) + shape,))
        spos, cell_start, _ = particle_cells(p, shape)
        call("df_particle_levelset_union%dd" % nd, _ptr(spos), _ptr(cell_start), _ptr(out), B, N, *(list(shape) + [float(radius_factor), _stream()]))
        return out


def _levelset_averaged(spos, cell_start, out, tmp, radius_factor, smooth, smooth_neg, bound_value, bnd):
    """the launches of ``particle_levelset_averaged`` on sorted particles, into ``out`` [B,(Z,)Y,X]; ``tmp`` is a second buffer of its
    shape (None without smoothing passes).  The passes alternate between the two buffers and end in ``out``; the band is fused into the
    last one."""
    dims = list(out.shape)
    B, shape = dims[0], dims[1:]
    nd = len(shape)
    N = spos.numel() // (B * nd)
    passes = [1] * smooth + [2] * smooth_neg
    bufs = (out, tmp) if len(passes) % 2 == 0 else (tmp, out)
    cur = bufs[0]
    call("df_particle_levelset_averaged%dd" % nd, _ptr(spos), _ptr(cell_start), _ptr(cur), B, N, *(shape + [float(radius_factor), _stream()]))
    for n, mode in enumerate(passes):
        nxt = bufs[(n + 1) % 2]
        call("df_levelset_smooth%dd" % nd, _ptr(cur), _ptr(nxt), *(dims + [mode, bnd if n == len(passes) - 1 else 0, float(bound_value), _stream()]))
        cur = nxt
    if not passes and bnd > 0:
        call("df_levelset_smooth%dd" % nd, _ptr(out), _ptr(out), *(dims + [0, bnd, float(bound_value), _stream()]))
    return out


def particle_levelset_averaged(pos, shape, radius_factor=1.0, smooth=1, smooth_neg=1, bound_value=1.0, bnd=1, out=None, cells=None,
                               entry_start=None):
    """The averaged surface level set of the particles ``pos`` [B,N,D] on a grid ``shape`` -- modelled on mantaflow's
    ``averagedParticleLevelset(pp, pindex, flags, gpi, phi, radius_factor, smooth, smooth_neg)`` followed by ``phi.setBound(bound_value,
    bnd)`` (scene/liquid_pos_size.py:254-295), restated from memory and NOT bit-identical to it; include/deepfluids_hip.h holds the
    definition that is tested, against tests/liquid_gf_ref.py.  With R = 0.5*sqrt(D)*(radius_factor + 0.01) and w = max(0, 1 -
    |x_c - p|^2 / (4 R^2)) over the particles of the cells within +-(int(R) + 1) of cell c: phi = |x_c - sum(w p) / sum(w)| - R where
    sum(w) > 1e-6, else R.  Then ``smooth`` passes of the (2D+1)-point average on every cell off the outermost layer, ``smooth_neg``
    passes of the same average kept only where it is smaller, and the ``bnd``-wide band set to ``bound_value`` (``bnd=0``: no band).
    ``cells=(sorted_pos, cell_start)`` of ``particle_cells`` reuses a sort already done (``pos`` is then only read for its shape).  The
    sums run in ascending cell order and, inside a cell, in sorted order: deterministic, no atomics.
    ``entry_start`` [B+1] int32: ``pos`` (and ``cells[0]``) is a ragged batch [P,D]; the kernels are driven by ``cell_start`` alone."""
    with torch.no_grad():
        smooth, smooth_neg = int(smooth), int(smooth_neg)
        if smooth < 0 or smooth_neg < 0:
            raise ValueError("particle_levelset_averaged: smooth and smooth_neg must be >= 0, got %r, %r" % (smooth, smooth_neg))
        if int(bnd) != bnd or bnd < 0:
            raise ValueError("particle_levelset_averaged: bnd must be an integer >= 0, got %r" % (bnd,))
        if not 0.0 <= radius_factor <= 1024.0:
            raise ValueError("particle_levelset_averaged: radius_factor must lie in [0, 1024], got %r" % (radius_factor,))
        if entry_start is not None:
            p, _ = _ragged_arg(pos, entry_start, "particle_levelset_averaged")
        else:
            p = _particle_pos(pos, "particle_levelset_averaged")
        B, N, nd = p.shape
        shape = _grid_shape(shape, nd, "particle_levelset_averaged")
        if out is None:
            out = _empty((B,) + shape, p)
        elif tuple(out.shape) != (B,) + shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("particle_levelset_averaged: out must be a contiguous float32 GPU tensor %s" % ((B,) + shape,))
        if cells is None:
            spos, cell_start, _ = particle_cells(pos if entry_start is not None else p, shape, entry_start=entry_start)
        else:
            spos, cell_start = cells
            spos = _ragged_arg(spos, entry_start, "particle_levelset_averaged")[0] if entry_start is not None else \
                _particle_pos(spos, "particle_levelset_averaged")
            if tuple(spos.shape) != tuple(p.shape):
                raise ValueError("particle_levelset_averaged: cells hold positions %s for positions %s" % (tuple(spos.shape), tuple(p.shape)))
            if (cell_start.dtype != torch.int32 or not cell_start.is_cuda or not cell_start.is_contiguous()
                    or cell_start.numel() != B * int(np.prod(shape)) + 1):
                raise ValueError("particle_levelset_averaged: cells[1] must be the int32 GPU tensor [B*ncell + 1] of particle_cells")
        tmp = torch.empty_like(out) if smooth + smooth_neg else None
        return _levelset_averaged(spos, cell_start, out, tmp, radius_factor, smooth, smooth_neg, bound_value, int(bnd))


def liquid_sequence(pos0, vels, dt, bnd=1, vel_scale=1.0, radius_factor=1.0, images=False, on_frame=None):
    """The frame loop of the liquid scenes' ``advect()`` (scene/liquid3_vis.py:100-148) over ``vels`` [T,B,(Z,)Y,X,D] (a tensor or a
    sequence of T tensors): per frame build the level set of the current particles, optionally render it with ``density_image`` (the
    ``l_adv`` frame: clipped where the reference's cast wraps), then trace the particles through the frame's velocity.  ``pos0`` is left
    untouched.  Returns ``(final positions [B,N,D], last phi [B,(Z,)Y,X])`` -- the last phi is the level set of the positions BEFORE the
    last trace, as in the reference's loop -- and with ``images`` also the uint8 frames [T,B,Y,X], copied to the host once.
    ``on_frame(t, phi)``: called for every frame with the level set just built, before the trace; phi is the loop's one buffer, to be
    read (``extract_surface``) and not kept or written.  Without it the loop allocates and launches what it always did."""
    with torch.no_grad():
        T = len(vels)
        if T < 1:
            raise ValueError("liquid_sequence: no velocity frames")
        cur = _particle_pos(pos0, "liquid_sequence").clone()
        shape = tuple(vels[0].shape[1:-1])
        phi = _empty((cur.shape[0],) + shape, cur)
        imgs = _u8((T, cur.shape[0], shape[-2], shape[-1]), cur) if images else None
        for t in range(T):
            particle_levelset(cur, shape, radius_factor, out=phi)
            if images:
                density_image(phi, out=imgs[t])
            if on_frame is not None:
                on_frame(t, phi)
            advect_particles(cur, vels[t], dt, bnd=bnd, vel_scale=vel_scale, out=cur)
        if images:
            return cur, phi, imgs.cpu().numpy()
        return cur, phi


def _centres(shape, a):
    """centre coordinate along axis a (0 = x) of every cell, broadcastable against [(Z,)Y,X]"""
    ax = len(shape) - 1 - a
    sh = [1] * len(shape)
    sh[ax] = shape[ax]
    return (np.arange(shape[ax]) + 0.5).reshape(sh)


def box_levelset(shape, p0, p1):
    """Signed distance of the cell centres of a grid ``shape`` [(Z,)Y,X] to the box p0 .. p1 (cell units, xyz order), negative inside
    (mantaflow's ``Box.computeLevelset``); float32, host.  Join two level sets with ``np.minimum``."""
    shape = tuple(int(n) for n in shape)
    if len(shape) not in (2, 3) or len(p0) != len(shape) or len(p1) != len(shape):
        raise ValueError("box_levelset expects a 2-D or 3-D shape and corners of as many coordinates, got %s, %s, %s" % (shape, tuple(p0), tuple(p1)))
    q = []
    for a in range(len(shape)):
        mid, half = 0.5 * (float(p0[a]) + float(p1[a])), 0.5 * (float(p1[a]) - float(p0[a]))
        q.append(np.broadcast_to(np.abs(_centres(shape, a) - mid) - half, shape))
    q = np.stack(q)
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=0))
    return (outside + np.minimum(q.max(axis=0), 0.0)).astype(np.float32)


def sphere_levelset(shape, center, radius):
    """Signed distance of the cell centres of a grid ``shape`` [(Z,)Y,X] to the sphere (cell units, xyz order), negative inside;
    float32, host."""
    shape = tuple(int(n) for n in shape)
    if len(shape) not in (2, 3) or len(center) != len(shape):
        raise ValueError("sphere_levelset expects a 2-D or 3-D shape and a centre of as many coordinates, got %s, %s" % (shape, tuple(center)))
    r2 = np.zeros(shape, np.float64)
    for a, c in enumerate(center):
        r2 = r2 + (_centres(shape, a) - float(c)) ** 2
    return (np.sqrt(r2) - float(radius)).astype(np.float32)


def seed_particles(phi0, discretization=2, randomness=0.05, seed=123, bnd=1):
    """Marker particles of the liquid body ``phi0`` [(Z,)Y,X] (negative inside), after mantaflow's ``sampleLevelsetWithParticles``
    (scene/liquid3_vis.py:89): every cell with phi0 < 0 that is not on the ``bnd`` band gets discretization^D particles at its sub-cell
    centres (i + (s + 0.5)/discretization, ...), each moved by a uniform jitter of +-randomness/discretization per axis drawn from
    ``np.random.RandomState(seed)``.  Cells in [(Z,)Y,X] order, sub-cells likewise with x innermost.  Host NumPy; returns [N,D] float32
    in xyz order."""
    phi0 = np.asarray(phi0)
    nd = phi0.ndim
    if nd not in (2, 3):
        raise ValueError("seed_particles expects a level set [(Z,)Y,X], got %s" % (phi0.shape,))
    disc = int(discretization)
    if disc < 1 or not 0 <= randomness < 0.5:
        raise ValueError("seed_particles: discretization must be >= 1 and randomness in [0, 0.5)")
    inside = phi0 < 0
    for ax, n in enumerate(phi0.shape):
        idx = np.arange(n)
        sh = [1] * nd
        sh[ax] = n
        inside = inside & ((idx >= bnd) & (idx < n - bnd)).reshape(sh)
    cells = np.argwhere(inside)[:, ::-1].astype(np.float64)                                   # [M, D] in xyz order
    sub = np.argwhere(np.ones((disc,) * nd, bool))[:, ::-1].astype(np.float64)                # [disc^D, D], x innermost
    pos = (cells[:, None, :] + (sub[None, :, :] + 0.5) / disc).reshape(-1, nd)
    rng = np.random.RandomState(seed)
    pos = pos + rng.uniform(-1.0, 1.0, size=pos.shape) * (float(randomness) / disc)
    return pos.astype(np.float32)


# ---- the liquid solver step (the main() loops of the reference's liquid scenes, scene/liquid_pos_size.py:254-295 and
#      scene/liquid3_d_r.py): FLIP.  The step is defined in include/deepfluids_hip.h (tests/liquid_ref.py restates it); mantaflow cannot
#      be run here, so parity with it is not claimed.  By default p = 0 sits at the air cell centres (a first-order surface);
#      ``ghost_fluid=True`` adds averagedParticleLevelset / phi.setBound and the ghost-fluid surface of solvePressure(phi=)
#      (tests/liquid_gf_ref.py restates them).  Left out: adjustNumber resampling (N is constant), extrapolateLsSimple, resetOutflow
#      and open sides, obstacles inside the liquid, MIC(0), per-entry particle counts (one call, one N) ----
DEFAULT_FLIP_RATIO = 0.97


def _liquid_vel(vel, B, nd, who):
    v = _prep(vel.detach(), "vel")
    if v.dim() != nd + 2 or v.shape[0] != B or v.shape[-1] != nd:
        raise ValueError("%s expects a velocity [%d,%s%d], got %s" % (who, B, "Z,Y,X," if nd == 3 else "Y,X,", nd, tuple(v.shape)))
    return v


def _liquid_bnd(bnd, who):
    if int(bnd) != bnd or bnd < 1:
        raise ValueError("%s: bnd must be an integer >= 1, got %r" % (who, bnd))
    return int(bnd)


def _marks(t, like, who):
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(like.shape):
        raise ValueError("%s: marks must be a contiguous uint8 GPU tensor of shape %s" % (who, tuple(like.shape)))
    return t


def particles_to_grid(pos_sorted, pvel_sorted, cell_start, shape):
    """mantaflow's ``mapPartsToMAC`` as a gather: ``(vel, weight, known)`` on a grid ``shape`` [(Z,)Y,X] from particles SORTED by cell
    (``particle_cells``; ``pvel`` permuted by the same order).  Component a of a face is ``sum(w * pvel_a) / sum(w)`` over the
    particles whose ``u(p)`` reads that face, w the weight of that read (the scatter is the transpose of the sample of
    ``advect_particles``), 0 where ``sum(w)`` is 0; ``weight`` is ``sum(w)``, ``known`` (uint8) marks ``weight > 0``.  The sums run in
    ascending cell order and, inside a cell, in sorted order: deterministic, no atomics."""
    with torch.no_grad():
        p = _particle_pos(pos_sorted, "particles_to_grid")
        u = _particle_pos(pvel_sorted, "particles_to_grid")
        B, N, nd = p.shape
        if tuple(u.shape) != tuple(p.shape):
            raise ValueError("particles_to_grid: velocities %s for positions %s" % (tuple(u.shape), tuple(p.shape)))
        shape = _grid_shape(shape, nd, "particles_to_grid")
        ncell = int(np.prod(shape))
        if cell_start.dtype != torch.int32 or not cell_start.is_cuda or not cell_start.is_contiguous() or cell_start.numel() != B * ncell + 1:
            raise ValueError("particles_to_grid: cell_start must be the int32 GPU tensor [B*ncell + 1] of particle_cells")
        vel = _empty((B,) + shape + (nd,), p)
        weight = torch.empty_like(vel)
        known = torch.empty(vel.shape, dtype=torch.uint8, device=p.device)
        call("df_liquid_p2g%dd" % nd, _ptr(p), _ptr(u), _ptr(cell_start), _ptr(vel), _ptr(weight), _ptr(known), B, N,
             *(list(shape) + [_stream()]))
        return vel, weight, known


def extrapolate_mac(vel, known, distance, bnd=1):
    """mantaflow's ``extrapolateMACFromWeight`` / ``extrapolateMACSimple`` in one form: ``known`` [B,(Z,)Y,X,D] uint8 marks the faces that
    hold a value (1) or not (0).  For layer d = 1..distance an unknown face between two interior cells takes the mean of its axis
    neighbours (x-, x+, y-, y+[, z-, z+]) marked 1..d and the mark d + 1; wall faces are never filled.  One launch per layer between
    two buffers.  Returns new ``(vel, marks)``; the inputs are left untouched."""
    with torch.no_grad():
        v, nd = _smoke_vel(vel, "extrapolate_mac")
        bnd = _liquid_bnd(bnd, "extrapolate_mac")
        m = _marks(known, v, "extrapolate_mac")
        distance = int(distance)
        if not 0 <= distance <= 254:
            raise ValueError("extrapolate_mac: distance must be in 0..254, got %r" % (distance,))
        dims = list(v.shape[:-1])
        cur = (v.clone(), m.clone()) if distance == 0 else (v, m)
        bufs = [(torch.empty_like(v), torch.empty_like(m)) for _ in range(min(distance, 2))]
        for d in range(1, distance + 1):
            nxt = bufs[(d - 1) % 2]
            call("df_mac_extrapolate%dd" % nd, _ptr(cur[0]), _ptr(cur[1]), _ptr(nxt[0]), _ptr(nxt[1]), *(dims + [bnd, d, _stream()]))
            cur = nxt
        return cur


def liquid_flags(cell_start, shape, batch, n_particles, bnd=1):
    """mantaflow's ``markFluidCells`` from the ranges of ``particle_cells``: ``(flags, touch)``.  An interior cell is liquid when it
    holds a particle, every other interior cell is air.  ``flags`` [B,(Z,)Y,X] uint8 has the layout of ``obstacle_flags`` (bit 0: the
    cell is liquid, bits 1..6: that neighbour is); ``touch`` [B,(Z,)Y,X,D] uint8 marks the faces with a liquid cell on either side."""
    with torch.no_grad():
        shape = tuple(int(n) for n in shape)
        nd = len(shape)
        if nd not in (2, 3):
            raise ValueError("liquid_flags expects a grid shape [(Z,)Y,X], got %s" % (shape,))
        bnd = _liquid_bnd(bnd, "liquid_flags")
        B, ncell = int(batch), int(np.prod(shape))
        if cell_start.dtype != torch.int32 or not cell_start.is_cuda or not cell_start.is_contiguous() or cell_start.numel() != B * ncell + 1:
            raise ValueError("liquid_flags: cell_start must be the int32 GPU tensor [B*ncell + 1] of particle_cells")
        flags = torch.empty((B,) + shape, dtype=torch.uint8, device=cell_start.device)
        touch = torch.empty((B,) + shape + (nd,), dtype=torch.uint8, device=cell_start.device)
        call("df_liquid_flags%dd" % nd, _ptr(cell_start), _ptr(flags), _ptr(touch), B, int(n_particles), *(list(shape) + [bnd, _stream()]))
        return flags, touch


def _liquid_flags_arg(flags, v, who):
    if flags.dtype != torch.uint8 or not flags.is_cuda or not flags.is_contiguous() or tuple(flags.shape) != tuple(v.shape[:-1]):
        raise ValueError("%s: flags must be the uint8 GPU tensor %s of liquid_flags" % (who, tuple(v.shape[:-1])))
    return flags


def liquid_forces(vel, flags, force, bnd=1, out=None):
    """``addGravity`` + ``setWallBcs`` in one element-wise pass: a face with a wall cell becomes 0, a face between two interior cells of
    which at least one is liquid gets ``+ force[a]``, every other face is left unchanged.  ``force``: D numbers in cells per step.
    ``out`` may be ``vel``."""
    with torch.no_grad():
        v, nd = _smoke_vel(vel, "liquid_forces")
        bnd = _liquid_bnd(bnd, "liquid_forces")
        fl = _liquid_flags_arg(flags, v, "liquid_forces")
        f = [float(x) for x in force]
        if len(f) != nd:
            raise ValueError("liquid_forces: force must have %d components, got %r" % (nd, force))
        out = _smoke_out(out, v, "liquid_forces")
        call("df_liquid_forces%dd" % nd, _ptr(v), _ptr(fl), _ptr(out), *(list(v.shape[:-1]) + f + [bnd, _stream()]))
        return out


def default_gravity_force(shape, dt, gravity=-1e-3):
    """The ``force`` of ``liquid_forces`` for the reference's liquid scenes: (0, gravity * dt * max(extent)[, 0]) -- mantaflow's
    ``gravity * dt / dx`` with ``dx = 1 / max(gridSize)`` and the scenes' ``gravity = -1e-3``, the convention of
    ``default_buoyancy_force``.  Restated from memory of mantaflow's addGravity; it cannot be checked here."""
    f = [0.0] * len(shape)
    f[1] = float(gravity) * float(dt) * max(int(n) for n in shape)
    return tuple(f)


_Solve = collections.namedtuple("_Solve", "ws nbytes status4 count iters acc max_iter check_every")


def _solve_begin(who, v, nd, accuracy, max_iter, check_every, ws, diffusion=False):
    """The head every solve shares: the iteration controls checked and defaulted, the workspace ``ws`` checked, and the words the host
    reads -- the number of systems still iterating and their iteration counts.  A system is a batch entry, or, for a ``diffusion``, an
    (entry, component) pair: ``df_pressure_status`` then runs over the B*D pairs."""
    if not accuracy >= 0:
        raise ValueError("%s: accuracy must be >= 0, got %r" % (who, accuracy))
    dims, dims4 = _pressure_dims(v, nd)
    if max_iter is None:
        max_iter = (default_diffusion_max_iter if diffusion else default_max_iter)(dims[1:])
    check_every = DEFAULT_CHECK_EVERY if check_every is None else int(check_every)
    if max_iter < 0 or check_every < 1:
        raise ValueError("%s: max_iter must be >= 0 and check_every >= 1, got %r, %r" % (who, max_iter, check_every))
    if ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous():
        raise ValueError("%s: workspace must be a contiguous float32 GPU tensor (%s_workspace)" % (who, "diffusion" if diffusion else "pressure"))
    systems = dims[0] * (nd if diffusion else 1)
    words = torch.empty((1 + systems,), dtype=torch.int32, device=v.device)
    return _Solve(ws, ws.numel() * 4, [systems] + dims4[1:], words[:1], words[1:], float(accuracy), int(max_iter), check_every)


def _cg_loop(direction, update, s):
    """the host loop of a solve and its end: ``direction(k)`` and ``update(k)`` launch one iteration's two kernels, the host reads one
    word every ``check_every`` iterations; returns the iteration counts of the systems (a copy)"""
    k = 0
    while True:
        direction(k)
        if k % s.check_every == s.check_every - 1 or k >= s.max_iter:
            call("df_pressure_status", _ptr(s.ws), s.nbytes, *(s.status4 + [k, _ptr(s.count), None, _stream()]))
            if _read_word(s.count) == 0:
                break
        update(k)
        k += 1
    call("df_pressure_status", _ptr(s.ws), s.nbytes, *(s.status4 + [k, None, _ptr(s.iters), _stream()]))
    return s.iters.clone()


def _mg_rows_loop(h, s, nd, update):
    """``_cg_loop`` for the recurrence preconditioned with hierarchy ``h``, whose level 0 also gives the rows of ``q = A p``
    (include/deepfluids_hip_liquid_mg.h): ``z = M r`` after the init and after every ``update(k)``, r.z in the place of r.r"""
    hb, mg = [_ptr(h.block), h.nbytes], [nd] + s.status4

    def precondition(k):
        call("df_pressure_mg_precondition", *(hb + [_ptr(s.ws), s.nbytes] + mg + [h.alpha, k, _stream()]))

    def direction(k):
        call("df_pressure_cg_direction_mg_rows", _ptr(s.ws), s.nbytes, *(hb + mg + [k, s.acc, s.max_iter, _stream()]))

    def step(k):
        update(k)
        precondition(k)
    precondition(-1)
    return _cg_loop(direction, step, s)


def _gf_phi_arg(phi, vel, who):
    """checked against ``vel``'s shape and device before anything asks where ``vel`` lives (a bad phi is refused without a GPU): a
    contiguous float32 tensor of the cells' shape, on a GPU, and on the SAME device as ``vel`` -- the kernels take raw pointers"""
    if not isinstance(vel, torch.Tensor) or vel.dim() < 2:
        raise ValueError("%s expects a velocity tensor [B,(Z,)Y,X,D], got %r" % (who, type(vel)))
    want = tuple(vel.shape[:-1])
    if (not isinstance(phi, torch.Tensor) or phi.dtype != torch.float32 or tuple(phi.shape) != want or not phi.is_cuda
            or phi.device != vel.device or not phi.is_contiguous()):
        raise ValueError("%s: phi must be a contiguous float32 GPU tensor %s on the velocity's device" % (who, want))
    return phi.detach()


def _gf_clamp_arg(gf_clamp, who):
    if not 0.0 < gf_clamp <= 1.0:
        raise ValueError("%s: gf_clamp must lie in (0, 1], got %r" % (who, gf_clamp))
    return float(gf_clamp)


def solve_pressure_liquid(vel, flags, bnd=1, accuracy=1e-4, max_iter=None, check_every=None, out=None, workspace=None, phi=None,
                          gf_clamp=1e-4, preconditioner=None):
    """The free-surface projection: ``solve_pressure`` with rows for the liquid cells of ``flags`` (``liquid_flags``) only and p = 0 in
    the air cells -- n_c counts every neighbour that is interior by its index, the neighbour sums run over the liquid ones.  Faces
    between two interior cells of which at least one is liquid are corrected with p as the array holds it (0 in air), other interior
    faces are left unchanged, wall faces become 0: every liquid cell ends divergence free to the solve's accuracy.  p = 0 sits at the
    air cell centres (first-order surface; mantaflow's ghost-fluid treatment is left out), and there is no preconditioner.  A liquid
    region that touches no air is singular but consistent, as a closed box is.  Returns ``(vel_projected, pressure, iterations)``;
    ``out`` may be ``vel``.
    ``phi`` [B,(Z,)Y,X] (``particle_levelset_averaged``): the ghost-fluid surface of mantaflow's ``solvePressure(phi=phi)``, restated
    from memory; the definition that is tested is the one in include/deepfluids_hip.h (tests/liquid_gf_ref.py), NOT mantaflow.  Between a
    liquid cell i and an interior air neighbour a the surface sits at theta = phi_i / (phi_i - phi_a) of the way (0.5 if phi_i - phi_a
    > -1e-4, else clamped to [``gf_clamp``, 1]): the row of i gets p_i / theta for that neighbour, and the face is corrected with
    p_i / theta.  The solve is then Jacobi-preconditioned CG (the clamp puts diagonals up to 1 / gf_clamp beside diagonals of 4-6),
    stopping on the UNscaled residual as before, and needs ``pressure_workspace(vel, ghost_fluid=True)``.  With ``phi=None`` nothing of
    this is launched.
    ``preconditioner``: an ``ops.Multigrid`` (the hierarchy is then built here from ``flags`` and ``phi``) or a hierarchy of
    ``multigrid_hierarchy_liquid`` built for the SAME flags (and phi), which is NOT checked beyond its system, geometry and device: the
    solve becomes multigrid-preconditioned conjugate gradients on the same matrix (include/deepfluids_hip_liquid_mg.h; with ``phi`` the
    cycle replaces Jacobi), stops on the same unscaled ``max|r|``, and ``check_every`` then defaults to 4.  The string ``"mg"`` is the
    smoke calls' and is refused.  With ``None`` nothing of it is allocated or launched."""
    pre = _liquid_preconditioner_arg(preconditioner, "solve_pressure_liquid")
    with torch.no_grad():
        gf = phi is not None
        if gf:
            gfc = _gf_clamp_arg(gf_clamp, "solve_pressure_liquid")
            phi = _gf_phi_arg(phi, vel, "solve_pressure_liquid")
        v, nd = _smoke_vel(vel, "solve_pressure_liquid")
        bnd = _liquid_bnd(bnd, "solve_pressure_liquid")
        fl = _liquid_flags_arg(flags, v, "solve_pressure_liquid")
        if pre is not None and check_every is None:
            check_every = DEFAULT_MG_CHECK_EVERY
        s = _solve_begin("solve_pressure_liquid", v, nd, accuracy, max_iter, check_every,
                         workspace if workspace is not None else pressure_workspace(v, ghost_fluid=gf))
        out = _smoke_out(out, v, "solve_pressure_liquid")
        dims, ws, nbytes = list(v.shape[:-1]), s.ws, s.nbytes
        pressure = _empty(dims, v)
        # the entry points' twins: `_gf` throughout with phi, which init and correct take after the flags, with the clamp after bnd
        sfx, twin = "%dd_" % nd, ("gf", "gf") if gf else ("flags", "liquid")
        surface = [_ptr(fl)] + ([_ptr(phi)] if gf else []) + dims + [bnd] + ([gfc] if gf else [])
        call("df_pressure_init" + sfx + twin[0], _ptr(v), _ptr(pressure), _ptr(ws), nbytes, *(surface + [_stream()]))
        if pre is not None:
            if isinstance(pre, Multigrid):
                h = multigrid_hierarchy_liquid(v, fl, bnd, phi, gfc if gf else 1e-4, pre.alpha)
            else:
                h = _hierarchy_for(pre, v, bnd, None, 0, "solve_pressure_liquid", "gf" if gf else "liquid")
            iters = _mg_rows_loop(h, s, nd, lambda k: call("df_pressure_cg_update_mg", _ptr(pressure), _ptr(ws), nbytes, _ptr(fl), nd,
                                                           *(s.status4 + [bnd, k, _stream()])))
        else:
            iters = _cg_loop(
                lambda k: call("df_pressure_cg_direction" + sfx + twin[1], _ptr(ws), nbytes, _ptr(fl), *(dims + [bnd, k, s.acc, s.max_iter, _stream()])),
                lambda k: call("df_pressure_cg_update" + sfx + twin[0], _ptr(pressure), _ptr(ws), nbytes, _ptr(fl), *(dims + [bnd, k, _stream()])), s)
        call("df_pressure_correct" + sfx + twin[1], _ptr(v), _ptr(pressure), _ptr(out), *(surface + [_stream()]))
        return out, pressure, iters


# ---- implicit velocity diffusion: cgSolveDiffusion of the viscous liquid scene (scene/liquid3_vis.py:277-281), the definition of
#      include/deepfluids_hip.h ----
def diffusion_alpha(viscosity, dt, resolution_x):
    """The script's ``alphaV = visc * s.timestep * float(resolution_x * resolution_x)`` (scene/liquid3_vis.py:277): the diffusion number
    ``viscosity * dt / dx^2`` with ``dx = 1 / resolution_x`` -- x, not the largest extent."""
    return viscosity * dt * resolution_x ** 2


def default_diffusion_max_iter(shape):
    """mantaflow's ``cgMaxIterFac=1.0`` of cgSolveDiffusion: ``int(max(extent))``, times 4 in 2-D."""
    return int(max(shape)) * (1 if len(shape) == 3 else 4)


def diffusion_workspace(vel):
    """The scratch ``diffuse_velocity`` needs for ``vel`` [B,(Z,)Y,X,D] (the pressure solve's arrays for B*D entries and the planar
    solution): a float32 GPU tensor, reusable across calls of the same shape."""
    v, nd = _smoke_vel(vel, "diffusion_workspace")
    nbytes = query("df_diffuse_workspace_bytes", *([int(x) for x in _pressure_dims(v, nd)[1]] + [nd]))
    if nbytes < 0:
        raise ValueError("diffusion_workspace: unsupported extents %s" % (tuple(v.shape),))
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=v.device)


def _diffusion_alpha_arg(alpha, B, who):
    """[B] float32 on the host: a number for every entry or B of them, finite and >= 0"""
    a = np.asarray(alpha, dtype=np.float64)
    if a.ndim == 0:
        a = np.full((B,), float(a))
    if a.shape != (B,):
        raise ValueError("%s: alpha must be a number or %d numbers, got shape %s" % (who, B, a.shape))
    if not (np.isfinite(a).all() and (a >= 0).all()):
        raise ValueError("%s: alpha must be finite and >= 0, got %r" % (who, alpha))
    a32 = a.astype(np.float32)
    if not np.isfinite(a32).all():
        raise ValueError("%s: alpha must be finite in float32, got %r" % (who, alpha))
    return a32


def diffuse_velocity(vel, alpha, bnd=1, accuracy=1e-4, max_iter=None, check_every=None, out=None, workspace=None, preconditioner=None):
    """mantaflow's ``cgSolveDiffusion(flags, vel, alpha)`` as include/deepfluids_hip.h restates it: every component of ``vel``
    [B,(Z,)Y,X,D] is diffused implicitly, ``(I - alpha * Laplacian) x = u`` on the cells interior by index with the ``bnd`` band as
    Dirichlet data (copied through bit for bit), by plain conjugate gradients from ``x = u``.  ``alpha``: a number or B numbers on the
    host (``diffusion_alpha``), finite and >= 0.  Every (entry, component) pair is its own system and stops on its own at
    ``max|r| <= accuracy`` or after ``max_iter`` iterations (default ``default_diffusion_max_iter``); the host reads one word every
    ``check_every`` iterations, as in ``solve_pressure``.  ``alpha = 0`` returns the input's bits.  No preconditioner, no obstacles.
    Returns ``(vel_out, iterations)``, ``iterations`` int32 [B, D].  ``out`` may be ``vel``.
    ``preconditioner``: an ``ops.Multigrid`` (the hierarchy is built here) or a hierarchy of ``multigrid_hierarchy_diffusion`` built for
    the SAME ``alpha`` (not checked beyond system, geometry and device): multigrid-preconditioned conjugate gradients on the same matrix
    (include/deepfluids_hip_liquid_mg.h), the same stop, ``check_every`` then defaults to 4.  It pays for large ``alpha`` only: a plain
    solve of a few iterations is cheaper than the cycles (profiles/liquid_mg.md).  ``"mg"`` is the smoke calls' and is refused; with
    ``None`` nothing of it is allocated or launched."""
    pre = _liquid_preconditioner_arg(preconditioner, "diffuse_velocity")
    with torch.no_grad():
        if not isinstance(vel, torch.Tensor) or vel.dtype != torch.float32 or not vel.is_cuda or not vel.is_contiguous():
            raise ValueError("diffuse_velocity: vel must be a contiguous float32 GPU tensor [B,(Z,)Y,X,D]")
        v, nd = _smoke_vel(vel, "diffuse_velocity")
        bnd = _liquid_bnd(bnd, "diffuse_velocity")
        a32 = _diffusion_alpha_arg(alpha, v.shape[0], "diffuse_velocity")
        if pre is not None and check_every is None:
            check_every = DEFAULT_MG_CHECK_EVERY
        s = _solve_begin("diffuse_velocity", v, nd, accuracy, max_iter, check_every, workspace if workspace is not None else diffusion_workspace(v),
                         diffusion=True)
        out = _smoke_out(out, v, "diffuse_velocity")
        need = query("df_diffuse_workspace_bytes", *([int(x) for x in _pressure_dims(v, nd)[1]] + [nd]))
        if need < 0 or s.nbytes < need:
            raise ValueError("diffuse_velocity: unsupported extents %s or a workspace of %d bytes where %d are needed (diffusion_workspace)"
                             % (tuple(v.shape), s.nbytes, need))
        al = torch.from_numpy(a32).to(v.device)
        if isinstance(pre, Multigrid):
            pre = multigrid_hierarchy_diffusion(v, al, bnd, pre.alpha)
        elif pre is not None:
            pre = _hierarchy_for(pre, v, bnd, None, 0, "diffuse_velocity", "diffusion", v.shape[0] * nd)
        return _diffuse(v, al, out, bnd, s, pre)


def _diffuse(v, al, out, bnd, s, h=None):
    """the launches of ``diffuse_velocity``; ``al`` [B] float32 on the device, ``s`` the ``_solve_begin`` of a diffusion, ``h`` the
    diffusion hierarchy built for ``al`` (None: the plain solve)"""
    nd, dims, ws, nbytes = v.dim() - 2, list(v.shape[:-1]), s.ws, s.nbytes
    call("df_diffuse_init%dd" % nd, _ptr(v), _ptr(al), _ptr(ws), nbytes, *(dims + [bnd, _stream()]))
    if h is not None:
        iters = _mg_rows_loop(h, s, nd, lambda k: call("df_diffuse_cg_update_mg", _ptr(ws), nbytes, nd, dims[0], *(s.status4[1:] + [bnd, k, _stream()])))
    else:
        iters = _cg_loop(lambda k: call("df_diffuse_cg_direction%dd" % nd, _ptr(al), _ptr(ws), nbytes, *(dims + [bnd, k, s.acc, s.max_iter, _stream()])),
                         lambda k: call("df_diffuse_cg_update%dd" % nd, _ptr(ws), nbytes, *(dims + [bnd, k, _stream()])), s)
    call("df_diffuse_finish%dd" % nd, _ptr(ws), nbytes, _ptr(out), *(dims + [bnd, _stream()]))
    return out, iters.reshape(dims[0], nd)


def flip_update(pos, pvel, vel, vel_old, flip_ratio=DEFAULT_FLIP_RATIO, out=None, entry_start=None):
    """mantaflow's ``flipVelocityUpdate``: with ``u(.)`` the MAC sample of ``advect_particles``, ``un = u(vel, p)``,
    ``d = un - u(vel_old, p)``, ``pvel = flip_ratio * (pvel + d) + (1 - flip_ratio) * un``.  ``out`` may be ``pvel``.
    ``entry_start`` [B+1] int32: ``pos``, ``pvel`` are a ragged batch [P,D]; unused rows are neither read nor written."""
    with torch.no_grad():
        if entry_start is not None:
            p, es = _ragged_arg(pos, entry_start, "flip_update")
            if not isinstance(pvel, torch.Tensor) or tuple(pvel.shape) != tuple(pos.shape):
                raise ValueError("flip_update: velocities %s for positions %s" % (tuple(getattr(pvel, "shape", ())), tuple(pos.shape)))
            u = _prep(pvel.detach(), "pvel").view(p.shape)
        else:
            p = _particle_pos(pos, "flip_update")
            u = _particle_pos(pvel, "flip_update")
        B, N, nd = p.shape
        if tuple(u.shape) != tuple(p.shape):
            raise ValueError("flip_update: velocities %s for positions %s" % (tuple(u.shape), tuple(p.shape)))
        v = _liquid_vel(vel, B, nd, "flip_update")
        vo = _liquid_vel(vel_old, B, nd, "flip_update")
        if tuple(vo.shape) != tuple(v.shape):
            raise ValueError("flip_update: vel_old %s for vel %s" % (tuple(vo.shape), tuple(v.shape)))
        if not 0.0 <= flip_ratio <= 1.0:
            raise ValueError("flip_update: flip_ratio must lie in [0, 1], got %r" % (flip_ratio,))
        if out is None:
            out = torch.empty_like(pvel if entry_start is not None else u)
        elif tuple(out.shape) != tuple(pvel.shape if entry_start is not None else u.shape) or out.dtype != torch.float32 or not out.is_cuda \
                or not out.is_contiguous():
            raise ValueError("flip_update: out must be a contiguous float32 GPU tensor of the velocities' shape")
        if entry_start is not None:
            call("df_flip_update%dd_ragged" % nd, _ptr(p), _ptr(u), _ptr(out), _ptr(v), _ptr(vo), _ptr(es), B, N,
                 *(list(v.shape[1:-1]) + [float(flip_ratio), _stream()]))
            return out
        call("df_flip_update%dd" % nd, _ptr(p), _ptr(u), _ptr(out), _ptr(v), _ptr(vo), B, N, *(list(v.shape[1:-1]) + [float(flip_ratio), _stream()]))
        return out


def sample_velocity(vel, pos, entry_start=None):
    """``u(vel, p)`` at the particles (mantaflow's ``mapGridToPartsVec3`` of a MAC grid): the FLIP update with ratio 0 from zero particle
    velocities, which is ``0 * (0 + 0) + 1 * u`` -- the sample's own bits.  ``entry_start``: ``pos`` is a ragged batch [P,D]; unused
    rows come back 0."""
    with torch.no_grad():
        if entry_start is not None:
            _ragged_arg(pos, entry_start, "sample_velocity")
            return flip_update(pos, torch.zeros_like(pos), vel, vel, flip_ratio=0.0, out=torch.zeros_like(pos), entry_start=entry_start)
        p = _particle_pos(pos, "sample_velocity")
        return flip_update(p, torch.zeros_like(p), vel, vel, flip_ratio=0.0)


def extrapolate_levelset(phi, distance=4, inside=True, out=None):
    """mantaflow's ``extrapolateLsSimple(phi, distance, inside)``, restated from memory; the definition that is tested is the one in
    include/deepfluids_hip.h (tests/liquid_resample_ref.py), NOT mantaflow.  Over the cells off the outermost layer of ``phi``
    [B,(Z,)Y,X]: mark 1 where phi > 0 (``inside``) or phi < 0, mark 2 on unmarked cells with a face neighbour marked 1, and for d = 2 ..
    ``distance`` an unmarked cell with n > 0 face neighbours marked d takes mark d + 1 and phi = (their sum, x-, x+, y-, y+[, z-, z+]) / n
    - 1 (``inside``) or + 1.  Cells never reached and the outermost layer keep their bits; ``distance <= 1`` returns the input's bits.
    One launch for the marks and one per layer, in place on the result.  ``out`` may be ``phi``.  With ``inside`` this makes phi
    decrease with depth below the surface, which ``resample_particles`` relies on."""
    with torch.no_grad():
        distance = int(distance)
        if not 0 <= distance <= 254:
            raise ValueError("extrapolate_levelset: distance must be in 0..254, got %r" % (distance,))
        if not isinstance(phi, torch.Tensor) or phi.dim() not in (3, 4):
            raise ValueError("extrapolate_levelset expects phi [B,(Z,)Y,X], got %s" % (tuple(phi.shape) if isinstance(phi, torch.Tensor) else type(phi),))
        ph = _prep(phi.detach(), "phi")
        nd = ph.dim() - 1
        if out is None:
            out = ph.clone()
        else:
            if tuple(out.shape) != tuple(ph.shape) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
                raise ValueError("extrapolate_levelset: out must be a contiguous float32 GPU tensor of phi's shape")
            if out.data_ptr() != ph.data_ptr():
                out.copy_(ph)
        if distance <= 1:
            return out
        dims = list(ph.shape)
        mark = _u8(tuple(ph.shape), ph)
        call("df_levelset_extrapolate_marks%dd" % nd, _ptr(out), _ptr(mark), *(dims + [1 if inside else 0, _stream()]))
        for d in range(2, distance + 1):
            call("df_levelset_extrapolate_layer%dd" % nd, _ptr(out), _ptr(mark), *(dims + [1 if inside else 0, d, _stream()]))
        return out


_Resampled = collections.namedtuple("_Resampled", "pos pvel entry_start cell_start keep kept seeds")


def _resample_launch(sp, su, cell_start, ph, fl, v, bnd, radius_factor, rs):
    """the launches of ``resample_particles`` on checked arguments, ``rs`` a ``Resample`` (its counts, seed and step); the wanted total is
    the result's ``cell_start[-1]``, still on the device"""
    shape = tuple(v.shape[1:-1])
    nd, B = len(shape), v.shape[0]
    N = sp.shape[0] // B
    ncell = int(np.prod(shape))
    keep = torch.zeros((B * N,), dtype=torch.uint8, device=v.device)
    counts = torch.empty((2, B * ncell), dtype=torch.int32, device=v.device)
    kept, seeds = counts[0], counts[1]
    call("df_resample_count%dd" % nd, _ptr(sp), _ptr(cell_start), _ptr(ph), _ptr(fl), _ptr(keep), _ptr(kept), _ptr(seeds), B, N,
         *(list(shape) + [bnd, rs.min_particles, rs.max_particles, float(radius_factor), _stream()]))
    new_start = torch.zeros((B * ncell + 1,), dtype=torch.int32, device=v.device)
    torch.cumsum(kept + seeds, 0, dtype=torch.int32, out=new_start[1:])
    pos_out, pvel_out = torch.empty_like(sp), torch.empty_like(su)
    call("df_resample_scatter%dd" % nd, _ptr(sp), _ptr(su), _ptr(cell_start), _ptr(keep), _ptr(seeds), _ptr(new_start), _ptr(v), _ptr(pos_out),
         _ptr(pvel_out), B, N, *(list(shape) + [rs.min_particles, rs.seed & 0xFFFFFFFF, rs.step & 0xFFFFFFFF, _stream()]))
    return _Resampled(pos_out, pvel_out, new_start[::ncell].contiguous(), new_start, keep, kept, seeds)


def _resample_counts_arg(min_particles, max_particles, who):
    min_particles = int(min_particles)
    max_particles = 2 * min_particles if max_particles is None else int(max_particles)
    if not 1 <= min_particles <= 4096:
        raise ValueError("%s: min_particles must be in 1..4096, got %r" % (who, min_particles))
    if max_particles < min_particles or max_particles > 8192:
        raise ValueError("%s: max_particles must be in min_particles..8192 (max < min is refused), got %r for min_particles %r" %
                         (who, max_particles, min_particles))
    return min_particles, max_particles


def resample_particles(spos, spvel, cell_start, entry_start, phi, flags, vel, min_particles, max_particles=None, radius_factor=1.0, seed=123,
                       step=0, bnd=1, details=False):
    """mantaflow's ``adjustNumber(pp, vel, flags, minParticles, maxParticles, phi, radiusFactor)`` after ``pVel.setSource(vel,
    isMAC=True)``, restated from memory; the definition that is tested is the one in include/deepfluids_hip.h
    (tests/liquid_resample_ref.py), NOT mantaflow.  On a SORTED ragged batch (``particle_cells(.., entry_start=)``; ``spvel`` permuted
    alike) with ``phi`` the extrapolated level set (``extrapolate_levelset``), ``flags`` of ``liquid_flags`` and the MAC velocity ``vel``:
    a particle is dropped where the interpolated phi is > 0, or where its cell already kept more than ``max_particles`` (default ``2 *
    min_particles``) and it is not at the surface (phi <= -2R, R the level sets' radius); a liquid cell below the surface with fewer
    than ``min_particles`` kept is filled up with seeds at hashed positions (``seed``, ``step``) strictly inside the cell, carrying
    ``u(vel, p)``.  Returns ``(pos [P,D], pvel [P,D], entry_start [B+1], cell_start [B*ncell+1])``, again sorted by cell; rows from
    ``entry_start[B]`` on are unused.  Raises when the result needs more than P rows, naming the capacity needed (nothing is written
    past row P - 1; this reads one word back from the device).  ``details``: also ``(keep [P] uint8, kept, seeds [B*ncell] int32)``."""
    with torch.no_grad():
        min_particles, max_particles = _resample_counts_arg(min_particles, max_particles, "resample_particles")
        if not 0.0 <= radius_factor <= 1024.0:
            raise ValueError("resample_particles: radius_factor must lie in [0, 1024], got %r" % (radius_factor,))
        bnd = _liquid_bnd(bnd, "resample_particles")
        p, es = _ragged_arg(spos, entry_start, "resample_particles")
        if not isinstance(spvel, torch.Tensor) or tuple(spvel.shape) != tuple(spos.shape):
            raise ValueError("resample_particles: velocities %s for positions %s" % (tuple(getattr(spvel, "shape", ())), tuple(spos.shape)))
        u = _prep(spvel.detach(), "spvel")
        B, N, nd = p.shape
        v = _liquid_vel(vel, B, nd, "resample_particles")
        shape = tuple(v.shape[1:-1])
        ph = _gf_phi_arg(phi, v, "resample_particles")
        fl = _liquid_flags_arg(flags, v, "resample_particles")
        ncell = int(np.prod(shape))
        if cell_start.dtype != torch.int32 or not cell_start.is_cuda or not cell_start.is_contiguous() or cell_start.numel() != B * ncell + 1:
            raise ValueError("resample_particles: cell_start must be the int32 GPU tensor [B*ncell + 1] of particle_cells")
        new = _resample_launch(p.view(-1, nd), u, cell_start, ph, fl, v, bnd, radius_factor, Resample(min_particles, max_particles, seed, step=step))
        _resample_check(new.cell_start, B * N, B, "resample_particles")
        if details:
            return new.pos, new.pvel, new.entry_start, new.cell_start, (new.keep, new.kept, new.seeds)
        return new.pos, new.pvel, new.entry_start, new.cell_start


def _resample_check(new_start, P, B, who):
    """refuse a resampled state that did not fit: ``new_start[-1]`` is the total the scan wanted"""
    total = _read_word(new_start[-1:])
    if total > P:
        raise _lib.DeepFluidsHipError("%s: the resampled batch holds %d particles but the storage has P = %d rows; it needs a capacity of at "
                                      "least %d (a multiple of B = %d)" % (who, total, P, -(-total // B) * B, B))


class Resample(object):
    """The settings of ``resample=`` on ``liquid_step`` / ``simulate_liquid``: ``min_particles`` per deep liquid cell, ``max_particles``
    (None: ``2 * min_particles``, as the scripts call adjustNumber), the ``seed`` of the seed positions' hash, and the ``capacity`` P of the
    ragged storage (None: twice the initial live total, rounded up to a multiple of B).  ``step`` is the counter fed to the hash; every
    step taken with this object advances it by one, so chained ``liquid_step`` calls and ``simulate_liquid`` seed alike."""

    def __init__(self, min_particles, max_particles=None, seed=123, capacity=None, step=0):
        self.min_particles, self.max_particles = _resample_counts_arg(min_particles, max_particles, "Resample")
        self.seed, self.step = int(seed), int(step)
        if capacity is not None and (int(capacity) != capacity or capacity < 1):
            raise ValueError("Resample: capacity must be a positive integer, got %r" % (capacity,))
        self.capacity = None if capacity is None else int(capacity)


class _LiquidSettings(object):
    """What a liquid step needs besides its state, built once per ``liquid_step`` call or ``simulate_liquid`` sequence (``who``).  The
    constructor keeps the call's scalars and refuses what can be refused before any tensor is touched; ``prepare(vel)`` then allocates
    what the options need and nothing else: the device ``alpha`` and the diffusion workspace (``viscosity_alpha``), the two phi buffers
    (``ghost_fluid`` or ``resample``), the pressure workspace (ghost-fluid-sized only with ``ghost_fluid``).  ``rs`` is the ``Resample``."""

    def __init__(self, who, dt, force, bnd, accuracy, max_iter, check_every, flip_ratio, open_bound, viscosity_alpha, ghost_fluid, radius_factor,
                 gf_clamp, resample, entry_start, preconditioner=None):
        self.pre = _liquid_preconditioner_arg(preconditioner, who)
        if isinstance(self.pre, MultigridHierarchy):
            raise ValueError("%s: preconditioner must be None or an ops.Multigrid(...): the liquid moves, so the step builds its hierarchies itself, got "
                             "preconditioner=%r" % (who, preconditioner))
        if open_bound:
            raise NotImplementedError("%s: open sides (resetOutflow) are not implemented for the liquid solver" % who)
        if ghost_fluid:
            _gf_clamp_arg(gf_clamp, who)
        if resample is not None and not isinstance(resample, Resample):
            raise ValueError("%s: resample must be None or an ops.Resample, got %r" % (who, type(resample)))
        if resample is None and entry_start is not None:
            raise ValueError("%s: entry_start (a ragged state) needs resample=" % who)
        if (resample is not None or ghost_fluid) and not 0.0 <= radius_factor <= 1024.0:
            raise ValueError("%s: radius_factor must lie in [0, 1024], got %r" % (who, radius_factor))
        self.who, self.rs, self.dt, self.force, self.bnd = who, resample, dt, force, bnd
        self.accuracy, self.max_iter, self.check_every, self.flip_ratio = accuracy, max_iter, check_every, flip_ratio
        self.viscosity_alpha, self.ghost_fluid, self.radius_factor, self.gf_clamp = viscosity_alpha, bool(ghost_fluid), radius_factor, gf_clamp

    def prepare(self, v):
        self.bnd = _liquid_bnd(self.bnd, self.who)
        if self.force is None:
            self.force = default_gravity_force(v.shape[1:-1], self.dt)
        self.phi = self.phi_tmp = self.alpha = self.dws = None
        if self.ghost_fluid or self.rs is not None:
            self.phi = _empty(tuple(v.shape[:-1]), v)
            self.phi_tmp = torch.empty_like(self.phi)
        self.pws = pressure_workspace(v, self.ghost_fluid)
        if self.viscosity_alpha is not None:
            self.alpha = torch.from_numpy(_diffusion_alpha_arg(self.viscosity_alpha, v.shape[0], self.who)).to(v.device)
            self.dws = diffusion_workspace(v)
        # the hierarchy blocks of preconditioner=Multigrid(...): the projection's is allocated here and rebuilt from every step's flags
        # (and phi); the diffusion's matrix does not change, so it is built here once.  None: nothing is allocated.
        self.hp = self.hd = None
        if self.pre is not None:
            self.hp = _hierarchy_block(self.who, v.dim() - 2, v.shape[0], tuple(v.shape[1:-1]), v.device, None, self.bnd, self.pre.alpha,
                                       "gf" if self.ghost_fluid else "liquid")
            if self.alpha is not None and self.pre.diffusion:
                self.hd = multigrid_hierarchy_diffusion(v, self.alpha, self.bnd, self.pre.alpha)

    def frame(self, r, counts=False):
        """the public tuple of a ``_LiquidResult``: ``(pos, pvel, vel[, iterations[, diffusion_iterations]][, entry_start])``"""
        out = (r.pos, r.pvel, r.vel)
        if counts:
            out += (r.iters,) if r.diters is None else (r.iters, r.diters)
        return out if self.rs is None else out + (r.entry_start,)


def _liquid_state(pos, pvel, vel, entry_start, cfg):
    """the checked state ``(pos, pvel, vel, entry_start)`` a step runs on: dense [B,N,D] with ``entry_start`` None, or, with ``resample``,
    ragged [P,D] -- a dense input is packed (entry b in rows b*N ..), a ragged one is moved into storage of ``capacity`` rows if it has
    another size"""
    who, rs = cfg.who, cfg.rs
    if entry_start is None:
        p = _particle_pos(pos, who)
        u = _particle_pos(pvel, who)
        if tuple(u.shape) != tuple(p.shape):
            raise ValueError("%s: particle velocities %s for positions %s" % (who, tuple(u.shape), tuple(p.shape)))
        B, N, nd = p.shape
        v = _liquid_vel(vel, B, nd, who)
        if rs is None:
            return p, u, v, None
        live = B * N
        es = torch.arange(B + 1, dtype=torch.int32, device=p.device) * N
        p, u = p.reshape(-1, nd), u.reshape(-1, nd)
    else:
        p3, es = _ragged_arg(pos, entry_start, who)
        if not isinstance(pvel, torch.Tensor) or tuple(pvel.shape) != tuple(pos.shape):
            raise ValueError("%s: particle velocities %s for positions %s" % (who, tuple(getattr(pvel, "shape", ())), tuple(pos.shape)))
        B, nd = p3.shape[0], p3.shape[-1]
        p, u = p3.view(-1, nd), _prep(pvel.detach(), "pvel")
        v = _liquid_vel(vel, B, nd, who)
        live = None
    P = rs.capacity
    if P is None:
        if live is None:
            P = p.shape[0]                                   # a ragged state already has its storage
        else:
            P = -(-2 * live // B) * B
    if P % B:
        raise ValueError("%s: the capacity %d is not a multiple of B = %d" % (who, P, B))
    if P != p.shape[0]:
        if live is None:
            live = _read_word(es[-1:])
        if P < live:
            raise ValueError("%s: the capacity %d does not hold the %d particles" % (who, P, live))
        np_, nu = torch.zeros((P, nd), dtype=torch.float32, device=p.device), torch.zeros((P, nd), dtype=torch.float32, device=p.device)
        np_[:live], nu[:live] = p[:live], u[:live]
        p, u = np_, nu
    return p, u, v, es


_LiquidResult = collections.namedtuple("_LiquidResult", "pos pvel vel iters diters entry_start cell_start")


def _liquid_step(p, u, v, es, cfg):
    """One step on the dense state ``p``, ``u`` [B,N,D] (``es`` None: the dense kernels) or on the ragged one [P,D] with its
    ``entry_start`` ``es`` (``cfg.rs`` set: the script's extrapolateLsSimple and adjustNumber run too), ``cfg`` a prepared
    ``_LiquidSettings``.  Fields of the result that do not apply are None: ``diters`` [B, D] without ``viscosity_alpha``; ``entry_start``
    and ``cell_start`` without ``resample`` -- the total the resampling wanted is ``cell_start[-1]``, still on the device: the caller
    checks it."""
    nd, bnd, rs = p.shape[-1], cfg.bnd, cfg.rs
    shape = tuple(v.shape[1:-1])
    B = v.shape[0]
    N = p.numel() // (B * nd)
    moved = advect_particles(p, v, cfg.dt, bnd=bnd, entry_start=es)
    spos, cell_start, order = particle_cells(moved, shape, entry_start=es)
    su = torch.empty_like(u)
    call("df_particles_gather", _ptr(u), _ptr(order), _ptr(su), B * N, nd, _stream())
    vel, weight, known = particles_to_grid(spos.view(B, N, nd), su.view(B, N, nd), cell_start, shape)
    vel_old = vel                                            # extrapolate_mac leaves its input untouched
    vel, _ = extrapolate_mac(vel, known, 2, bnd=bnd)
    flags, touch = liquid_flags(cell_start, shape, B, N, bnd=bnd)
    phi = None
    if cfg.phi is not None:
        # averagedParticleLevelset(.., radius_factor, 1, 1) and phi.setBound(1, bWidth), from the sort above: no second sort; computed
        # whenever the step resamples, and then extrapolated before the solve sees it
        phi = _levelset_averaged(spos, cell_start, cfg.phi, cfg.phi_tmp, cfg.radius_factor, 1, 1, 1.0, bnd)
        if rs is not None:
            extrapolate_levelset(phi, 4, True, out=phi)
    diters = None
    if cfg.alpha is not None:
        # the viscous step of scene/liquid3_vis.py:256-296: setWallBcs as a zero-force pass (+ 0.0 leaves a value's bits but for -0),
        # then cgSolveDiffusion: the step's accuracy, the iteration cap of cgSolveDiffusion's own default (max_iter is the pressure solve's)
        liquid_forces(vel, flags, (0.0,) * nd, bnd=bnd, out=vel)
        dce = DEFAULT_MG_CHECK_EVERY if cfg.hd is not None and cfg.check_every is None else cfg.check_every
        _, diters = _diffuse(vel, cfg.alpha, vel, bnd, _solve_begin(cfg.who, vel, nd, cfg.accuracy, None, dce, cfg.dws, diffusion=True), cfg.hd)
    liquid_forces(vel, flags, cfg.force, bnd=bnd, out=vel)
    surface = dict(phi=phi, gf_clamp=cfg.gf_clamp) if cfg.ghost_fluid else dict()
    if cfg.hp is not None:
        multigrid_hierarchy_liquid(vel, flags, bnd, alpha=cfg.pre.alpha, out=cfg.hp, **surface)       # this step's liquid, in place
    _, _, iters = solve_pressure_liquid(vel, flags, bnd=bnd, accuracy=cfg.accuracy, max_iter=cfg.max_iter, check_every=cfg.check_every, out=vel,
                                        workspace=cfg.pws, preconditioner=cfg.hp, **surface)
    if rs is not None:
        # pVel.setSource(vel, isMAC=True) + adjustNumber against the projected velocity, then extrapolateMACSimple and the FLIP update on
        # old and new particles alike
        new = _resample_launch(spos, su, cell_start, phi, flags, vel, bnd, cfg.radius_factor, rs)
        spos, su, es, cell_start = new.pos, new.pvel, new.entry_start, new.cell_start
    vel, _ = extrapolate_mac(vel, touch, 4, bnd=bnd)
    flip_update(spos, su, vel, vel_old, flip_ratio=cfg.flip_ratio, out=su, entry_start=es)
    if rs is None:
        return _LiquidResult(spos, su, vel, iters, diters, None, None)
    rs.step += 1
    return _LiquidResult(spos, su, vel, iters, diters, es, cell_start)


def liquid_step(pos, pvel, vel, dt, force=None, bnd=1, accuracy=1e-4, max_iter=None, check_every=None, flip_ratio=DEFAULT_FLIP_RATIO,
                open_bound=False, viscosity_alpha=None, ghost_fluid=False, radius_factor=1.0, gf_clamp=1e-4, resample=None, entry_start=None,
                preconditioner=None):
    """One frame of the reference's liquid scenes (scene/liquid_pos_size.py:254-295) on particles ``pos``, ``pvel`` [B,N,D] and the MAC
    velocity ``vel`` [B,(Z,)Y,X,D], in the script's order: trace the particles through ``vel`` (RK4), sort them by cell, map their
    velocities to the grid, extrapolate 2 layers from the faces that received weight, mark the liquid cells, add gravity (``force``,
    cells per step; default ``default_gravity_force``, restated from memory of mantaflow's addGravity) and zero the wall faces, project
    with p = 0 in the air cells, extrapolate 4 layers from the faces of liquid cells, update the particle velocities (FLIP,
    ``flip_ratio``).  Returns ``(pos, pvel, vel, iterations)``: the particles come back SORTED by cell, so the step permutes them
    (``pos`` and ``pvel`` alike); ``vel`` is the frame the script saves.  Left out, as named in include/deepfluids_hip.h:
    adjustNumber and extrapolateLsSimple unless ``resample`` is set, open sides (``open_bound=True`` is refused), obstacles, MIC(0).
    ``ghost_fluid=True``: right after the liquid cells are marked, the averaged level set of the step's own sorted particles
    (``particle_levelset_averaged`` with ``radius_factor``, smooth 1, smooth_neg 1, the ``bnd`` band set to 1.0 -- the script's order) is
    computed and handed to the solve (``solve_pressure_liquid(phi=..., gf_clamp=...)``): the velocity is projected against a surface
    between the cell centres.  With ``False`` p = 0 sits at the air cell centres and nothing of this is launched.
    ``viscosity_alpha`` (a number or B numbers, ``diffusion_alpha``): the viscous step of scene/liquid3_vis.py:256-296 -- after the
    liquid cells are marked the wall faces are zeroed (setWallBcs, a zero-force ``liquid_forces`` pass) and the velocity is diffused
    (``diffuse_velocity`` at the step's ``accuracy`` and its own default iteration cap), then gravity and the rest as above; the
    result is then ``(pos, pvel, vel, iterations, diffusion_iterations [B, D])``.  With ``None`` nothing of this is launched.
    ``resample`` (an ``ops.Resample``): the step also runs the script's ``extrapolateLsSimple(phi, 4, inside=True)`` and ``pVel.setSource``
    + ``adjustNumber``.  The state is then ragged: a dense [B,N,D] input is packed into storage of ``resample.capacity`` rows, or pass
    ``pos``, ``pvel`` [P,D] with ``entry_start`` [B+1] as a step returned them.  Order: flags; the averaged level set (computed whenever
    ``resample`` is set, shared with ``ghost_fluid``, which then sees the EXTRAPOLATED phi, as in the script); ``extrapolate_levelset``;
    forces and the solve; ``resample_particles`` against the projected velocity (``resample.step`` feeds the hash and advances);
    the 4-layer extrapolation; the FLIP update on old and new particles alike.  The result is ``(pos [P,D], pvel [P,D], vel,
    iterations[, diffusion_iterations], entry_start)``; a state that does not fit the capacity raises before the step returns.  With
    ``None`` nothing of this is launched and every result keeps its bits.
    ``preconditioner=ops.Multigrid(...)``: the projection -- free surface or ghost fluid, according to ``ghost_fluid`` -- is
    multigrid-preconditioned (``solve_pressure_liquid``; the hierarchy is rebuilt from the step's flags and phi), and with
    ``viscosity_alpha`` and ``Multigrid.diffusion`` the diffusion is too (``diffuse_velocity``).  Nothing else of the step changes, so it
    combines with ``resample`` and ``entry_start`` as it is.  The string ``"mg"`` is refused; with ``None`` nothing is allocated or
    launched and every result keeps its bits.  The projections of the two arms agree to ``accuracy``.  The diffusions do NOT wherever
    the plain solve stops at its iteration cap (``default_diffusion_max_iter``: ``max(extent)`` in 3-D) short of ``accuracy``, as it
    does at the large ``viscosity_alpha`` of the 96x72x48 scene: the preconditioned solve converges under the same cap, so the viscous
    frames then differ from the plain arm's by the plain solve's truncation, far more than ``accuracy`` (profiles/liquid_mg.md);
    ``Multigrid(diffusion=False)`` keeps the plain diffusion."""
    cfg = _LiquidSettings("liquid_step", dt, force, bnd, accuracy, max_iter, check_every, flip_ratio, open_bound, viscosity_alpha, ghost_fluid,
                          radius_factor, gf_clamp, resample, entry_start, preconditioner)
    with torch.no_grad():
        p, u, v, es = _liquid_state(pos, pvel, vel, entry_start, cfg)
        cfg.prepare(v)
        r = _liquid_step(p, u, v, es, cfg)
        if cfg.rs is not None:
            _resample_check(r.cell_start, p.shape[0], v.shape[0], "liquid_step")
        return cfg.frame(r, counts=True)


def _liquid_frames(pos0, pvel0, vel0, entry_start, steps, keep_every, stats, cfg):
    """the kept steps' ``_LiquidResult`` of ``steps`` chained steps"""
    p, u, v, es = _liquid_state(pos0, pvel0, vel0, entry_start, cfg)
    cfg.prepare(v)
    for t in range(int(steps)):
        r = _liquid_step(p, u, v, es, cfg)
        p, u, v, es = r.pos, r.pvel, r.vel, r.entry_start
        if stats is not None:
            stats.append(r.iters)
        if cfg.rs is not None and (t % keep_every == 0 or t == int(steps) - 1):
            # a state that did not fit is refused at every kept frame and after the last step; between them a step that follows an
            # overflow reads clamped ranges only, and its result is never handed out
            _resample_check(r.cell_start, p.shape[0], v.shape[0], cfg.who)
        if t % keep_every == 0:
            yield r


def simulate_liquid(pos0, pvel0, vel0, steps, dt=0.5, force=None, bnd=1, accuracy=1e-4, max_iter=None, check_every=None,
                    flip_ratio=DEFAULT_FLIP_RATIO, stack=True, stats=None, open_bound=False, viscosity_alpha=None, keep_every=1,
                    ghost_fluid=False, radius_factor=1.0, gf_clamp=1e-4, resample=None, entry_start=None, preconditioner=None):
    """``steps`` chained ``liquid_step`` frames from ``(pos0, pvel0, vel0)`` (left untouched).  With ``stack`` returns
    ``(pos, pvel, vels)``, ``vels`` [steps,B,(Z,)Y,X,D] the velocity after each step; without it a generator of ``(pos, pvel, vel)`` per
    step.  ``stats``: a list that receives the iteration counts [B] of every step's solve.  ``viscosity_alpha``: as in ``liquid_step``.
    ``keep_every=k``: only the steps 0, k, 2k, ... (0-based) are yielded or stacked (``vels`` [ceil(steps/k),...]; a scene whose frame
    is ``k`` solver steps) -- every step still runs and reports to ``stats``, and with ``stack`` the returned particles are those after
    the LAST step.  ``ghost_fluid``, ``radius_factor``, ``gf_clamp``: as in ``liquid_step``.  ``resample`` (and ``entry_start`` for a
    ragged start): as in ``liquid_step``; the state is ragged, the result is ``(pos [P,D], pvel [P,D], vels, entry_start)`` or a generator
    of ``(pos, pvel, vel, entry_start)``, and a state that does not fit the capacity raises at the next kept frame at the latest.
    ``preconditioner``: as in ``liquid_step`` -- what is said there about viscous frames and the plain diffusion's iteration cap holds for
    every frame here; the hierarchy blocks are allocated once for the sequence and rebuilt per step."""
    _liquid_preconditioner_arg(preconditioner, "simulate_liquid")
    keep_every = int(keep_every)
    if keep_every < 1:
        raise ValueError("simulate_liquid: keep_every must be >= 1, got %r" % (keep_every,))
    cfg = _LiquidSettings("simulate_liquid", dt, force, bnd, accuracy, max_iter, check_every, flip_ratio, open_bound, viscosity_alpha, ghost_fluid,
                          radius_factor, gf_clamp, resample, entry_start, preconditioner)
    with torch.no_grad():
        gen = _liquid_frames(pos0, pvel0, vel0, entry_start, steps, keep_every, stats, cfg)
        if not stack:
            return _no_grad_iter(cfg.frame(r) for r in gen)
        kept = (int(steps) + keep_every - 1) // keep_every
        vels = torch.empty((kept,) + tuple(vel0.shape), dtype=torch.float32, device=vel0.device)
        last = _LiquidResult(pos0, pvel0, vels, None, None, entry_start, None)                            # steps == 0: the inputs
        for t, last in enumerate(gen):
            vels[t].copy_(last.vel)
        return cfg.frame(last._replace(vel=vels))


def liquid_initial_state(shape, phi0, vel_spheres=(), discretization=2, randomness=0.05, seed=123, bnd=1, device="cuda"):
    """The state the liquid scenes start from (scene/liquid_pos_size.py:235-252): particles seeded in ``phi0`` [(Z,)Y,X] < 0
    (``seed_particles``; join bodies with ``np.minimum``), a velocity that is (0, -1[, 0]) on the faces whose centre lies inside one of
    ``vel_spheres`` ((centre xyz, radius) pairs, cell units; ``Sphere.applyToGrid`` on a MAC grid, restated from memory) and 0
    elsewhere, and ``pvel = u(vel, p)``.  Returns ``(pos [1,N,D], pvel [1,N,D], vel [1,(Z,)Y,X,D])`` on ``device``."""
    shape = tuple(int(n) for n in shape)
    nd = len(shape)
    if nd not in (2, 3) or tuple(np.shape(phi0)) != shape:
        raise ValueError("liquid_initial_state expects a shape [(Z,)Y,X] and a level set of that shape, got %s, %s" % (shape, np.shape(phi0)))
    pos = seed_particles(phi0, discretization, randomness, seed, bnd)
    vel = np.zeros(shape + (nd,), np.float32)
    for centre, radius in vel_spheres:
        if len(centre) != nd:
            raise ValueError("liquid_initial_state: a sphere centre of %d coordinates on a %d-D grid" % (len(centre), nd))
        d2 = np.zeros(shape, np.float64)
        for a, c in enumerate(centre):
            d2 = d2 + ((_centres(shape, a) - (0.5 if a == 1 else 0.0)) - float(c)) ** 2       # the y face: (i + .5, j[, k + .5])
        vel[..., 1] = np.where(d2 <= float(radius) ** 2, np.float32(-1.0), vel[..., 1])
    p = torch.from_numpy(pos[None]).to(device)
    v = torch.from_numpy(vel[None]).to(device)
    return p, sample_velocity(v, p), v


# ---- the surface of a 3-D level set as a triangle mesh (what the reference's 3-D liquid scripts get from phi.createMesh + mesh.save,
#      scene/liquid3_vis.py:136-143).  Marching tetrahedra on the Kuhn split of the cubes between cell centres: the definition is this
#      project's own (include/deepfluids_hip.h, "liquid surface meshes"), tested against tests/liquid_mesh_ref.py; no parity with
#      mantaflow's marching-cubes mesh is claimed.  Left out: 2-D contours, smoothMesh / subdivideMesh (smooth phi with
#      ``particle_levelset_averaged`` instead), .bobj.gz, rendering ----
class SurfaceMesh(object):
    """The result of ``extract_surface``: ``vertices`` [V,3] float32 (xyz, grid units, a cell centre at +0.5), ``faces`` [T,3] int32 holding
    vertex rows LOCAL to their batch entry, ``normals`` [V,3] or None, and ``vertex_start``, ``face_start`` [B+1] int32: entry b owns the
    vertex rows ``vertex_start[b] .. vertex_start[b+1] - 1`` and the face rows ``face_start[b] .. face_start[b+1] - 1`` (a ragged batch in
    the ``entry_start`` style).  All on the device of phi."""

    def __init__(self, vertices, faces, normals, vertex_start, face_start):
        self.vertices, self.faces, self.normals = vertices, faces, normals
        self.vertex_start, self.face_start = vertex_start, face_start
        self._starts = None

    @property
    def batch(self):
        return self.vertex_start.numel() - 1

    def entry(self, i):
        """``(vertices [V_i,3], faces [T_i,3], normals [V_i,3] | None)`` of batch entry ``i``, views of the batch's arrays; the first
        call copies the 2 (B + 1) starts to the host."""
        if self._starts is None:
            self._starts = (self.vertex_start.cpu().numpy().astype(np.int64), self.face_start.cpu().numpy().astype(np.int64))
        vs, fs = self._starts
        if not 0 <= int(i) < len(vs) - 1:
            raise IndexError("SurfaceMesh.entry: %r is not one of the %d batch entries" % (i, len(vs) - 1))
        i = int(i)
        v = slice(int(vs[i]), int(vs[i + 1]))
        return self.vertices[v], self.faces[int(fs[i]):int(fs[i + 1])], None if self.normals is None else self.normals[v]


def _mesh_args(phi, bnd, closed, closed_value, capacity):
    """the checks of ``extract_surface`` that need no device: ``(bnd, closed, closed_value, (vertex rows, face rows) | None)``"""
    who = "extract_surface"
    if not isinstance(phi, torch.Tensor):
        raise TypeError("%s: phi must be a torch.Tensor on the MI355X (got %r)" % (who, type(phi)))
    if phi.dim() != 4:
        raise ValueError("%s expects a 3-D level set phi [B,Z,Y,X], got %s (2-D contours are not built)" % (who, tuple(phi.shape)))
    if phi.dtype != torch.float32:
        raise TypeError("%s: phi must be float32, got %s" % (who, phi.dtype))
    if not phi.is_contiguous():
        raise ValueError("%s: phi must be contiguous (strides %s for shape %s)" % (who, tuple(phi.stride()), tuple(phi.shape)))
    B, Z, Y, X = (int(n) for n in phi.shape)
    if B < 1 or min(Z, Y, X) < 2:
        raise ValueError("%s: every extent of phi [B,Z,Y,X] must be >= 2 (and B >= 1), got %s" % (who, tuple(phi.shape)))
    if isinstance(bnd, bool) or int(bnd) != bnd or bnd < 0:
        raise ValueError("%s: bnd must be an integer >= 0, got %r" % (who, bnd))
    bnd, closed = int(bnd), bool(closed)
    if closed and bnd < 1:
        raise ValueError("%s: closed=True needs bnd >= 1 (the capped layer is the outer layer of the box one wider than bnd)" % who)
    if min(Z, Y, X) - 1 - 2 * (bnd - 1 if closed else bnd) < 1:
        raise ValueError("%s: bnd = %d is too wide for a grid %s: the meshed box has no cube" % (who, bnd, (Z, Y, X)))
    closed_value = float(closed_value)
    if closed and not (closed_value > 0.0 and math.isfinite(closed_value)):
        raise ValueError("%s: closed_value must be finite and > 0 (an outside value), got %r" % (who, closed_value))
    if 12 * B * Z * Y * X >= 2 ** 31:
        raise ValueError("%s: %d samples: 12 triangles per sample do not fit an int32 offset" % (who, B * Z * Y * X))
    if capacity is not None:
        cap = (capacity, capacity) if isinstance(capacity, (int, np.integer)) else tuple(capacity)
        if len(cap) != 2 or any(isinstance(c, bool) or int(c) != c or c < 0 or c > (2 ** 31 - 1) // 3 for c in cap):
            raise ValueError("%s: capacity must be a row count >= 0 or a pair (vertex rows, face rows), got %r" % (who, capacity))
        capacity = (int(cap[0]), int(cap[1]))
    return bnd, closed, closed_value, capacity


def _mesh_fit(V, T, capacity, who="extract_surface"):
    """refuse a mesh that does not fit ``capacity = (vertex rows, face rows)``, naming the capacity needed"""
    if capacity is not None and (V > capacity[0] or T > capacity[1]):
        raise _lib.DeepFluidsHipError("%s: the mesh holds %d vertices and %d faces but capacity gives %d vertex rows and %d face rows; it "
                                      "needs capacity=(%d, %d)" % (who, V, T, capacity[0], capacity[1], V, T))


def extract_surface(phi, bnd=0, closed=False, closed_value=0.5, normals=False, capacity=None):
    """The surface phi = 0 of a 3-D level set ``phi`` [B,Z,Y,X] (float32, contiguous, negative inside) as an indexed triangle mesh, one
    per batch entry: a ``SurfaceMesh``.  Marching tetrahedra on the Kuhn split of the cubes between cell centres, as
    include/deepfluids_hip.h defines it -- this project's own definition, not mantaflow's ``phi.createMesh`` (marching cubes); the
    kernels give the bits of tests/liquid_mesh_ref.py's fp32 twin, order included.  A vertex sits on every grid edge (axis, face
    diagonal or cube diagonal, always towards +) whose ends differ in sign, an exact zero counting as outside; triangles are wound with
    their normal out of the liquid.
    ``bnd``: leave out the ``bnd`` outermost samples per side.  ``closed`` (needs ``bnd >= 1``): mesh one layer more and read that outer
    layer as ``max(phi, closed_value)``, which caps a liquid that rests against a wall: every mesh is then a closed surface.
    ``normals``: also the normalised gradient of phi at the vertices.
    Two launches and two scans: count, ``torch.cumsum`` twice, emit.  The host reads the two totals between them -- ONE
    synchronisation -- and allocates exactly; with ``capacity`` (rows, or ``(vertex rows, face rows)``) the arrays are views of buffers
    of that size instead, and a mesh that does not fit raises, naming the capacity needed, before anything is emitted."""
    bnd, closed, closed_value, capacity = _mesh_args(phi, bnd, closed, closed_value, capacity)
    with torch.no_grad():
        ph = _prep(phi.detach(), "phi")
        dims = [int(n) for n in ph.shape]
        B, ncell = dims[0], dims[1] * dims[2] * dims[3]
        n = B * ncell
        tail = [bnd, 1 if closed else 0, closed_value, _stream()]
        mask = _u8((n,), ph)
        counts = _u8((2, n), ph)
        call("df_mesh_count", _ptr(ph), _ptr(mask), _ptr(counts[0]), _ptr(counts[1]), *(dims + tail))
        offsets = torch.zeros((2, n + 1), dtype=torch.int32, device=ph.device)
        torch.cumsum(counts[0], 0, dtype=torch.int32, out=offsets[0, 1:])
        torch.cumsum(counts[1], 0, dtype=torch.int32, out=offsets[1, 1:])
        V, T = (int(x) for x in offsets[:, -1].cpu().numpy())           # the one synchronisation
        _mesh_fit(V, T, capacity)
        vcap, fcap = (V, T) if capacity is None else capacity
        vertices = _empty((vcap, 3), ph)
        nrm = _empty((vcap, 3), ph) if normals else None
        faces = torch.empty((fcap, 3), dtype=torch.int32, device=ph.device)
        call("df_mesh_emit", _ptr(ph), _ptr(mask), _ptr(offsets[0]), _ptr(offsets[1]), _ptr(vertices), _ptr(nrm), _ptr(faces), vcap, fcap,
             *(dims + tail))
        return SurfaceMesh(vertices[:V], faces[:T], None if nrm is None else nrm[:V], offsets[0, ::ncell].contiguous(),
                           offsets[1, ::ncell].contiguous())


def plane_view_np(x, xy_plane=True, project=True):
    """ops.py:326-342: host NumPy, x [Z,Y,X,C] -> float image in [0,255] (no uint8 cast)."""
    x = np.asarray(x)
    if xy_plane:
        x = np.mean(x, axis=0) if project else x[int(x.shape[0] / 2)]
    else:
        x = (np.mean(x, axis=2) if project else x[:, :, int(x.shape[2] / 2)]).transpose([1, 0, 2])
    return np.clip((x + 1) * 127.5, 0, 255)


# ---- NumPy-facing twins (ops.py:305-324, 344-374): ndarray in, ndarray out, computed on the GPU ----
def _np_in(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_DEFAULT_DEVICE)


def vort_np(x):
    """ops.py:305-310."""
    return jacobian(_np_in(x), data_format="NHWC")[1].cpu().numpy()


def curl_np(x):
    """ops.py:312-317."""
    return curl(_np_in(x)).cpu().numpy()


def grad_np(x):
    """ops.py:319-324: (dp/dx, dp/dy) == (-curl_v, curl_u)."""
    c = curl(_np_in(x)).cpu().numpy()
    return np.stack([-c[..., 1], c[..., 0]], axis=-1)


def jacobian_np3(x):
    """ops.py:344-374."""
    j, c = jacobian3(_np_in(x))
    return j.cpu().numpy(), c.cpu().numpy()


# --------------------------------------------------------------------------------------------------
# latent-space integrator, arch='nn' (model.py:218-224, trainer.py:586-747): libdeepfluids_hip_nn.so, include/deepfluids_hip_nn.h
# --------------------------------------------------------------------------------------------------
NN_BN_EPSILON = 1e-5        # ops.py:26 batch_norm(epsilon=1e-5, momentum=0.9)
NN_BN_DECAY = 0.9

# what the dropout mask of a training-mode `NN` application is a hash of, besides the element's row and column and the layer: the
# trainer's seed, the global step and the index of the application inside the window (see `nn_mask_state`)
_NN_MASK = {"seed": 123, "step": 0, "window": 0}


def nn_mask_state(seed=None, step=None, window=None):
    """Set (the arguments given) and return the mask state ``{"seed", "step", "window"}`` the next training-mode ``NN`` reads.  The
    reference's masks come from TensorFlow's generator, which cannot be restated; this hash is this project's own."""
    for k, v in (("seed", seed), ("step", step), ("window", window)):
        if v is not None:
            _NN_MASK[k] = int(v) & 0xFFFFFFFF
    return dict(_NN_MASK)


def batch_norm_variables(n, name=None, device=None):
    """The variables of ``slim.batch_norm(scale=True)`` under the current scope, slim's names and creation order:
    ``<BatchNorm>/beta`` (0), ``gamma`` (1), ``moving_mean`` (0), ``moving_variance`` (1)."""
    lname = _layer_name(name, "BatchNorm")
    return (get_variable(lname + "/beta", (int(n),), "zeros", device), get_variable(lname + "/gamma", (int(n),), "ones", device),
            get_variable(lname + "/moving_mean", (int(n),), "zeros", device), get_variable(lname + "/moving_variance", (int(n),), "ones", device))


class _NNBlockTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, keep_prob, seed, step, window, layer):
        x = _prep(x, "x"); gamma = _prep(gamma, "gamma"); beta = _prep(beta, "beta")
        B, N = x.shape
        act, out = torch.empty_like(x), torch.empty_like(x)
        mean, rstd = _empty((N,), x), _empty((N,), x)
        call("df_nn_bn_elu_dropout_fwd", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var), _ptr(act), _ptr(out),
             _ptr(mean), _ptr(rstd), B, N, NN_BN_EPSILON, NN_BN_DECAY, float(keep_prob), seed, step, window, layer, _stream())
        ctx.save_for_backward(x, act, gamma, mean, rstd)
        ctx.mask = (float(keep_prob), seed, step, window, layer)
        ctx.bptr = beta.data_ptr()
        return out

    @staticmethod
    def backward(ctx, gout):
        x, act, gamma, mean, rstd = ctx.saved_tensors
        gout = _prep(gout, "grad")
        B, N = x.shape
        gx = torch.empty_like(x)
        gg, gb = _empty((N,), x), _empty((N,), x)
        call("df_nn_bn_elu_dropout_bwd", _ptr(x), _ptr(act), _ptr(gout), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(gx), _ptr(gg), _ptr(gb),
             B, N, *(ctx.mask + (_stream(),)))
        return (gx, gg, gb) + (None,) * 7


def nn_bn_elu_dropout(x, gamma, beta, moving_mean, moving_var, train=True, keep_prob=0.1, seed=0, step=0, window=0, layer=0):
    """``slim.dropout(slim.batch_norm(x, activation_fn=elu), keep_prob, is_training=train)`` on [B,N] as one launch (two with its
    backward).  ``train=True``: batch statistics, ``moving_mean`` / ``moving_var`` updated IN PLACE (``updates_collections=None``), the
    hash mask of (seed, step, window, layer, row, column) kept with probability ``keep_prob`` and scaled by 1 / keep_prob.
    ``train=False``: moving statistics, no mask, no gradient."""
    mm, mv = _prep(moving_mean.detach(), "moving_mean"), _prep(moving_var.detach(), "moving_var")
    if train:
        u32 = [int(v) & 0xFFFFFFFF for v in (seed, step, window, layer)]
        return _NNBlockTrain.apply(x, gamma, beta, mm, mv, keep_prob, *u32)
    x = _prep(x.detach(), "x"); gamma = _prep(gamma.detach(), "gamma"); beta = _prep(beta.detach(), "beta")
    B, N = x.shape
    out = torch.empty_like(x)
    call("df_nn_bn_elu_infer", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mm), _ptr(mv), _ptr(out), B, N, NN_BN_EPSILON, _stream())
    return out


class _NNWindowAdvance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, xw, i, ratio):
        x = _prep(x, "x"); y = _prep(y, "y"); xw = _prep(xw, "xw")
        B, K = x.shape
        Z = y.shape[1]
        if xw.dim() != 3 or xw.shape[0] != B or xw.shape[2] != K or y.shape[0] != B or Z >= K:
            raise ValueError("nn_window_advance: x %s, y %s, xw %s do not belong together" % (tuple(x.shape), tuple(y.shape), tuple(xw.shape)))
        xn = torch.empty_like(x)
        call("df_nn_window_advance_fwd", _ptr(x), _ptr(y), _ptr(xw), _ptr(xn), B, xw.shape[1], Z, K - Z, int(i), float(ratio), _stream())
        ctx.dims = (B, Z, K - Z, float(ratio))
        return xn

    @staticmethod
    def backward(ctx, gxn):
        gxn = _prep(gxn, "grad")
        B, Z, P, ratio = ctx.dims
        gx = torch.empty_like(gxn) if ctx.needs_input_grad[0] else None
        gy = _empty((B, Z), gxn) if ctx.needs_input_grad[1] else None
        call("df_nn_window_advance_bwd", _ptr(gxn), _ptr(gx), _ptr(gy), B, Z, P, ratio, _stream())
        return gx, gy, None, None, None


def nn_window_advance(x, y, xw, i, ratio):
    """trainer.py:608-614: ``concat(x[:, :-p] + y * ratio, xw[:, i+1, -p:])`` with ratio = out_std / code_std; x [B,z+p], y [B,z],
    xw [B,w,z+p].  The gradient flows to ``x[:, :-p]`` and to ``y``."""
    return _NNWindowAdvance.apply(x, y, xw, i, ratio)


class _NNWindowStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *ys):
        ys = [_prep(y, "y") for y in ys]
        B, Z = ys[0].shape
        W = len(ys)
        out = _empty((B, W, Z), ys[0])
        for i, y in enumerate(ys):
            if tuple(y.shape) != (B, Z):
                raise ValueError("nn_window_stack: entry %d is %s, entry 0 is %s" % (i, tuple(y.shape), (B, Z)))
            call("df_nn_rows_copy", _ptr(y), Z, out.data_ptr() + 4 * i * Z, W * Z, B, Z, _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        g = _prep(g, "grad")
        B, W, Z = g.shape
        gys = []
        for i in range(W):
            gy = None
            if ctx.needs_input_grad[i]:
                gy = _empty((B, Z), g)
                call("df_nn_rows_copy", g.data_ptr() + 4 * i * Z, W * Z, _ptr(gy), Z, B, Z, _stream())
            gys.append(gy)
        return tuple(gys)


def nn_window_stack(ys):
    """The window's predictions, w tensors [B,z], as yw_ [B,w,z] (``tf.concat`` of the expanded entries, trainer.py:597-606)."""
    return _NNWindowStack.apply(*ys)


class _NNMse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a = _prep(a, "a"); b = _prep(b, "b")
        if a.shape != b.shape:
            raise ValueError("nn_mse: shapes differ %s vs %s" % (tuple(a.shape), tuple(b.shape)))
        n = a.numel()
        out = _empty((), a)
        nbytes = query("df_nn_mse_workspace_bytes", n)
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=a.device)
        call("df_nn_mse_fwd", _ptr(a), _ptr(b), n, _ptr(out), _ptr(ws), nbytes, _stream())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        gout = _prep(gout, "grad")
        ga = torch.empty_like(a)
        call("df_nn_mse_bwd", _ptr(a), _ptr(b), _ptr(gout), _ptr(ga), a.numel(), _stream())
        return ga, None


def nn_mse(pred, target):
    """``tf.losses.mean_squared_error(target, pred)`` (trainer.py:630): the mean over every element, summed in the fixed order of
    deepfluids_hip_nn.h; the gradient 2 (pred - target) / count goes to ``pred``."""
    return _NNMse.apply(pred, target.detach())


def nn_rollout(x_test, y_test, variables, num_scenes, num_frames, z_num, code_std, out_std):
    """``test_nn`` (trainer.py:698-747) for every test scene in ONE launch: ``z_out`` [num_scenes, num_frames, z_num].  ``x_test``
    [num_scenes (num_frames - 1), z_num + p_num] and ``y_test`` [.., z_num] are the normalised rows of the batch manager; ``variables``
    maps the slim names below the network's scope (``fully_connected/weights`` ... ``BatchNorm_1/moving_variance``) to tensors."""
    x_test = _prep(x_test, "x_test"); y_test = _prep(y_test, "y_test")
    S, F, Z = int(num_scenes), int(num_frames), int(z_num)
    K0 = x_test.shape[1]
    if tuple(x_test.shape) != (S * (F - 1), K0) or tuple(y_test.shape) != (S * (F - 1), Z) or K0 <= Z:
        raise ValueError("nn_rollout: x_test %s / y_test %s are not %d scenes of %d frames with a code of %d" % (
            tuple(x_test.shape), tuple(y_test.shape), S, F, Z))
    v = {k: _prep(t.detach(), k) for k, t in variables.items()}
    names = ["fully_connected/weights", "fully_connected/biases", "BatchNorm/gamma", "BatchNorm/beta", "BatchNorm/moving_mean",
             "BatchNorm/moving_variance", "fully_connected_1/weights", "fully_connected_1/biases", "BatchNorm_1/gamma", "BatchNorm_1/beta",
             "BatchNorm_1/moving_mean", "BatchNorm_1/moving_variance", "fully_connected_2/weights", "fully_connected_2/biases"]
    w1, w2, w3 = v[names[0]], v[names[6]], v[names[12]]
    N1, N2 = w1.shape[1], w2.shape[1]
    if tuple(w1.shape) != (K0, N1) or tuple(w2.shape) != (N1, N2) or tuple(w3.shape) != (N2, Z):
        raise ValueError("nn_rollout: weights %s, %s, %s do not chain from %d to %d" % (tuple(w1.shape), tuple(w2.shape), tuple(w3.shape), K0, Z))
    for k, n in zip(names, [None, N1, N1, N1, N1, N1, None, N2, N2, N2, N2, N2, None, Z]):
        if n is not None and tuple(v[k].shape) != (n,):
            raise ValueError("nn_rollout: %s is %s, expected (%d,)" % (k, tuple(v[k].shape), n))
    z_out = _empty((S, F, Z), x_test)
    call("df_nn_rollout", _ptr(x_test), _ptr(y_test), *([_ptr(v[k]) for k in names] + [_ptr(z_out), S, F, Z, K0 - Z, N1, N2, NN_BN_EPSILON,
                                                                                        float(code_std), float(out_std), _stream()]))
    return z_out
