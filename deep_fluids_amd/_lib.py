"""ctypes binding of libdeepfluids_hip.so (the C-ABI declared in include/deepfluids_hip.h).

There is NO fallback: if the HIP library is missing this module raises at import of the first
symbol, and every compute entry point of the package goes through it.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libdeepfluids_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "deepfluids_hip.h")
# the fused field metrics: a library and a header of their own (deepfluids_hip.h is frozen at DF_VERSION 207), bound the same way
METRICS_LIB_PATH = os.path.join(_HERE, "csrc", "libdeepfluids_hip_metrics.so")
METRICS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "deepfluids_hip_metrics.h")
# the latent-space integrator (arch='nn'): likewise a library and a header of its own
NN_LIB_PATH = os.path.join(_HERE, "csrc", "libdeepfluids_hip_nn.so")
NN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "deepfluids_hip_nn.h")
# SSIM / MS-SSIM: likewise
SSIM_LIB_PATH = os.path.join(_HERE, "csrc", "libdeepfluids_hip_ssim.so")
SSIM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "deepfluids_hip_ssim.h")
# the multigrid preconditioner for the liquid and diffusion systems: likewise
LIQUID_MG_LIB_PATH = os.path.join(_HERE, "csrc", "libdeepfluids_hip_liquid_mg.so")
LIQUID_MG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "deepfluids_hip_liquid_mg.h")

P, I64, I32, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
U32 = ctypes.c_uint32

# the header's scalar types; a parameter with a `*` in it is a pointer whatever it points to
CTYPES = {"int": I32, "int64_t": I64, "float": F32, "uint32_t": U32, "df_stream_t": P, "const char*": ctypes.c_char_p}


class DeepFluidsHipError(RuntimeError):
    pass


def parse_header(text):
    """The header is the only description of the C-ABI:  ``(signatures, constants)`` of its text, signatures as name -> (restype, argtypes),
    constants as name -> int for ``DF_VERSION`` and every enumerator.  Strict: every statement with a parenthesis in it must be a
    ``ret df_name(params);`` whose types are all in ``CTYPES``; anything else raises instead of binding a guess."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    constants = {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+(DF_VERSION)\s+(\d+)", text, re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, re.S):
        constants.update((n, int(v, 0)) for n, v in re.findall(r"(\w+)\s*=\s*([-+\w]+)", body))

    def ctype(decl, proto):
        t = re.sub(r"\s*\*\s*", "* ", decl).strip()
        if t not in CTYPES:
            raise DeepFluidsHipError("%s: type `%s` is not one the ctypes binding knows (%s)" % (proto, t, ", ".join(sorted(CTYPES))))
        return CTYPES[t]

    signatures = {}
    for stmt in re.split(r"[;{}]", re.sub(r"^\s*#.*$", "", text, flags=re.M)):
        if "(" not in stmt:
            continue
        proto = " ".join(stmt.split())
        m = re.fullmatch(r"(.+?)\b(df_\w+) ?\((.*)\)", proto)
        if m is None:
            raise DeepFluidsHipError("not a `ret df_name(params)` prototype: %s" % proto)
        params = [] if m.group(3).strip() == "void" else [q.strip() for q in m.group(3).split(",")]
        # a parameter is `type name`: the name goes, and what holds a `*` is a pointer
        signatures[m.group(2)] = (ctype(m.group(1), proto), [P if "*" in q else ctype(re.sub(r"\w+$", "", q), proto) for q in params])
    return signatures, constants


def _read_header(path=None):
    path = path or HEADER_PATH
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise DeepFluidsHipError("the C-ABI header %s cannot be read (%s): the ctypes binding is derived from it" % (path, e))


# SIGNATURES: name -> (restype, argtypes) of every entry point;  CONSTANTS: DF_VERSION, the status codes DF_OK / DF_EINVAL / DF_ESHAPE / DF_EALIGN /
# DF_EWORKSPACE and the conv flags DF_CONV_LRELU / _RESIDUAL / _MASK / _BIAS / _ADDUP / _VALU_ONLY, each also a module attribute of its own name
SIGNATURES, CONSTANTS = parse_header(_read_header())
globals().update(CONSTANTS)
# ... and of deepfluids_hip_metrics.h: df_field_metrics* and the DF_FM_* word indices of their output rows
METRICS_SIGNATURES, METRICS_CONSTANTS = parse_header(_read_header(METRICS_HEADER_PATH))
globals().update(METRICS_CONSTANTS)
# ... and of deepfluids_hip_nn.h: df_nn_*
NN_SIGNATURES, NN_CONSTANTS = parse_header(_read_header(NN_HEADER_PATH))
# ... and of deepfluids_hip_ssim.h: df_ssim* and the DF_SSIM_* word indices and limits
SSIM_SIGNATURES, SSIM_CONSTANTS = parse_header(_read_header(SSIM_HEADER_PATH))
globals().update(SSIM_CONSTANTS)
# ... and of deepfluids_hip_liquid_mg.h: the level-0 builders and the iteration of the liquid and diffusion systems
LIQUID_MG_SIGNATURES, _ = parse_header(_read_header(LIQUID_MG_HEADER_PATH))


class NoiseParams(ctypes.Structure):
    """``df_noise_params`` of the header: the host-side argument of ``df_density_noise_inflow*`` (pass ``ctypes.addressof`` of it)"""
    _fields_ = [("pos_scale", F32 * 3), ("pos_offset", F32 * 3), ("time_anim", F32), ("val_offset", F32), ("val_scale", F32),
                ("clamp", ctypes.c_int32), ("clamp_neg", F32), ("clamp_pos", F32), ("seed", ctypes.c_uint32), ("inv_extent", F32)]


_lib = None
_metrics_lib = None
_nn_lib = None
_ssim_lib = None
_liquid_mg_lib = None


def declared_symbols():
    """Every function the public header declares (used by the export test)."""
    src = open(HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(df_[a-z0-9_]+)\s*\(", src)))


def lib():
    global _lib, LIB_PATH
    if _lib is None:
        if os.environ.get("DF_HIP_LIBRARY"):          # sanitizer runs only (tools/run_asan.sh): another BUILD of the same library
            LIB_PATH = os.environ["DF_HIP_LIBRARY"]
        if not os.path.exists(LIB_PATH):
            raise DeepFluidsHipError(
                "libdeepfluids_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C deep_fluids_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def metrics_lib():
    """libdeepfluids_hip_metrics.so; the main library is loaded first (it holds the error buffer the metrics library writes to)"""
    global _metrics_lib
    if _metrics_lib is None:
        lib()
        if not os.path.exists(METRICS_LIB_PATH):
            raise DeepFluidsHipError("libdeepfluids_hip_metrics.so not found at %s -- `make -C deep_fluids_amd/csrc` builds it with the main "
                                     "library. There is no CPU fallback." % METRICS_LIB_PATH)
        handle = ctypes.CDLL(METRICS_LIB_PATH)
        for name, (res, args) in METRICS_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _metrics_lib = handle
    return _metrics_lib


def nn_lib():
    """libdeepfluids_hip_nn.so; the main library is loaded first (it holds the error buffer the nn library writes to)"""
    global _nn_lib
    if _nn_lib is None:
        lib()
        if not os.path.exists(NN_LIB_PATH):
            raise DeepFluidsHipError("libdeepfluids_hip_nn.so not found at %s -- `make -C deep_fluids_amd/csrc` builds it with the main "
                                     "library. There is no CPU fallback." % NN_LIB_PATH)
        handle = ctypes.CDLL(NN_LIB_PATH)
        for name, (res, args) in NN_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _nn_lib = handle
    return _nn_lib


def ssim_lib():
    """libdeepfluids_hip_ssim.so; the main library is loaded first (it holds the error buffer the ssim library writes to)"""
    global _ssim_lib
    if _ssim_lib is None:
        lib()
        if not os.path.exists(SSIM_LIB_PATH):
            raise DeepFluidsHipError("libdeepfluids_hip_ssim.so not found at %s -- `make -C deep_fluids_amd/csrc` builds it with the main "
                                     "library. There is no CPU fallback." % SSIM_LIB_PATH)
        handle = ctypes.CDLL(SSIM_LIB_PATH)
        for name, (res, args) in SSIM_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _ssim_lib = handle
    return _ssim_lib


def liquid_mg_lib():
    """libdeepfluids_hip_liquid_mg.so; the main library is loaded first (it holds the error buffer this library writes to)"""
    global _liquid_mg_lib
    if _liquid_mg_lib is None:
        lib()
        if not os.path.exists(LIQUID_MG_LIB_PATH):
            raise DeepFluidsHipError("libdeepfluids_hip_liquid_mg.so not found at %s -- `make -C deep_fluids_amd/csrc` builds it with the main "
                                     "library. There is no CPU fallback." % LIQUID_MG_LIB_PATH)
        handle = ctypes.CDLL(LIQUID_MG_LIB_PATH)
        for name, (res, args) in LIQUID_MG_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _liquid_mg_lib = handle
    return _liquid_mg_lib


def _handle(name):
    if name in NN_SIGNATURES:
        return nn_lib()
    if name in LIQUID_MG_SIGNATURES:
        return liquid_mg_lib()
    if name in SSIM_SIGNATURES:
        return ssim_lib()
    return metrics_lib() if name in METRICS_SIGNATURES else lib()


class KernelTimer(object):
    """Optional HIP-event timing of selected C-ABI calls (bench.py's live roofline measurement).

    ``select(name, args)`` returns None or ``(key, work)``; matching calls are bracketed by two events recorded
    on the CURRENT torch stream -- the stream the kernels are launched on -- and summarised after a sync."""

    def __init__(self, select):
        self.select = select
        self.records = []

    def summary(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for key, work, e0, e1 in self.records:
            d = out.setdefault(key, {"launches": 0, "seconds": 0.0, "work": 0.0})
            d["launches"] += 1
            d["seconds"] += e0.elapsed_time(e1) * 1e-3
            d["work"] += work
        return out


TIMER = None   # set to a KernelTimer to enable


def call(name, *args):
    """Call an int-returning df_* entry point; raise with df_last_error() on failure."""
    h = lib()
    hit = TIMER.select(name, args) if TIMER is not None else None
    if hit is not None:
        import torch
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(_handle(name), name)(*args)
        e1.record()
        TIMER.records.append((hit[0], hit[1], e0, e1))
    else:
        rc = getattr(_handle(name), name)(*args)
    if rc != 0:
        msg = h.df_last_error()
        raise DeepFluidsHipError("%s failed (%d): %s" % (name, rc, msg.decode() if msg else ""))


_QUERY_CACHE = {}


def query(name, *args):
    """Call a value-returning helper (workspace sizes, packed-operand sizes, algorithm forms, version).  One without a pointer argument is a pure
    function of its integer arguments, so its answers are memoised: a 2-D train step at the reference's default batch asks ~150 of them, and its
    host issue time (2.6 ms) is within a millisecond of the device time (3.5 ms).  One that takes a pointer is asked every time (a cache keyed on
    addresses only grows)."""
    key = (name,) + args
    try:
        return _QUERY_CACHE[key]
    except KeyError:
        v = getattr(_handle(name), name)(*args)
        if P not in (NN_SIGNATURES.get(name) or SSIM_SIGNATURES.get(name) or METRICS_SIGNATURES.get(name) or LIQUID_MG_SIGNATURES.get(name)
                     or SIGNATURES[name])[1]:
            _QUERY_CACHE[key] = v
        return v
