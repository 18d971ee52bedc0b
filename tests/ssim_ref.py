"""NumPy restatement of SSIM / MS-SSIM as include/deepfluids_hip_ssim.h defines them, in either precision: ``dtype=float64`` is the
truth (unrounded taps, every step in fp64), ``float32`` is the op-for-op twin of csrc/ssim.hip -- the taps rounded once, the planes, both
filter passes and the values in fp32 in the header's tap and operation order, the per-thread sums in fp32, the sums across threads,
workgroups and images in fp64 in the header's tree -- whose bits the kernels must give.

Also the seeded inputs of the SSIM tests: tests/golden/make_golden_ssim.py runs the reference on exactly these and stores a checksum of
each, so the arrays themselves need not be stored.

Shared by tests/test_ssim_host.py (no GPU), tests/test_gpu_ssim.py and tests/golden/make_golden_ssim.py."""
import functools
import os
import re

import numpy as np

F32, F64 = np.float32, np.float64
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = re.sub(r"/\*.*?\*/", "", open(os.path.join(_ROOT, "include", "deepfluids_hip_ssim.h")).read(), flags=re.S)
CONST = {n[len("DF_SSIM_"):].lower(): int(v) for n, v in re.findall(r"(DF_SSIM_\w+)\s*=\s*(\d+)", _HDR)}
TILE, MAX_SIZE, WORDS = CONST["tile"], CONST["max_size"], CONST["words"]
K_THREADS, WAVE, PER_THREAD = 256, 64, 4
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
DEFAULTS = dict(filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, min_val=-1.0, max_val=1.0)


def taps(size, sigma, dtype=F32):
    """the normalised 1-D factor of the window: fp64, and for the twin rounded to fp32 once"""
    u = np.arange(size, dtype=F64) - size // 2 + (0.5 if size % 2 == 0 else 0.0)
    e = np.exp(-(u * u) / (2.0 * float(sigma) ** 2))
    return (e / e.sum()).astype(dtype)


def window(size, sigma, channels):
    """the reference's ``fspecial_gauss`` [size,size,C,C] from the 1-D factor, fp64: t_i t_j / C^2"""
    t = taps(size, sigma, F64)
    return np.broadcast_to((t[:, None] * t[None, :] / channels ** 2)[:, :, None, None], (size, size, channels, channels)).copy()


def _tree(v):
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


def _strided(v):
    """[..., n] fp64 -> [...]: step 3 of the header (thread t adds elements t, t + 256, ... from 0; then the tree)"""
    n = v.shape[-1]
    k = -(-n // K_THREADS)
    q = np.zeros(v.shape[:-1] + (k * K_THREADS,), F64)
    q[..., :n] = v
    q = q.reshape(v.shape[:-1] + (k, K_THREADS))
    a = np.zeros(v.shape[:-1] + (K_THREADS,), F64)
    for i in range(k):
        a = a + q[..., i, :]
    return _waves(a)


def image_totals(m, dtype):
    """m [N,H',W'] in ``dtype`` -> the images' fp64 totals [N] in the header's order"""
    N, OH, OW = m.shape
    nty, ntx = -(-OH // TILE), -(-OW // TILE)
    p = np.zeros((N, nty * TILE, ntx * TILE), dtype)
    p[:, :OH, :OW] = m                                               # a pixel that does not exist adds +0 to a sum that starts at +0
    p = p.reshape(N, nty, TILE // PER_THREAD, PER_THREAD, ntx, TILE)      # [n, ty, yq, i, tx, x]
    t = np.zeros((N, nty, TILE // PER_THREAD, ntx, TILE), dtype)
    for i in range(PER_THREAD):                                      # 1. per thread, ascending i, in dtype
        t = t + p[:, :, :, i]
    assert t.dtype == dtype
    t = t.transpose(0, 1, 3, 2, 4).reshape(N, nty * ntx, K_THREADS)  # tile ty * TX + tx; thread 32 yq + x
    return _strided(_waves(t.astype(F64)))                           # 2. and 3.


def group_mean(totals, count, groups):
    """``df_ssim_group_mean``: totals [N] fp64 -> [G] fp64"""
    t = np.asarray(totals, F64).reshape(groups, -1)
    return _strided(t) / (F64(t.shape[1]) * F64(count))


def ssim(a, b, dtype=F32, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, min_val=-1.0, max_val=1.0):
    """one level: ``{"size", "sigma", "ssim_map", "cs_map" [N,H',W'] in dtype, "sum", "sum_cs" fp64 [N], "mean", "mean_cs" dtype [N],
    "count"}``"""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    assert a.shape == b.shape and a.ndim == 4
    N, H, W, C = a.shape
    size = min(filter_size, H, W)
    sigma = filter_sigma * size / filter_size
    t = taps(size, sigma, dtype)
    lo, rng = dtype(min_val), dtype(max_val) - dtype(min_val)
    p, q = (a - lo) / rng, (b - lo) / rng
    planes = []
    for u, v in ((p, None), (q, None), (p, p), (q, q), (p, q)):
        term = u if v is None else u * v
        s = term[..., 0]
        for c in range(1, C):
            s = s + term[..., c]
        planes.append(s)
    OH, OW = H - size + 1, W - size + 1
    F = []
    for P in planes:
        R = np.zeros((N, H, OW), dtype)
        for j in range(size):
            R = R + t[j] * P[:, :, j:j + OW]
        V = np.zeros((N, OH, OW), dtype)
        for i in range(size):
            V = V + t[i] * R[:, i:i + OH]
        assert V.dtype == dtype
        F.append(V)
    s = dtype(1.0 / (C * C))
    c1, c2 = dtype(k1) * dtype(k1), dtype(k2) * dtype(k2)
    mu1, mu2, e11, e22, e12 = (f * s for f in F)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = e11 - mu11, e22 - mu22, e12 - mu12
    two = dtype(2.0)
    v1, v2 = two * s12 + c2, (s11 + s22) + c2
    with np.errstate(all="ignore"):
        val = ((two * mu12 + c1) * v1) / (((mu11 + mu22) + c1) * v2)
        cs = v1 / v2
    assert val.dtype == dtype and cs.dtype == dtype
    count = OH * OW
    tot, tot_cs = image_totals(val, dtype), image_totals(cs, dtype)
    return {"size": size, "sigma": sigma, "ssim_map": val, "cs_map": cs, "sum": tot, "sum_cs": tot_cs, "count": count,
            "mean": (tot / F64(count)).astype(dtype), "mean_cs": (tot_cs / F64(count)).astype(dtype)}


def raw_words(r):
    """the int32 rows [N, DF_SSIM_WORDS] the kernel writes for a float32 result of ``ssim``"""
    N = len(r["sum"])
    raw = np.zeros((N, WORDS), np.int32)
    raw[:, CONST["count"]] = r["count"]
    raw[:, CONST["mean"]] = r["mean"].astype(F32).view(np.int32)
    raw[:, CONST["mean_cs"]] = r["mean_cs"].astype(F32).view(np.int32)
    raw[:, CONST["sum"]:CONST["sum"] + 2] = np.ascontiguousarray(r["sum"], F64).view(np.int32).reshape(N, 2)
    raw[:, CONST["sum_cs"]:CONST["sum_cs"] + 2] = np.ascontiguousarray(r["sum_cs"], F64).view(np.int32).reshape(N, 2)
    return raw


def pool(v, dtype=F32):
    """TF's avg_pool 2x2 / stride 2 / 'SAME' of [N,H,W,C]: the elements that exist added in the header's order, times 1 / their number"""
    v = np.asarray(v, dtype)
    N, H, W, C = v.shape
    he, we = H // 2, W // 2
    out = np.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype)
    out[:, :he, :we] = (((v[:, 0:2 * he:2, 0:2 * we:2] + v[:, 0:2 * he:2, 1:2 * we:2]) + v[:, 1:2 * he:2, 0:2 * we:2])
                        + v[:, 1:2 * he:2, 1:2 * we:2]) * dtype(0.25)
    if W % 2:
        out[:, :he, we] = (v[:, 0:2 * he:2, W - 1] + v[:, 1:2 * he:2, W - 1]) * dtype(0.5)
    if H % 2:
        out[:, he, :we] = (v[:, H - 1, 0:2 * we:2] + v[:, H - 1, 1:2 * we:2]) * dtype(0.5)
    if H % 2 and W % 2:
        out[:, he, we] = v[:, H - 1, W - 1]
    return out


def ms_ssim(a, b, dtype=F32, groups=1, min_val=-1.0, max_val=1.0):
    """``{"levels": [ssim results], "images": [(a, b) per level], "mssim", "mcs" fp64 [5, G], "value" [G]}``: the group means of
    every level from the fp64 totals, combined in fp64; ``value`` in ``dtype`` (nan where a power's base is not positive)"""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    levels, images = [], []
    for k in range(len(WEIGHTS)):
        images.append((a, b))
        levels.append(ssim(a, b, dtype, min_val=min_val, max_val=max_val))
        if k < len(WEIGHTS) - 1:
            a, b = pool(a, dtype), pool(b, dtype)
    mssim = np.stack([group_mean(r["sum"], r["count"], groups) for r in levels])
    mcs = np.stack([group_mean(r["sum_cs"], r["count"], groups) for r in levels])
    w = np.asarray(WEIGHTS, F64)
    with np.errstate(invalid="ignore"):
        value = np.prod(mcs[:-1] ** w[:-1, None], axis=0) * mssim[-1] ** w[-1]
    return {"levels": levels, "images": images, "mssim": mssim, "mcs": mcs, "value": value.astype(dtype)}


# ---- the cases of the tests and of the golden ---------------------------------------------------------------------------------------
# (H, W): what each one crosses
SSIM_SHAPES = [
    ((11, 11), "one output pixel"),
    ((12, 17), "2 x 7 outputs, odd width"),
    ((7, 20), "the window shrinks to 7 taps"),
    ((6, 9), "an even window: the half-cell offset"),
    ((1, 5), "a window of one tap"),
    ((33, 45), "23 x 35 outputs: a second, ragged tile along x"),
    ((64, 70), "54 x 60 outputs: two ragged tiles along both axes"),
]
SSIM_CHANNELS = (1, 2, 3)
SSIM_N = 3
WINDOWS = [(11, 1.5), (7, 1.5 * 7 / 11), (6, 1.5 * 6 / 11), (1, 1.5 / 11)]      # the sizes the shapes above reach
MS_CASES = [((16, 16), 1), ((21, 16), 2), ((37, 50), 3), ((128, 96), 2)]
MS_N = 2
MS_NOISE = (0.05, 0.3)
POOL_CASE = ((37, 50), 3)                                            # -> (19,25) -> (10,13) -> (5,7) -> (3,4)


def _ro(a):
    a.setflags(write=False)
    return a


def _field(rng, N, H, W, C):
    """a smooth field of amplitude 0.8: a few low-frequency waves with random phases"""
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = np.zeros((N, H, W, C))
    for n in range(N):
        for c in range(C):
            ph = rng.uniform(0, 2 * np.pi, 4)
            f[n, :, :, c] = 0.4 * np.sin(2 * np.pi * x / 37.0 + ph[0]) * np.cos(2 * np.pi * y / 29.0 + ph[1]) \
                + 0.4 * np.sin(2 * np.pi * (x + y) / 53.0 + ph[2]) * np.cos(2 * np.pi * (x - y) / 41.0 + ph[3])
    return f


@functools.lru_cache(maxsize=None)
def inputs(shape, channels, noise=0.05, n=SSIM_N):
    """(truth, generated) float32 [n,H,W,C], read-only, seeded by the case: a smooth field of amplitude 0.8 plus N(0, 0.1) as the
    ground truth, that plus N(0, noise) as the generated field"""
    H, W = shape
    rng = np.random.RandomState(4000 + 131 * H + 17 * W + channels + int(round(noise * 1000)))
    x = _field(rng, n, H, W, channels) + rng.normal(0, 0.1, (n, H, W, channels))
    g = x + rng.normal(0, noise, (n, H, W, channels))
    return _ro(x.astype(F32)), _ro(g.astype(F32))


def checksum(a, b):
    """what the golden stores in place of the seeded inputs"""
    return np.array([np.asarray(a, F64).sum(), np.square(np.asarray(a, F64)).sum(), np.asarray(b, F64).sum(), np.square(np.asarray(b, F64)).sum()])


@functools.lru_cache(maxsize=None)
def reference(shape, channels):
    """(fp32 twin, fp64 truth) of one SSIM case on the shared inputs, computed once"""
    x, g = inputs(shape, channels)
    return ssim(g, x, F32), ssim(g, x, F64)


@functools.lru_cache(maxsize=None)
def ms_reference(shape, channels, noise, negate=False):
    """(fp32 twin, fp64 truth) of one MS-SSIM case"""
    x, g = inputs(shape, channels, noise, MS_N)
    if negate:
        x = -x
    return ms_ssim(g, x, F32), ms_ssim(g, x, F64)
