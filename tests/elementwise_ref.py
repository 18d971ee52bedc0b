"""NumPy restatements of the small train-step kernels of csrc/elementwise.hip, written from the kernels' definitions and parametrised by
dtype: float64 is the reference of the GPU tests (tests/test_gpu_elementwise.py); float32 is the op-for-op twin -- the kernel's own order of
operations and its own mix of precisions (a kernel that accumulates in double does so in the twin as well) -- whose distance from float64
sets their tolerance.  The library is built with -ffp-contract=off, so an fp32 expression rounds after every operation exactly as NumPy's
float32 does; the explicit fmaf of the linear kernels is emulated through a double (one extra rounding in rare cases: the linear twins are
informative, their tests use an a-priori bound).  Also the case tables and seeded inputs that the host gate (tests/test_elementwise_host.py)
and the GPU tests share.  Plain helper: no GPU, no torch, no fixtures."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
EXACT = float(1 << 24)          # integers below this magnitude are exact in fp32, hence so is any sum of them in any order
U = 2.0 ** -24                  # unit round-off of fp32

# constants of the source that the case tables are built around
K_THREADS, K_MAX_BLOCKS, K_FC_CHUNK, K_COLSUM_ROWS, K_EW_TILE = 256, 2048, 2048, 512, 4 * 256 * 4
WRAP = K_THREADS * K_MAX_BLOCKS          # 524288: a grid-stride loop takes a second trip above this many work items


def _t(dtype):
    return np.dtype(dtype).type


def _quiet():
    return np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- optimisers -----------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, lr_t, b1, b2, eps, gscale, dtype):
    """adam_kernel: gi = g*gscale; m' = b1*m + (1-b1)*gi; v' = b2*v + ((1-b2)*gi)*gi; p' = p - (lr_t*m') / (sqrt(v') + eps)."""
    T = _t(dtype)
    p, g, m, v = (np.asarray(a).astype(T) for a in (p, g, m, v))
    lr_t, b1, b2, eps, gscale = T(lr_t), T(b1), T(b2), T(eps), T(gscale)
    with _quiet():
        gi = g * gscale
        mi = b1 * m + (T(1) - b1) * gi
        vi = b2 * v + ((T(1) - b2) * gi) * gi
        pn = p - (lr_t * mi) / (np.sqrt(vi) + eps)
    return pn, mi, vi


def gd(p, g, lr, gscale, dtype):
    """gd_kernel: a = lr * gscale formed once, then p - a * g."""
    T = _t(dtype)
    a = T(lr) * T(gscale)
    with _quiet():
        return np.asarray(p).astype(T) - a * np.asarray(g).astype(T)


def store_scalars(dst, n, vals):
    out = np.array(dst, F32)
    out[:n] = np.asarray(vals, F32)[:n]
    return out


# ---- lrelu / add ----------------------------------------------------------------------------------------------------------------------
def lrelu(x, leak, dtype):
    T = _t(dtype)
    x = np.asarray(x).astype(T)
    return np.maximum(x, T(leak) * x)


def lrelu_bwd(gy, y, leak, dtype):
    T = _t(dtype)
    gy = np.asarray(gy).astype(T)
    return np.where(np.asarray(y) > 0, gy, T(leak) * gy)


def add(a, b, dtype):
    T = _t(dtype)
    return np.asarray(a).astype(T) + np.asarray(b).astype(T)


# ---- means ----------------------------------------------------------------------------------------------------------------------------
def l1_mean(a, b, dtype):
    """|a-b| in the working precision, summed in double (the kernel promotes fp32 partials of <= 256 terms), times the double 1/n."""
    T = _t(dtype)
    d = np.abs(np.asarray(a).astype(T) - np.asarray(b).astype(T))
    s = float(d.astype(F64).sum())
    return T(s * (1.0 / d.size))


def l1_mean_bwd(a, b, gout, scale, dtype):
    """sgn(a-b) * s with s = (scale / T(n)) * gout, 0 at ties."""
    T = _t(dtype)
    a, b = np.asarray(a).astype(T), np.asarray(b).astype(T)
    s = (T(scale) / T(a.size)) * T(gout)
    return (np.sign(a - b) * s).astype(T)


def mse_mean(a, b, dtype):
    """d = a-b, d*d in the working precision, accumulated in double, times the double 1/n."""
    T = _t(dtype)
    d = np.asarray(a).astype(T) - np.asarray(b).astype(T)
    s = float((d * d).astype(F64).sum())
    return T(s * (1.0 / d.size))


def mse_mean_bwd(a, b, gout, scale, dtype):
    """(2 * (a-b)) * s with s = (scale / T(n)) * gout."""
    T = _t(dtype)
    a, b = np.asarray(a).astype(T), np.asarray(b).astype(T)
    s = (T(scale) / T(a.size)) * T(gout)
    return (T(2) * (a - b)) * s


# ---- sigmoid --------------------------------------------------------------------------------------------------------------------------
def sigmoid(x, dtype):
    T = _t(dtype)
    x = np.asarray(x).astype(T)
    with _quiet():
        return T(1) / (T(1) + np.exp(-x))


def sigmoid_bwd(gy, y, dtype):
    T = _t(dtype)
    gy, y = np.asarray(gy).astype(T), np.asarray(y).astype(T)
    return (gy * y) * (T(1) - y)


# ---- Bernoulli KL ---------------------------------------------------------------------------------------------------------------------
# The kernel works in double throughout (column means, logs) and rounds once at the end (forward) or before two fp32 multiplies (backward);
# float64 below is the plain formula, float32 the kernel's order: means summed over b ascending, thread t owns columns t, t+256, ..., the
# 256 thread sums are added in order.  rho is an fp32 argument: both take the value it has after that rounding.
def _kl_col_means(z, n):
    z = np.asarray(z)
    m = np.zeros(n, F64)
    for b in range(z.shape[0]):
        m = m + z[b, :n].astype(F64)
    return m / z.shape[0]


def kl_bernoulli(z, n, rho, dtype):
    rho = float(rho)
    if _t(dtype) is F64:
        q = np.asarray(z, F64)[:, :n].mean(axis=0)
        return float((rho * np.log(rho / q) + (1 - rho) * np.log((1 - rho) / (1 - q))).sum())
    m = _kl_col_means(z, n)
    term = rho * np.log(rho / m) + (1.0 - rho) * np.log((1.0 - rho) / (1.0 - m))
    per_thread = np.zeros(K_THREADS, F64)
    for j in range(n):
        per_thread[j % K_THREADS] += term[j]
    t = 0.0
    for i in range(K_THREADS):
        t += per_thread[i]
    return F32(t)


def kl_bernoulli_bwd(z, n, rho, gout, scale, dtype):
    rho = float(rho)
    z = np.asarray(z)
    B = z.shape[0]
    if _t(dtype) is F64:
        q = z.astype(F64)[:, :n].mean(axis=0)
        g = np.zeros(z.shape, F64)
        g[:, :n] = (-rho / q + (1 - rho) / (1 - q)) / B * float(gout) * float(scale)
        return g
    m = _kl_col_means(z, n)
    col = ((-rho / m + (1.0 - rho) / (1.0 - m)) / B).astype(F32) * F32(gout) * F32(scale)
    g = np.zeros(z.shape, F32)
    g[:, :n] = col
    return g


# ---- up-sampling family; every tensor is [B, D, H, W, C], D = 1 and untouched when not is3d ---------------------------------------------
def _axes(is3d):
    return (1, 2, 3) if is3d else (2, 3)


def upsample2x(x, is3d):
    x = np.asarray(x)
    for a in _axes(is3d):
        x = np.repeat(x, 2, axis=a)
    return x


def upsample2x_bwd(gy, is3d, dtype):
    """sum of the 4 | 8 fine cells of a coarse cell, (dz, dy, dx) ascending from +0."""
    T = _t(dtype)
    gy = np.asarray(gy).astype(T)
    B, D2, H2, W2, C = gy.shape
    acc = np.zeros((B, D2 // 2 if is3d else 1, H2 // 2, W2 // 2, C), T)
    for dz in ((0, 1) if is3d else (0,)):
        for dy in (0, 1):
            for dx in (0, 1):
                acc = acc + (gy[:, dz::2, dy::2, dx::2] if is3d else gy[:, :, dy::2, dx::2])
    return acc


def add_up2x(a, bc, is3d, dtype):
    T = _t(dtype)
    return np.asarray(a).astype(T) + upsample2x(np.asarray(bc).astype(T), is3d)


def dilate2_odd(g, is3d):
    """out[2o+1] = g[o] on every spatial axis, +0.0 elsewhere."""
    g = np.asarray(g)
    B, D, H, W, C = g.shape
    out = np.zeros((B, 2 * D if is3d else 1, 2 * H, 2 * W, C), g.dtype)
    if is3d:
        out[:, 1::2, 1::2, 1::2] = g
    else:
        out[:, :, 1::2, 1::2] = g
    return out


def lrelu_bwd_pool2x(dy, y, leak, is3d, dtype):
    return lrelu_bwd(dy, y, leak, dtype), upsample2x_bwd(dy, is3d, dtype)


def fine_shape(cshape, is3d):
    B, D, H, W, C = cshape
    return (B, 2 * D if is3d else 1, 2 * H, 2 * W, C)


# ---- concat ---------------------------------------------------------------------------------------------------------------------------
def concat2(a, b):
    return np.concatenate([a, b], axis=1)


def concat2_bwd(gy, Ca):
    return gy[:, :Ca].copy(), gy[:, Ca:].copy()


# ---- column sums ----------------------------------------------------------------------------------------------------------------------
def colsum(g, dtype):
    """float64: plain.  float32: fp32 partials of 512 consecutive rows each, added row by row; the partials are summed in double."""
    g = np.asarray(g)
    if _t(dtype) is F64:
        return g.astype(F64).sum(axis=0)
    rows, C = g.shape
    nb = -(-rows // K_COLSUM_ROWS)
    gp = np.zeros((nb * K_COLSUM_ROWS, C), F32)
    gp[:rows] = g
    gp = gp.reshape(nb, K_COLSUM_ROWS, C)
    acc = np.zeros((nb, C), F32)
    for r in range(K_COLSUM_ROWS):
        acc = acc + gp[:, r]
    return acc.astype(F64).sum(axis=0).astype(F32)


# ---- fully connected ------------------------------------------------------------------------------------------------------------------
def linear_family(B, K, N):
    return "splitk" if (N <= 32 and K >= 1024) else "tinyk"


def _fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def linear(x, w, b, dtype):
    x, w = np.asarray(x), np.asarray(w)
    if _t(dtype) is F64:
        y = x.astype(F64) @ w.astype(F64)
        return y + np.asarray(b, F64) if b is not None else y
    B, K = x.shape
    N = w.shape[1]
    if linear_family(B, K, N) == "tinyk":                  # linear_fwd_kernel: fmaf over k ascending, then the bias
        acc = np.zeros((B, N), F32)
        for k in range(K):
            acc = _fma32(x[:, k, None], w[k][None, :], acc)
        return acc + b if b is not None else acc
    # linear_splitk_kernel: chunk of 2048 rows of w; thread t takes rows t, t+256, .. (8 fmaf), 64-lane shuffle tree (6 adds), 4 waves in
    # order (4 adds); linear_splitk_final_kernel: the chunks in double, rounded, plus the bias
    nch = -(-K // K_FC_CHUNK)
    xp = np.zeros((B, nch * K_FC_CHUNK), F32); xp[:, :K] = x
    wp = np.zeros((nch * K_FC_CHUNK, N), F32); wp[:K] = w
    xr = xp.reshape(B, nch, K_FC_CHUNK // K_THREADS, K_THREADS)
    wr = wp.reshape(nch, K_FC_CHUNK // K_THREADS, K_THREADS, N)
    acc = np.zeros((B, nch, K_THREADS, N), F32)
    for j in range(K_FC_CHUNK // K_THREADS):
        acc = _fma32(xr[:, :, j, :, None], wr[None, :, j], acc)
    v = acc.reshape(B, nch, K_THREADS // 64, 64, N).copy()
    off = 32
    while off:
        v[:, :, :, :off] = v[:, :, :, :off] + v[:, :, :, off:2 * off]
        off >>= 1
    r = np.zeros((B, nch, N), F32)
    for q in range(K_THREADS // 64):
        r = r + v[:, :, q, 0]
    y = r.astype(F64).sum(axis=1).astype(F32)
    return y + b if b is not None else y


def linear_bwd(x, w, gy, dtype):
    """(gx, gw, gb).  float32: gw and gb run over b ascending (fmaf / add); gx is a double dot product rounded once in the tiny-K family
    (linear_bwd_x_kernel) and an fmaf chain over n ascending in the small-N one (linear_bwd_smalln_kernel)."""
    x, w, gy = np.asarray(x), np.asarray(w), np.asarray(gy)
    if _t(dtype) is F64:
        x, w, gy = x.astype(F64), w.astype(F64), gy.astype(F64)
        return gy @ w.T, x.T @ gy, gy.sum(axis=0)
    B, K = x.shape
    N = w.shape[1]
    gw = np.zeros((K, N), F32); gb = np.zeros(N, F32)
    for b in range(B):
        gw = _fma32(x[b][:, None], gy[b][None, :], gw)
        gb = gb + gy[b]
    if linear_family(B, K, N) == "tinyk":
        gx = (gy.astype(F64) @ w.astype(F64).T).astype(F32)
    else:
        gx = np.zeros((B, K), F32)
        for n in range(N):
            gx = _fma32(gy[:, n][:, None], w[:, n][None, :], gx)
    return gx, gw, gb


def linear_chain(B, K, N):
    """L per output: the longest sequential fp32 chain of the kernel that writes it, read from the source.  y: K fmaf + the bias add (tiny
    K); 8 fmaf + 6 shuffle adds + 4 wave adds (split-K; the chunk sum is in double).  gw, gb: B steps over the batch.  gx: one rounding of a
    double dot product (tiny K), N fmaf (small N)."""
    if linear_family(B, K, N) == "tinyk":
        return {"y": K + 1, "gx": 1, "gw": B, "gb": B}
    return {"y": 8 + 6 + 4, "gx": N, "gw": B, "gb": B}


def linear_abs_terms(x, w, b, gy):
    """sum of |terms| of every output of forward and backward: the condition of exactness on integer data and the scale of the a-priori
    rounding bound on random data."""
    ax, aw, ag = np.abs(np.asarray(x, F64)), np.abs(np.asarray(w, F64)), np.abs(np.asarray(gy, F64))
    return {"y": ax @ aw + (np.abs(np.asarray(b, F64)) if b is not None else 0.0), "gx": ag @ aw.T, "gw": ax.T @ ag, "gb": ag.sum(axis=0)}


def chain_bound(L, nterms, abs_terms):
    """|fp32 evaluation - exact| <= (L * 2^-24 + nterms * 2^-53) * sum|terms| for a sum whose longest sequential fp32 chain has L
    roundings; the second term covers the stages the kernels run in double."""
    return (L * U + nterms * 2.0 ** -53) * np.asarray(abs_terms, F64)


# ---- the rule of the rounding-bounded comparisons ---------------------------------------------------------------------------------------
def bounded(got, ref64, twin32):
    """3 * e32 + floor rule on every cell.  Where the fp64 reference overflows fp32 the result must be that infinity; elsewhere it must be
    finite-or-not exactly as fp32 allows (never NaN) and within the bound.  Returns dict(e32, err, bound, bitwise); raises AssertionError."""
    got = np.asarray(got); ref64 = np.asarray(ref64, F64); twin32 = np.asarray(twin32)
    assert got.shape == ref64.shape == twin32.shape, (got.shape, ref64.shape, twin32.shape)
    assert not np.isnan(ref64).any()
    with _quiet():
        r32 = ref64.astype(F32)
    over = np.isinf(r32)
    assert np.array_equal(got[over], r32[over]), "the fp64 reference overflows fp32 here: the same infinity is required"
    fin = ~over
    res = {"bitwise": bool(np.array_equal(got, twin32, equal_nan=True)), "e32": 0.0, "err": 0.0, "bound": 0.0}
    if fin.any():
        assert not np.isnan(got[fin]).any(), "NaN where the reference is finite"
        e32 = float(np.abs(twin32[fin].astype(F64) - ref64[fin]).max())
        floor = float(np.spacing(F32(np.abs(ref64[fin]).max())))
        err = float(np.abs(got[fin].astype(F64) - ref64[fin]).max())
        res.update(e32=e32, err=err, bound=3.0 * e32 + floor)
        assert err <= res["bound"], "error %.3e above 3 * e32 + floor = %.3e (e32 %.3e)" % (err, res["bound"], e32)
    return res


def fmt(name, r):
    ratio = r["err"] / r["bound"] if r["bound"] > 0 else 0.0
    return "%-44s e32 %.3e  kernel %.3e  bound %.3e  ratio %.3f  bitwise %s" % (name, r["e32"], r["err"], r["bound"], ratio, "yes" if r["bitwise"] else "no")


# ---- seeded inputs and case tables -----------------------------------------------------------------------------------------------------
def ints(rng, shape):
    """integers in [-4, 4] stored as fp32"""
    return rng.randint(-4, 5, size=shape).astype(F32)


def uni(rng, shape, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, size=shape).astype(F32)


ADAM_SIZES = (1, 255, 256, 257, WRAP, WRAP + 1, 2 * WRAP + 5)
ADAM_HYPER = dict(b1=float(F32(0.5)), b2=float(F32(0.999)), eps=float(F32(1e-8)))      # the fp32 values the kernel receives


def adam_lr_t(t, lr=1e-4, b1=0.5, b2=0.999):
    return float(F32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


@functools.lru_cache(maxsize=None)
def adam_inputs(n, first_step=False):
    """p, g, m, v; every 7th element has g = 0 and v = 0, so that its denominator is eps alone, and m of the order of eps, so that the
    step stays of the order of lr_t and does not widen the bound of the other elements; first_step: m = v = 0 (t = 1)."""
    rng = np.random.RandomState(1000 + n % 9973 + (1 if first_step else 0))
    p, g = uni(rng, n), uni(rng, n)
    m, v = uni(rng, n, -0.1, 0.1), uni(rng, n, 0.0, 0.1)
    g[::7] = 0.0; v[::7] = 0.0; m[::7] *= F32(1e-7)
    if first_step:
        m[:] = 0.0; v[:] = 0.0
    return frozen(p, g, m, v)


ADAM_EXTREME_G = (1e-20, -1e-20, 1e18, -1e18)


@functools.lru_cache(maxsize=None)
def adam_extreme_inputs(first_step):
    """n = 257; elements 3, 64, 130, 256 carry g = +-1e-20, +-1e18; element 10 has g = v = 0 with m = 0.1: a step of lr_t * b1 * m / eps
    (unless first_step zeroes m).  Returns (p, g, m, v, plain) with plain = the other elements, which the rule is applied to once more on
    their own: the large values must not widen their bound."""
    p, g, m, v = (a.copy() for a in adam_inputs(257, first_step))
    idx = np.array([3, 64, 130, 256])
    g[idx] = np.array(ADAM_EXTREME_G, F32)
    g[10] = 0.0; v[10] = 0.0
    if not first_step:
        m[10] = 0.1
    plain = np.ones(257, bool); plain[idx] = False; plain[10] = False
    return frozen(p, g, m, v, plain)


LINEAR_TINYK = ((1, 1, 1), (5, 3, 1000), (2, 16, 257), (3, 16, WRAP + 1), (2, 1023, 16), (2, 2048, 33))
LINEAR_SPLITK = ((1, 1024, 1), (3, 1024, 16), (2, 2049, 17), (4, 4096, 32), (2, 6143, 5), (1, WRAP + 300, 16))


@functools.lru_cache(maxsize=None)
def linear_inputs(B, K, N, integer):
    rng = np.random.RandomState((B * 31 + K * 7 + N) % 100003 + (0 if integer else 1))
    f = ints if integer else uni
    return frozen(f(rng, (B, K)), f(rng, (K, N)), f(rng, N), f(rng, (B, N)))


COLSUM_SHAPES = ((1, 1), (511, 3), (512, 3), (513, 128), (1025, 300), (5000, 257), (3, 1024))
COLSUM_RANDOM = (5000, 128)
COLSUM_CHAIN = K_COLSUM_ROWS


@functools.lru_cache(maxsize=None)
def colsum_input(rows, C, integer):
    rng = np.random.RandomState(rows * 13 + C + (0 if integer else 1))
    return frozen((ints if integer else uni)(rng, (rows, C)))[0]


KL_CASES = ((1, 16, 16), (4, 16, 16), (8, 16, 5), (3, 300, 300), (2, 513, 257), (5, 7, 0))      # (B, ncol, n)
KL_RHOS = (float(F32(0.05)), 0.5)
KL_GOUT = 1.75


@functools.lru_cache(maxsize=None)
def kl_input(B, ncol):
    rng = np.random.RandomState(B * 1000 + ncol)
    z = sigmoid(uni(rng, (B, ncol), -3.0, 3.0), F32)
    return frozen(z)[0]


@functools.lru_cache(maxsize=None)
def kl_extreme_input():
    """[4, 16] of constant columns: means 1e-6 (even columns) and 1 - 1e-6 (odd ones), exact because every row is the same fp32 value."""
    z = np.empty((4, 16), F32)
    z[:, 0::2] = F32(1e-6); z[:, 1::2] = F32(1.0 - 1e-6)
    return frozen(z)[0]


SIGMOID_SIZES = (1, 257, WRAP + 1)
SIGMOID_SPECIAL = (0.0, 16.6, -16.6, 17.0, -17.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e30, -1e30)


@functools.lru_cache(maxsize=None)
def sigmoid_inputs(n):
    """x, gy: random in (-3, 3) with the special values spread over it (n = 1: x = 0 only; see sigmoid_special_input)."""
    rng = np.random.RandomState(n)
    x, gy = uni(rng, n, -3.0, 3.0), uni(rng, n)
    if n >= 257:
        pos = np.linspace(0, n - 1, len(SIGMOID_SPECIAL)).astype(np.int64)
        x[pos] = np.array(SIGMOID_SPECIAL, F32)
    else:
        x[0] = 0.0
    return frozen(x, gy)


MEAN_SIZES = (1, 3, 4, 255, 257, 4097, 4 * WRAP + 3)


@functools.lru_cache(maxsize=None)
def mean_inputs(n, integer):
    """a, b with exact ties a == b planted in the float4 body (element 1, and one in the last float4) and in the scalar tail (the last
    element when n % 4 != 0).  Integer data: a in [-4, 4], b = clip(a + {-2..2}, -4, 4): |a-b| <= 2, so that n * 4 stays below 2^24."""
    rng = np.random.RandomState(n % 65521 + (0 if integer else 7))
    if integer:
        a = ints(rng, n)
        b = np.clip(a + rng.randint(-2, 3, size=n).astype(F32), -4, 4).astype(F32)
    else:
        a, b = uni(rng, n), uni(rng, n)
    body = 4 * (n // 4)
    for i in (1, body - 2):
        if 0 <= i < body:
            b[i] = a[i]
    if n % 4:
        b[n - 1] = a[n - 1]
    return frozen(a, b)


EW_SIZES = (1, 3, 5, 1003, K_EW_TILE - 1, K_EW_TILE, K_EW_TILE + 1, 3 * K_EW_TILE + 7, 4 * K_EW_TILE + 3, 1 << 20)
EW_LEAKS = (0.2, 0.0)

# coarse shapes (B, D, H, W, C); the 2-D kernels take them with D = 1
UP_SHAPES_3D = ((1, 1, 1, 1, 4), (2, 1, 3, 5, 4), (1, 3, 5, 7, 12), (1, 2, 2, 2, 128))
UP_SHAPES_2D = ((1, 1, 1, 1, 4), (2, 1, 3, 5, 4), (1, 1, 5, 7, 12), (1, 1, 2, 2, 128))
UP_WRAP_SRC = {True: (1, 8, 16, 33, 512), False: (2, 1, 64, 33, 512)}       # 540672 source float4: upsample fwd / bwd wrap
UP_WRAP_DST = {True: (1, 4, 8, 17, 512), False: (2, 1, 32, 17, 512)}        # 557056 destination float4: add_up2x / dilate2_odd wrap

CONCAT_CASES = ((1, 4, 4), (30, 8, 12), (7, 2, 1), (5, 3, 3), (9, 1, 4), (WRAP + 1, 4, 4), (3, 128, 64))      # (rows, Ca, Cb)
CONCAT_UNALIGNED = (6, 4, 8)      # float4-eligible extents; the b operand starts one float into its buffer
