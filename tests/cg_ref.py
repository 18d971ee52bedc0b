"""The reductions of the conjugate-gradient iteration in the order include/deepfluids_hip.h states (block 3 of the smoke section), restated
once: a workgroup is 256 consecutive cells of ONE batch entry; inside it an xor butterfly over the 64 lanes of a wave (offsets 32, 16, ..,
1), then the four wave results in ascending order; the nblk partials of an entry are combined by 256 strided running sums (thread t takes
partials t, t + 256, .. ascending, from +0) and the same tree.  No fused multiply-add anywhere.  NumPy only, parametrised by dtype:
float32 makes the cg() / pcg() restatements of smoke_ref, smoke_obs_ref, smoke_open_ref, liquid_ref, liquid_gf_ref, diffuse_ref and
smoke_mg_ref (``dot=`` and ``amax=``) the bit-for-bit twin of cg_direction_kernel / cg_update_kernel; every intermediate keeps the dtype,
which is asserted.

The butterfly: lane L adds the value of lane L ^ m to its own; a + b == b + a bit for bit, so every lane ends with the same bits and
lane 0's value is the half tree v[:m] + v[m:2m] that ``_tree`` writes (the shape of _tree / _waves in field_metrics_ref.py).  Cells
that do not count hold +0: a running sum here starts at +0 and never becomes -0 (x + -x rounds to +0), so such a term changes no bit.

``partials=`` and ``combine=`` of ordered_dot exist for tests/cg_cases.py, which swaps in wrong orders to show that a row tells them
apart."""
import numpy as np

K_THREADS = 256
WAVE = 64


def _type(dtype):
    return np.dtype(dtype).type


def _add(a, b):
    return a + b


def _tree(v, op=_add):
    """[..., 64] -> [...]: lane 0 of the xor butterfly with offsets 32, 16, .., 1"""
    v = v.copy()
    off = WAVE // 2
    while off > 0:
        v[..., :off] = op(v[..., :off], v[..., off:2 * off])
        off //= 2
    return v[..., 0]


def _waves(v, op=_add):
    """[..., 256] -> [...]: the tree inside each wave, then the four wave results in ascending order"""
    w = _tree(v.reshape(v.shape[:-1] + (K_THREADS // WAVE, WAVE)), op)
    acc = w[..., 0]
    for k in range(1, K_THREADS // WAVE):
        acc = op(acc, w[..., k])
    return acc


def _padded(v, dtype):
    """[E, n] -> [E, ceil(n / 256), 256] with +0 behind the last cell"""
    v = np.asarray(v)
    assert v.ndim == 2 and v.dtype == np.dtype(dtype), (v.shape, v.dtype)
    E, n = v.shape
    nblk = -(-n // K_THREADS)
    p = np.zeros((E, nblk * K_THREADS), dtype)
    p[:, :n] = v
    return p.reshape(E, nblk, K_THREADS)


def block_partials(v, dtype, op=_add, waves=_waves):
    """v [E, n] in ``dtype`` with 0 at the cells that do not count -> [E, nblk]: workgroup j reduces cells 256 j .. 256 j + 255"""
    out = waves(_padded(v, dtype), op)
    assert out.dtype == np.dtype(dtype)
    return out


def _strided(partials, dtype, op):
    """thread t: partials t, t + 256, .. ascending from +0 -> [E, 256]"""
    p = _padded(partials, dtype)                                     # [E, trips, 256]
    a = np.zeros((p.shape[0], K_THREADS), dtype)
    for i in range(p.shape[1]):
        a = op(a, p[:, i])
    assert a.dtype == np.dtype(dtype)
    return a


def entry_sum(partials, dtype):
    """[E, nblk] -> [E]: the 256 strided running sums, then the tree"""
    out = _waves(_strided(partials, dtype, _add))
    assert out.dtype == np.dtype(dtype)
    return out


def entry_max(partials):
    """the same with fmaxf from 0 (the partials are maxima of |r|: no NaN, no -0)"""
    out = _waves(_strided(partials, partials.dtype, np.maximum), np.maximum)
    assert out.dtype == partials.dtype
    return out


def ordered_dot(a, b, dtype=None, partials=block_partials, combine=entry_sum):
    """a, b [E, ...] -> [E]: the products cell by cell, then the header's order.  ``dtype`` defaults to a's."""
    dtype = a.dtype if dtype is None else np.dtype(dtype)
    assert a.dtype == dtype and b.dtype == dtype, (a.dtype, b.dtype, dtype)
    prod = (a * b).reshape(a.shape[0], -1)
    assert prod.dtype == dtype
    return combine(partials(prod, dtype), dtype)


def ordered_amax(r):
    """r [E, ...] -> [E]: max|r| through the same workgroups"""
    v = np.abs(r).reshape(r.shape[0], -1)
    return entry_max(block_partials(v, v.dtype, np.maximum))


# ---- what the restatements default to: NumPy's own reductions (pairwise sums), the values every earlier test was written against ----------
def numpy_dot(a, b):
    return (a * b).reshape(a.shape[0], -1).sum(axis=1, dtype=a.dtype)


def numpy_amax(r):
    return np.abs(r).reshape(r.shape[0], -1).max(axis=1)
