"""The staged (x,y,z) weight gradient (conv_wgrad.hip::wgrad_wxyz_staged_kernel: operands fetched and combined once per workgroup, kept in
LDS), the default of the 128 -> 128 layers at W = 64 | 32, against the fp64 oracle and against the kernel it replaced (wgrad_algo = 4).

Bound against algo 4: the staged kernel applies the same (xi_z, xi_y) combination in the same operation order, feeds the same MFMA
sequence and writes the same partial layout, so the two must agree BIT FOR BIT -- asserted with torch.equal, which also makes both sit at
the same distance from the oracle (asserted for both with the suite's TOL)."""
import re
import subprocess

import numpy as np
import pytest
import torch

from deep_fluids_amd import _lib

TOL = 2e-5      # tests/test_gpu_layers.py::TOL


def _inputs(shape, cin, cout, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, shape + (cin,)).astype(np.float32)
    x = np.where(x > 0, x, 0.2 * x).astype(np.float32)      # lrelu-distributed input
    g = rng.uniform(-1, 1, shape + (cout,)).astype(np.float32)
    return x, g


def _wgrad(x, g, algo, bias=True):
    """df_conv_wgrad_algo on device tensors; gw / gb start as NaN so that an element the kernels leave out shows."""
    from deep_fluids_amd._lib import call, query
    from deep_fluids_amd.ops import _ptr, _stream
    B, D, H, W, cin = x.shape
    cout = g.shape[-1]
    nb = query("df_conv_wgrad_workspace_bytes", B, D, H, W, cin, cout, 3)
    ws = torch.empty((nb + 3) // 4, device="cuda")
    gw = torch.full((27, cin, cout), float("nan"), device="cuda")
    gb = torch.full((cout,), float("nan"), device="cuda") if bias else None
    call("df_conv_wgrad_algo", _ptr(x), _ptr(g), _ptr(gw), _ptr(gb) if bias else None, B, D, H, W, cin, cout, 3, _ptr(ws), nb, algo, _stream())
    torch.cuda.synchronize()
    return gw, gb


def _oracle(x, g):
    import df_oracle as orc
    cin, cout = x.shape[-1], g.shape[-1]
    _, dw, db = orc.conv_same_bwd(x.astype(np.float64), np.zeros((3, 3, 3, cin, cout)), g.astype(np.float64), need_dx=False)
    return dw.reshape(27, cin, cout), db


# shape, Cin, Cout, bias gradient, partial-range override (0: the default count)
CASES = [
    ((1, 4, 4, 32), 128, 128, True, 0),       # D = H = 4: every row touches the SAME padding; W = 32
    ((2, 6, 4, 64), 128, 128, False, 0),      # W = 64, H = 4, no bias gradient
    ((1, 6, 6, 32), 128, 128, True, 0),       # 9 tile rows: the last pair has one live tile row
    ((3, 6, 10, 64), 128, 128, True, 0),      # 45 tile rows, three batches, W = 64
    ((3, 4, 6, 32), 128, 128, False, 0),
    ((2, 16, 24, 32), 128, 128, True, 7),     # 96 tile-row pairs over 7 ranges of 14: a tail range of 12
    ((1, 8, 20, 64), 128, 128, True, 3),      # 20 pairs over 3 ranges of 7: a tail range of 6
    ((1, 4, 4, 32), 96, 128, True, 0),        # channels short of the 128 padding: the forms of the other layers
    ((2, 4, 6, 64), 128, 96, False, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cin,cout,bias,ranges", CASES)
def test_staged_wgrad_vs_oracle_and_previous_kernel(shape, cin, cout, bias, ranges):
    from gpu_util import dev, host, rel_linf
    x, g = _inputs(shape, cin, cout, seed=sum(shape) + cin + 3 * cout + ranges)
    dw, db = _oracle(x, g)
    xt, gt = dev(x), dev(g)
    gw0, gb0 = _wgrad(xt, gt, 0 | (ranges << 3), bias)
    gw4, gb4 = _wgrad(xt, gt, 4 | (ranges << 3), bias)
    e0, e4 = rel_linf(host(gw0), dw), rel_linf(host(gw4), dw)
    print("gW rel L-inf vs fp64 oracle: default %.3e, algo 4 %.3e" % (e0, e4))
    assert e0 < TOL and e4 < TOL, (e0, e4)
    if bias:
        b0, b4 = rel_linf(host(gb0), db), rel_linf(host(gb4), db)
        print("gb rel L-inf vs fp64 oracle: default %.3e, algo 4 %.3e" % (b0, b4))
        assert b0 < TOL and b4 < TOL, (b0, b4)
    if cin == 128 and cout == 128:      # the staged kernel against the one it replaced: the same bits
        assert torch.equal(gw0, gw4)
        assert not bias or torch.equal(gb0, gb4)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 6, 10, 64), (3, 8, 6, 32)])
def test_staged_wgrad_is_bitwise_reproducible(shape):
    from gpu_util import dev
    x, g = _inputs(shape, 128, 128, seed=11 + sum(shape))
    xt, gt = dev(x), dev(g)
    runs = [_wgrad(xt, gt, 0) for _ in range(3)]
    assert not torch.isnan(runs[0][0]).any() and not torch.isnan(runs[0][1]).any()
    for gw, gb in runs[1:]:
        assert torch.equal(gw, runs[0][0]) and torch.equal(gb, runs[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 12, 64), (1, 16, 24, 32)])
def test_staged_wgrad_form_and_workspace_contract(shape):
    """df_conv_wgrad_form keeps reporting 3 for the (x,y,z) family; a workspace of exactly df_conv_wgrad_workspace_bytes is enough, one
    byte less is DF_EWORKSPACE (-4) before anything is launched."""
    from deep_fluids_amd.ops import _ptr, _stream
    from gpu_util import dev
    B, D, H, W = shape
    C = 128
    assert _lib.query("df_conv_wgrad_form", B, D, H, W, C, C, 3, 0) == 3
    assert _lib.query("df_conv_wgrad_form", B, D, H, W, C, C, 3, 4) == 3
    nb = _lib.query("df_conv_wgrad_workspace_bytes", B, D, H, W, C, C, 3)
    x, g = _inputs(shape, C, C, seed=5)
    xt, gt = dev(x), dev(g)
    ref, _ = _wgrad(xt, gt, 4)
    # exactly nb bytes, with a guard behind them that must stay untouched
    buf = torch.zeros(nb + 4096, dtype=torch.uint8, device="cuda")
    buf[nb:] = 0xA5
    h = _lib.lib()
    gw = torch.full((27, C, C), float("nan"), device="cuda")
    gb = torch.full((C,), float("nan"), device="cuda")
    assert h.df_conv_wgrad_algo(_ptr(xt), _ptr(gt), _ptr(gw), _ptr(gb), B, D, H, W, C, C, 3, _ptr(buf), nb, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gw, ref)
    assert bool((buf[nb:] == 0xA5).all())
    gw.fill_(float("nan")); gb.fill_(float("nan"))
    assert h.df_conv_wgrad_algo(_ptr(xt), _ptr(gt), _ptr(gw), _ptr(gb), B, D, H, W, C, C, 3, _ptr(buf), nb - 1, 0, _stream()) == -4
    assert b"workspace too small" in h.df_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(gw).all()) and bool(torch.isnan(gb).all())


def test_release_library_holds_only_the_production_staged_instantiations():
    """wgrad_wxyz_staged_kernel<WP8> exists for the row lengths the 128 -> 128 layers of the benchmarked generator run at (W = 8 WP8 = 64 | 32)
    and carries no experiment switch: the shipped library holds exactly these two, and exports no tuning entry point."""
    out = subprocess.check_output(["nm", "-C", _lib.LIB_PATH]).decode()
    got = sorted(set(int(v) for v in re.findall(r"wgrad_wxyz_staged_kernel<(\d+)>", out)))
    assert got == [4, 8], got
    assert not re.findall(r"wgrad_wxyz_staged_kernel<[^>]*,", out)
    assert "df_debug_" not in out
