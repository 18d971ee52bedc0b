"""-m gpu: every conjugate-gradient solve -- closed, obstacle flags, open sides, both, liquid, ghost fluid, diffusion, multigrid (closed,
flags, open) -- through the raw C ABI, one row of tests/cg_cases.py per (variant, grid), from one workgroup per entry to 519: past 256
entry_reduce's loop takes a second and a third trip, and an entry's workgroups straddle the XCD chunks of the block remap.
tests/test_cg_cases_host.py keeps the conditions on the rows without a GPU.

Harness: every operand, the output, the status words, the workspace (exactly ``df_*_workspace_bytes`` long) and the multigrid hierarchy
are guarded buffers (gpu_util.Guarded / GuardedBytes / GuardedInts) that hold the fill before the first call: nothing is read before it
is written, nothing behind a buffer is written.  Per row: init, then direction(k) / update(k) for k < K with accuracy 0 and
max_iter = K, status, and the correction (diffusion: finish).

Reference: the fp32 twin, the variant's own cg() / pcg() restatement with the reductions of tests/cg_ref.py in the header's order.  The
assertion is equality of bits -- pressure (diffusion: the finished velocity), corrected velocity, iterations, active_count.  The fp64
run of the same restatement stays as a second, loose witness under the suite's standing rule, distance <= 3 * e32 + 1e-7 with e32 the
twin's.  Also: a frozen entry's pressure stays as init left it; two more direction / update pairs after every entry froze change no
bit; one row per variant solves to the default accuracy with max_iter from the twin.  profiles/cg_edge_tests.md holds the record."""
import numpy as np
import pytest
import torch

import cg_cases as cc
import smoke_mg_ref as mg
from gpu_util import Guarded, GuardedBytes, GuardedInts, host

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def k():
    """(library handle, stream)"""
    from deep_fluids_amd import _lib
    from deep_fluids_amd.ops import _stream
    return _lib.lib(), _stream()


class Solve(object):
    """the guarded buffers of one row and its entry points by kind"""

    def __init__(self, k, r, solve=False):
        self.lib, stream = k
        self.r, self.ep = r, cc.entry_points(r)
        i = cc.inputs(r["name"], solve)
        shape, B = r["shape"], r["B"]
        nd = len(shape)
        self.full = (B,) + shape
        self.s = dict(dim=nd, B=B, S=cc.systems(r), Z=shape[0] if nd == 3 else 1, Y=shape[-2], X=shape[-1], bnd=r["bnd"], os=i["bits"], k=0,
                      acc=0.0, max_iter=0, gf_clamp=cc.GF_CLAMP, mg_alpha=mg.ALPHA, stream=stream)
        self.s["ws_bytes"] = self.query("bytes")
        assert self.s["ws_bytes"] > 0 and self.s["ws_bytes"] % 4 == 0
        self.b = dict(vel=Guarded(self.full + (nd,), i["vel"]), out=Guarded(self.full + (nd,)), ws=Guarded((self.s["ws_bytes"] // 4,)),
                      count=GuardedInts((1,)), iters=GuardedInts((self.s["S"],)))
        if r["variant"] != "diffuse":
            self.b["pressure"] = Guarded(self.full)
        if "flags" in i:
            self.b["flags"] = GuardedBytes(self.full, i["flags"])
        if r["variant"] == "gf":
            self.b["phi"] = Guarded(self.full, i["phi"])
        if r["variant"] == "diffuse":
            self.b["alpha"] = Guarded((B,), i["alpha"])
        if "hier_bytes" in self.ep:
            self.s["hier_bytes"] = self.query("hier_bytes")
            assert self.s["hier_bytes"] > 0 and self.s["hier_bytes"] % 4 == 0
            self.b["hier"] = Guarded((self.s["hier_bytes"] // 4,))

    def _args(self, kind, over):
        out = []
        for a in self.ep[kind][1]:
            if a in over:
                out.append(over[a])
            elif a in cc.POINTERS:
                out.append(self.b[a].ptr if a in self.b else None)
            else:
                out.append(self.s[a])
        return out

    def query(self, kind):
        return int(getattr(self.lib, self.ep[kind][0])(*self._args(kind, {})))

    def rc(self, kind, **over):
        return getattr(self.lib, self.ep[kind][0])(*self._args(kind, over))

    def call(self, kind, **over):
        rc = self.rc(kind, **over)
        assert rc == 0, (self.r["name"], self.ep[kind][0], rc, self.lib.df_last_error())

    def guards(self, what):
        torch.cuda.synchronize()
        for n, b in self.b.items():
            b.check_guards("%s %s %s" % (self.r["name"], what, n))

    # ---- the sequence ----
    def init(self):
        if "build" in self.ep:
            self.call("build")
        self.call("init")
        if "precondition" in self.ep:
            self.call("precondition", k=-1)

    def iterate(self, k, acc, max_iter):
        self.call("direction", k=k, acc=acc, max_iter=max_iter)
        self.call("update", k=k)
        if "precondition" in self.ep:
            self.call("precondition", k=k)

    def status(self, k):
        """(active_count, iterations) as direction(k) left them"""
        self.b["count"].refill(); self.b["iters"].refill()
        self.call("status", k=k)
        torch.cuda.synchronize()
        it = self.b["iters"].get("iterations")
        return int(self.b["count"].get("active_count")[0]), (it.reshape(self.r["B"], -1) if self.r["variant"] == "diffuse" else it)

    def field(self):
        """the pressure's words (diffusion: the finished velocity's)"""
        if self.r["variant"] == "diffuse":
            return self.velocity()
        torch.cuda.synchronize()
        return self.b["pressure"].get("pressure").view(np.int32).copy()

    def velocity(self):
        self.b["out"].refill()
        self.call("finish" if self.r["variant"] == "diffuse" else "correct")
        torch.cuda.synchronize()
        return self.b["out"].get("velocity").view(np.int32).copy()


def _same(name, what, got, want):
    want = np.ascontiguousarray(want, F32).view(np.int32)
    assert got.shape == want.shape, (name, what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError("%s %s: %d of %d words differ, first at %s: got %r, want %r" % (
            name, what, int(bad.sum()), bad.size, at, got.view(F32)[at], want.view(F32)[at]))


def _want_field(r, t):
    return t["out"] if r["variant"] == "diffuse" else t["x"]


@pytest.mark.parametrize("name", cc.names())
def test_row(k, name):
    r = cc.BY_NAME[name]
    s = Solve(k, r)
    K = max(r["ks"])
    s.init()
    s.guards("init")
    first = None if r["variant"] == "diffuse" else s.field()
    if first is not None:
        assert not first.any(), "%s: init leaves p = +0" % name
    got = None
    for kk in range(K):
        s.iterate(kk, 0.0, K)
        if kk + 1 in r["ks"]:
            t = cc.twin(name, kk + 1)
            got = s.field()
            _same(name, "field after %d iterations" % (kk + 1), got, _want_field(r, t))
            count, iters = s.status(kk)
            assert np.array_equal(iters, t["iters"]), (name, kk + 1, iters.tolist(), t["iters"].tolist())
            assert count == int((np.asarray(t["iters"]) == kk + 1).sum()), (name, kk + 1, count)
            if first is not None:                                      # the entry at rest: its pressure as init left it
                assert not got[1].any()
    t = cc.twin(name, K)
    vel = s.velocity()
    _same(name, "velocity", vel, t["out"])
    # the fp64 run of the same restatement, NumPy's reductions: the loose witness
    import cg_ref
    t64 = cc.run(name, K, dtype=np.float64, dot=cg_ref.numpy_dot, amax=cg_ref.numpy_amax)
    w32, w64 = np.asarray(_want_field(r, t), np.float64), np.asarray(_want_field(r, t64), np.float64)
    e32, d = float(np.abs(w32 - w64).max()), float(np.abs(got.view(F32).astype(np.float64) - w64).max())
    print("%-28s K %d  e32 %.3e  gpu-f64 %.3e  bound %.3e" % (name, K, e32, d, 3 * e32 + 1e-7))
    assert d <= 3 * e32 + 1e-7, (name, d, e32)
    # two more direction / update pairs after every entry froze (max_iter reached, or earlier): no bit moves
    for kk in (K, K + 1):
        s.iterate(kk, 0.0, K)
    count, iters = s.status(K + 1)
    assert count == 0 and np.array_equal(iters, t["iters"]), (name, count, iters.tolist())
    assert np.array_equal(s.field(), got), "%s: calls after the last entry froze changed the field" % name
    assert np.array_equal(s.velocity(), vel)
    s.guards("end")
    assert np.array_equal(host(s.b["vel"].payload()).reshape(-1).view(np.int32), cc.inputs(name)["vel"].reshape(-1).view(np.int32))


@pytest.mark.parametrize("name", cc.names(solve=True))
def test_solve_to_the_default_accuracy(k, name):
    r = cc.BY_NAME[name]
    t = cc.twin(name, None, solve=True)
    max_iter = int(np.max(t["iters"]))
    s = Solve(k, r, solve=True)
    s.init()
    for kk in range(max_iter + 2):                                     # two calls more than any entry needs
        s.iterate(kk, cc.ACCURACY, max_iter)
    count, iters = s.status(max_iter + 1)
    print("%-28s iterations %s (twin %s)" % (name, iters.tolist(), np.asarray(t["iters"]).tolist()))
    assert count == 0 and np.array_equal(iters, t["iters"]), (name, count, iters.tolist(), np.asarray(t["iters"]).tolist())
    _same(name, "field", s.field(), _want_field(r, t))
    _same(name, "velocity", s.velocity(), t["out"])
    s.guards("end")


# ---- refusals: the shared checks answer the same way at every entry point -------------------------------------------------------------------
def _refusal_rows():
    seen, out = set(), []
    for r in cc.ROWS:
        key = (r["variant"], len(r["shape"]))
        if cc.nblk(r) <= 2 and key not in seen:
            seen.add(key)
            out.append(r["name"])
    return out


@pytest.mark.parametrize("name", _refusal_rows())
def test_refusals(k, name):
    from deep_fluids_amd import _lib
    r = cc.BY_NAME[name]
    s = Solve(k, r)
    nd = len(r["shape"])
    ws = s.b["ws"].ptr
    before = dict((n, b.bits.clone()) for n, b in s.b.items())
    cases = []
    for kind in ("init", "direction", "update", "status", "finish", "precondition"):
        if kind not in s.ep:
            continue
        args = s.ep[kind][1]
        # df_pressure_status needs the plain solve's words only (the ghost-fluid and diffusion workspaces are longer behind them)
        need = int(s.lib.df_pressure_workspace_bytes(s.s["S"], s.s["Z"], s.s["Y"], s.s["X"])) if kind == "status" else s.s["ws_bytes"]
        assert 0 < need <= s.s["ws_bytes"]
        cases.append((kind, dict(ws_bytes=need - 1), _lib.DF_EWORKSPACE))
        cases.append((kind, dict(ws=ws + 2), _lib.DF_EALIGN))
        overlap = {"init": ["vel"], "update": ["pressure"], "status": ["count", "iters"], "finish": ["out"],
                   "direction": (["flags"] if cc.has_flags(r) else []) + ["alpha"]}.get(kind, [])
        for p in overlap:
            if p in args:
                cases.append((kind, {p: ws}, _lib.DF_EINVAL))
        if "os" in args:
            cases.append((kind, dict(os=64), _lib.DF_EINVAL))
            if nd == 2:
                cases.append((kind, dict(os=16), _lib.DF_EINVAL))
        if kind in ("direction", "update", "status"):
            cases.append((kind, dict(k=-1), _lib.DF_EINVAL))
        if kind == "direction":
            cases.append((kind, dict(acc=-1.0), _lib.DF_EINVAL))
            cases.append((kind, dict(max_iter=2 ** 31), _lib.DF_EINVAL))
    for kind in ("build", "correct"):
        if kind in s.ep and "os" in s.ep[kind][1]:
            cases.append((kind, dict(os=64), _lib.DF_EINVAL))
            if nd == 2:
                cases.append((kind, dict(os=16), _lib.DF_EINVAL))
    assert len(cases) >= 12
    for kind, over, want in cases:
        rc = s.rc(kind, **over)
        assert rc == want, (name, s.ep[kind][0], over, rc, want, s.lib.df_last_error())
        torch.cuda.synchronize()
        for n, b in s.b.items():
            assert torch.equal(b.bits, before[n]), "%s: %s refused %r and still changed %s" % (name, s.ep[kind][0], over, n)
