"""-m gpu: the launch sequence of the stride-1 conv nodes of ``ops.py``, call by call, against a recorded fixture.

Every case of the table below runs one forward and one backward through its node while ``ops.call`` is replaced by a wrapper that writes
down each C-ABI call and then calls through:  the entry-point name;  for a pointer argument (per ``_lib.SIGNATURES``) only whether it is
null;  every other argument's value;  for the trailing stream ``main`` (the stream that was current on entry) or ``side``.  Queries are
memoised and not part of the sequence.  The dict of dispatch counts of the case is compared as well.

The cases are the smallest at which a decision of the kernel choice flips -- grids at and below the Winograd size rules, channel counts
that are Winograd-eligible (32), direct-MFMA / bf16x3-eligible (16) and thin (4) -- under the default options and under each option that
enters the choice, each with the node input needing a gradient and not.

``python tests/test_gpu_conv_call_plan.py`` records the fixture (tests/golden/conv_call_plan.json.gz) from the ``ops.py`` it imports; with
``--only REGEX`` it re-records the cases whose id matches and keeps the others.
"""
import gzip
import json
import os
import re
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_call_plan.json.gz")

GRIDS = [(2, 8, 8, 8), (1, 4, 8, 8),        # 3-D: above / below the 6-voxel rule
         (2, 16, 24), (1, 16, 16)]          # 2-D: exactly at / below the 16 x 24 rule
OPTIONS = [{}, {"conv_algo": "direct"}, {"conv_algo": "winograd"}, {"wino3d_family": "f222"}, {"wino2d_family": "f22"}, {"wino2d_family": "auto"},
           {"sign_bit_masks": False}, {"conv_precision": "bf16x3"}, {"activation_fetch": []}, {"wgrad_algo": 1}, {"thin_valu_only": True},
           {"concurrent_wgrad_work": 0}]
SINGLE_CHANNELS = [(32, 32), (16, 16), (16, 4)]
#        node           leak/n  channels (cin, cout)
NODES = ([("same3", leak, c) for leak in (0.2, None) for c in SINGLE_CHANNELS] +
         [("same3s2", 0.2, c) for c in SINGLE_CHANNELS] +
         [("gen", n, (c, c)) for n in (1, 3) for c in (32, 16)] +
         [("chain", 2, c) for c in ((16, 32), (4, 32))] +
         [("up", n, (c, c)) for n in (1, 2, 3) for c in (32, 16)])


def _name(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def case_id(node, arg, ch, grid, opt, needs):
    o = ",".join("%s=%s" % kv for kv in opt.items()) or "default"
    return "%s-%s-C%s-%s-%s-%s" % (node, _name(arg), _name(ch), _name(grid), o, "gx" if needs else "nogx")


def cases():
    return [(node, arg, ch, grid, opt, needs) for opt in OPTIONS for grid in GRIDS for node, arg, ch in NODES for needs in (True, False)]


def run_case(node, arg, ch, grid, opt, needs):
    """-> (trace, dispatch counts) of one forward + backward"""
    import torch
    from deep_fluids_amd import ops, _lib
    nd = len(grid) - 1
    cin, cout = ch
    in_grid = (grid[0],) + tuple(d // 2 for d in grid[1:]) if node == "up" else grid      # the up-sampling node takes the coarse half
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(in_grid + (cin,), generator=g) * 2 - 1).cuda().requires_grad_(needs)
    n = 1 if node in ("same3", "same3s2") else arg
    wb = []
    for i in range(n):
        ci = cin if i == 0 else cout
        wb.append(((torch.rand((3,) * nd + (ci, cout), generator=g) * 2 - 1) / (ci * 3 ** nd) ** 0.5).cuda().requires_grad_(True))
        wb.append((torch.rand(cout, generator=g) * 0.6 - 0.3).cuda().requires_grad_(True))
    main = ops._stream()
    trace, counts = [], {}
    real = ops.call

    def spy(name, *a):
        types = _lib.SIGNATURES[name][1]
        assert len(types) == len(a) and types[-1] is _lib.P, name
        rec = [name]
        for t, v in zip(types[:-1], a[:-1]):
            rec.append(("null" if v is None else "ptr") if t is _lib.P else (float(v) if t is _lib.F32 else int(v)))
        rec.append("main" if a[-1] == main else "side")
        trace.append(rec)
        return real(name, *a)

    opt = dict(opt)
    if "activation_fetch" in opt:
        opt["activation_fetch"] = []
    with ops.options(dispatch_counts=counts, **opt):
        ops.call = spy
        try:
            if node == "same3":
                y = ops._ConvSame3.apply(x, wb[0], wb[1], arg)
            elif node == "same3s2":
                y = ops._ConvSame3S2.apply(x, wb[0], wb[1], arg)
            else:
                y = {"gen": ops._GenBlock, "chain": ops._ConvChain, "up": ops._UpGenBlock}[node].apply(x, 0.2, *wb)
            go = (torch.rand(tuple(y.shape), generator=g) * 2 - 1).cuda()
            torch.autograd.backward(y, go)
            torch.cuda.synchronize()
        finally:
            ops.call = real
    assert (x.grad is not None) == needs and all(t.grad is not None for t in wb)
    return trace, counts


def record(only=None):
    old = load() if only else {}
    out = {}
    for c in cases():
        cid = case_id(*c)
        if only and not re.search(only, cid):
            out[cid] = old[cid]
            continue
        trace, counts = run_case(*c)
        out[cid] = {"trace": trace, "dispatch": counts}
    # every distinct call once, the traces as indices into that list
    calls, index = [], {}
    for v in out.values():
        for i, rec in enumerate(v["trace"]):
            key = json.dumps(rec)
            if key not in index:
                index[key] = len(calls)
                calls.append(rec)
            v["trace"][i] = index[key]
    with gzip.GzipFile(FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps({"calls": calls, "cases": out}, sort_keys=True, separators=(",", ":")).encode())
    return len(out), len(calls)


def load():
    with gzip.open(FIXTURE, "rb") as f:
        fx = json.loads(f.read().decode())
    return {cid: {"trace": [fx["calls"][i] for i in v["trace"]], "dispatch": v["dispatch"]} for cid, v in fx["cases"].items()}


@pytest.fixture(scope="module")
def recorded():
    return load()


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded) == sorted(case_id(*c) for c in cases())


@pytest.mark.gpu
@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "default")
def test_launch_sequence_is_the_recorded_one(recorded, opt):
    bad = []
    for c in cases():
        if c[4] is not opt:
            continue
        cid = case_id(*c)
        trace, counts = run_case(*c)
        want = recorded[cid]
        if trace != want["trace"] or counts != want["dispatch"]:
            bad.append(cid)
            print("\n%s\n  recorded:\n%s\n  %r\n  now:\n%s\n  %r" % (cid, "\n".join("    %r" % (r,) for r in want["trace"]), want["dispatch"],
                                                                   "\n".join("    %r" % (r,) for r in trace), counts))
    assert not bad, "%d cases launch another sequence than recorded (both traces above): %s" % (len(bad), bad[:8])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    print("recorded %d cases, %d distinct calls -> %s" % (record(only) + (FIXTURE,)))
