#!/usr/bin/env python
"""Times ``ops.field_metrics`` (one fused pass; csrc/metrics.hip) against the composition of existing ops that gives the same numbers:
``jacobian3`` x2, ``divergence3`` x2 (2-D: ``jacobian``, ``divergence``), the differences, |.| and the torch reductions.  Two shapes in
one run, cfg3's 16 x 64x96x64x3 and the 2-D 64 x 128x96x2, each in a fresh child process under its own time limit; a child that fails or
runs out of time ends the run.  Prints a markdown table (the one of profiles/field_metrics.md): microseconds per call (median of
``--iters`` calls after ``--warmup``, HIP events), the speed-up, and the fused call's fraction of the HBM peak computed from the
algorithmic bytes -- two field reads (plus the mask, none here).

    python tools/field_metrics_probe.py [--iters 50] [--warmup 10] [--limit 120] [--peak-tbs 8.0]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 64, 96, 64), (64, 128, 96)]


def composition(ops, torch, g, x):
    """the same quantities from the existing ops (per entry): what a user had to write before"""
    is_3d = g.dim() == 5
    jac, div = (ops.jacobian3, ops.divergence3) if is_3d else (ops.jacobian, ops.divergence)
    B = g.shape[0]
    d = (g - x).reshape(B, -1)
    ad = d.abs()
    dg, dx = div(g).reshape(B, -1).abs(), div(x).reshape(B, -1).abs()
    xs = x.reshape(B, -1)
    return (ad.sum(1), (d * d).sum(1), ad.max(1), xs.abs().sum(1), (xs * xs).sum(1), (jac(g)[0] - jac(x)[0]).abs().reshape(B, -1).sum(1),
            dg.sum(1), dg.max(1).values, dx.sum(1), dx.max(1).values)


def child(shape, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from deep_fluids_amd import ops
    D = len(shape) - 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(shape + (D,), device="cuda", generator=gen) * 2 - 1
    g = x + 0.1 * (torch.rand(shape + (D,), device="cuda", generator=gen) * 2 - 1)
    ws = ops.field_metrics_workspace(g)

    def timed(fn):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]

    with torch.no_grad():
        fused = timed(lambda: ops.field_metrics(g, x, workspace=ws))
        comp = timed(lambda: composition(ops, torch, g, x))
        fm, c = ops.field_metrics(g, x, workspace=ws), composition(ops, torch, g, x)
    rel = float(((fm.sum_abs_jac - c[5]).abs() / c[5]).max())          # the two agree (fp32 torch reductions: to rounding)
    print(json.dumps({"shape": list(shape), "fused_us": fused, "composition_us": comp, "bytes": 2 * g.numel() * 4, "jac_rel_diff": rel}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak in TB/s the fraction refers to (MI355X: 8.0)")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(tuple(json.loads(a.child)), a.iters, a.warmup)
    rows = []
    for shape in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(shape), "--iters", str(a.iters), "--warmup", str(a.warmup)]
        try:
            out = subprocess.run(cmd, timeout=a.limit, check=True, stdout=subprocess.PIPE).stdout.decode()
        except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as e:
            print("shape %s: %s -- stopping" % (shape, e), file=sys.stderr)
            return 1
        rows.append(json.loads(out.strip().splitlines()[-1]))
    print("| shape | fused (us) | composition (us) | speed-up | algorithmic bytes | fused, fraction of %.1f TB/s |" % a.peak_tbs)
    print("|---|---|---|---|---|---|")
    for r in rows:
        frac = r["bytes"] / (r["fused_us"] * 1e-6) / (a.peak_tbs * 1e12)
        print("| %s | %.1f | %.1f | %.1fx | %.1f MB | %.0f %% |" % (" x ".join(str(n) for n in r["shape"]), r["fused_us"], r["composition_us"],
                                                                  r["composition_us"] / r["fused_us"], r["bytes"] / 1e6, 100 * frac))
    return 0


if __name__ == "__main__":
    sys.exit(main())
