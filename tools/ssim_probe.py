#!/usr/bin/env python
"""Times ``ops.field_ssim`` (SSIM and MS-SSIM per entry; csrc/ssim.hip) against the same quantities composed from existing torch ops on
the same device -- a depthwise-free ``conv2d`` with the reference's [S,S,C,C] window on the five products, the maps, ``mean`` and, for
MS-SSIM, ``avg_pool2d(ceil_mode=True, count_include_pad=False)`` between the levels.  The composition lives here only; no torch conv
enters the package.  Two shapes in one run, the 2-D data's 64 x 128x96x2 and one 3-D field 1 x 64x96x64x3 folded to 64 slices, each in a
fresh child process under its own time limit; a child that fails or runs out of time ends the run.  Prints a markdown table (the one of
profiles/ssim.md): microseconds per call (median of ``--iters`` calls after ``--warmup``, HIP events), the speed-up, and the fused call's
fraction of the COPY RATE measured in the same run (a device-to-device ``copy_`` of 256 MiB: bytes read plus bytes written per second)
from the algorithmic bytes -- two image reads per level plus the pooled pair written.

    python tools/ssim_probe.py [--iters 50] [--warmup 10] [--limit 120]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 128, 96, 2), (1, 64, 96, 64, 3)]
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def composition(torch, ops, a, b, multiscale):
    """per-image (ms-)ssim [N] of NHWC images from torch ops: what a user had to write before"""
    F = torch.nn.functional
    a, b = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)

    def level(a, b):
        C, H, W = a.shape[1:]
        size = min(11, H, W)
        w = ops.fspecial_gauss(size, 1.5 * size / 11, C).to(a.device).permute(3, 2, 0, 1).contiguous()
        p, q = (a + 1) / 2, (b + 1) / 2
        mu1, mu2, e11, e22, e12 = (F.conv2d(t, w) for t in (p, q, p * p, q * q, p * q))
        s11, s22, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
        v1, v2 = 2 * s12 + 0.03 ** 2, s11 + s22 + 0.03 ** 2
        val = ((2 * mu1 * mu2 + 0.01 ** 2) * v1) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * v2)
        return val.mean((1, 2, 3)), (v1 / v2).mean((1, 2, 3))
    if not multiscale:
        return level(a, b)[0]
    out = 1.0
    for k, wk in enumerate(WEIGHTS):
        s, c = level(a, b)
        out = out * (s if k == len(WEIGHTS) - 1 else c) ** wk
        if k < len(WEIGHTS) - 1:
            a, b = (F.avg_pool2d(t, 2, 2, ceil_mode=True, count_include_pad=False) for t in (a, b))
    return out


def child(shape, iters, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from deep_fluids_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(shape, device="cuda", generator=gen) * 1.6 - 0.8
    g = x + 0.05 * torch.randn(shape, device="cuda", generator=gen)
    a, b = g.reshape((-1,) + shape[-3:]), x.reshape((-1,) + shape[-3:])

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

    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src))
    out = {"shape": list(shape), "copy_tbs": 2 * src.numel() * 4 / (copy_us * 1e-6) / 1e12}
    lvl, n = [], a.numel() * 4
    H, W = shape[-3], shape[-2]
    for k in range(5):                                                   # bytes per level: both images read; the pooled pair written
        lvl.append((H * W, ((H + 1) // 2) * ((W + 1) // 2)))
        H, W = (H + 1) // 2, (W + 1) // 2
    px = shape[-3] * shape[-2]
    out["bytes_ssim"] = 2 * n
    out["bytes_ms"] = sum(2 * n * h // px + (2 * n * p // px if k < 4 else 0) for k, (h, p) in enumerate(lvl))
    with torch.no_grad():
        for ms, tag in ((False, "ssim"), (True, "ms")):
            ws = ops.ssim_workspace(g, multiscale=ms)
            out[tag + "_us"] = timed(lambda: ops.field_ssim(g, x, multiscale=ms, workspace=ws))
            out[tag + "_comp_us"] = timed(lambda: composition(torch, ops, a, b, ms))
            f = ops.field_ssim(g, x, multiscale=ms, workspace=ws)
            c = composition(torch, ops, a, b, ms).double().reshape(shape[0], -1).mean(1) if not ms else None
            out[tag + "_diff"] = float((f - c).abs().max()) if c is not None else None      # the two agree to fp32 rounding
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
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
    print("| shape | call | fused (us) | torch composition (us) | speed-up | algorithmic bytes | copy rate, same run (TB/s) | fused, fraction of it |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        for tag, name in (("ssim", "field_ssim"), ("ms", "field_ssim multiscale")):
            rate = r["bytes_" + tag] / (r[tag + "_us"] * 1e-6) / 1e12
            print("| %s | %s | %.1f | %.1f | %.1fx | %.1f MB | %.2f | %.0f %% |" % (
                " x ".join(str(n) for n in r["shape"]), name, r[tag + "_us"], r[tag + "_comp_us"], r[tag + "_comp_us"] / r[tag + "_us"],
                r["bytes_" + tag] / 1e6, r["copy_tbs"], 100 * rate / r["copy_tbs"]))
        print("<!-- %s: |fused - composition| ssim %.2e -->" % (r["shape"], r["ssim_diff"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
