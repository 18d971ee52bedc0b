#!/usr/bin/env python3
"""Measurements behind profiles/particles.md, on one MI355X:

  python tools/particles_probe.py [--out particles_probe.json] [--reps 20]

At the liquid3_vis size (96x72x48 = [Z,Y,X] 48x72x96, the box of scene/liquid3_vis.py:84-85 seeded at 8 particles per cell) and at the
2-D liquid_pos_size size (128x64, a basin), B = 1: per-launch HIP-event times, after warm-up, of the RK4 trace (df_particles_advect*),
the keys kernel, the gather and the level set (df_particle_levelset_union*, radius_factor 1), of torch's stable sort + searchsorted
between them and of one whole frame of ``ops.liquid_sequence``; each kernel's algorithmic bytes (every array read or written once)
beside a device-to-device copy of the same number of bytes in the same run.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_fluids_amd import ops  # noqa: E402
from deep_fluids_amd.ops import _ptr, _stream, call  # noqa: E402


def event_times(fn, n, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = np.array(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())}


def with_copy(rec, nbytes, reps):
    """the kernel's algorithmic bytes, its effective rate, and a copy that moves as many bytes (half read, half written)"""
    rec["bytes"] = int(nbytes)
    rec["GBps"] = nbytes / (rec["median_ms"] * 1e-3) / 1e9
    n = max(int(nbytes) // 8, 1)
    src = torch.empty((n,), dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    c = event_times(lambda: dst.copy_(src), reps)
    rec["copy_same_bytes_ms"] = c["median_ms"]
    rec["copy_GBps"] = 8.0 * n / (c["median_ms"] * 1e-3) / 1e9
    return rec


def scene(shape, body, reps):
    nd = len(shape)
    pos0 = ops.seed_particles(body, discretization=2, randomness=0.05, seed=123)
    N = pos0.shape[0]
    pos = torch.from_numpy(pos0).cuda().unsqueeze(0)
    g = torch.Generator().manual_seed(0)
    vel = ((torch.rand((1,) + shape + (nd,), generator=g) - 0.5) * 3).cuda()       # up to 1.5 cells per step at dt = 1
    out = torch.empty_like(pos)
    keys = torch.empty((N,), dtype=torch.int32, device="cuda")
    phi = torch.empty((1,) + shape, device="cuda")
    dims = list(shape)
    sfx = "%dd" % nd
    ncell = int(np.prod(shape))
    res = {"particles": int(N), "cells": ncell}
    rec = 4 * nd * N
    res["trace"] = with_copy(event_times(lambda: call("df_particles_advect" + sfx, _ptr(pos), _ptr(out), _ptr(vel), 1, N,
                                                      *(dims + [1.0, 1.0, 1, _stream()])), reps), 2 * rec + 4 * nd * ncell, reps)
    res["keys"] = with_copy(event_times(lambda: call("df_particles_cell_keys" + sfx, _ptr(pos), _ptr(keys), 1, N, *(dims + [_stream()])), reps),
                            rec + 4 * N, reps)
    skeys, order = torch.sort(keys, stable=True)
    res["torch_sort_searchsorted"] = event_times(
        lambda: torch.searchsorted(torch.sort(keys, stable=True)[0], torch.arange(ncell + 1, dtype=torch.int32, device="cuda"), out_int32=True), reps)
    spos = torch.empty_like(pos)
    res["gather"] = with_copy(event_times(lambda: call("df_particles_gather", _ptr(pos), _ptr(order), _ptr(spos), N, nd, _stream()), reps),
                              2 * rec + 8 * N, reps)
    _, cell_start, _ = ops.particle_cells(pos, shape)
    res["levelset_rf1"] = with_copy(event_times(lambda: call("df_particle_levelset_union" + sfx, _ptr(spos), _ptr(cell_start), _ptr(phi), 1, N,
                                                             *(dims + [1.0, _stream()])), reps), rec + 4 * (ncell + 1) + 4 * ncell, reps)
    res["levelset_rf1"]["particle_reads_per_cell"] = float((2 * 2 + 1) ** nd * N / float(ncell))   # upper bound: the full window
    res["frame_of_liquid_sequence"] = event_times(lambda: ops.liquid_sequence(pos, vel.unsqueeze(0), 1.0, images=True), max(reps // 4, 3), warm=2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {}
    s3 = (48, 72, 96)
    res["liquid3_vis 96x72x48"] = scene(s3, ops.box_levelset(s3, (0.3 * 96, 0.0, 0.3 * 48), (0.7 * 96, 0.8 * 72, 0.7 * 48)), a.reps)
    s2 = (64, 128)
    res["liquid_pos_size 128x64"] = scene(s2, ops.box_levelset(s2, (0.0, 0.0), (128.0, 0.2 * 64)), a.reps)
    print(json.dumps(res, indent=1, sort_keys=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
