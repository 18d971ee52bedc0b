#!/usr/bin/env python3
"""Measurements behind profiles/advect.md, on one MI355X:

  python tools/advect_probe.py [--out advect_probe.json] [--skip-sweeps] [--reps 20]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/advect_probe.py --skip-sweeps      (per-kernel times of the same launches)

1. Per-launch HIP-event times of kernel A (df_advect_sl*), kernel B (df_advect_mc*) and the image kernel at 112x160x112 (B = 1, 4),
   64x96x64 (B = 16) and 2-D 128x96 (B = 64), after warm-up, with their algorithmic bytes (each array read or written once) and the
   effective rate, beside df_jacobian3d_fwd (60 B/voxel) on the same grid in the same run.
2. Wall time of a 200-frame ``Trainer.advect_`` sweep at the reference's scene sizes (2-D 128x96, 3-D 32x64x112) beside ``test_``.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

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


def rate(rec, nbytes):
    rec["bytes"] = int(nbytes)
    rec["GBps"] = nbytes / (rec["median_ms"] * 1e-3) / 1e9
    return rec


def kernels(shape, B, reps):
    nd = len(shape)
    g = torch.Generator().manual_seed(0)
    d = torch.rand((B,) + shape, generator=g).cuda()
    v = ((torch.rand((B,) + shape + (nd,), generator=g) - 0.5) * 6).cuda()        # up to 1.5 cells per step at dt = 0.5
    fwd, out = torch.empty_like(d), torch.empty_like(d)
    img = torch.empty((B, shape[-2], shape[-1]), dtype=torch.uint8, device="cuda")
    dims = [B] + list(shape)
    sfx = "%dd" % nd
    n = d.numel()
    res = {}
    res["A_sl"] = rate(event_times(lambda: call("df_advect_sl" + sfx, _ptr(d), _ptr(v), _ptr(fwd), *(dims + [0.5, 1.0, 1, _stream()])), reps),
                       n * 4 * (2 + nd))                                           # orig + vel in, fwd out
    for mode in (2, 1):
        res["B_mc_mode%d" % mode] = rate(event_times(
            lambda: call("df_advect_mc" + sfx, _ptr(d), _ptr(fwd), _ptr(v), _ptr(out), *(dims + [0.5, 1.0, 1, mode, _stream()])), reps),
            n * 4 * (3 + nd))                                                      # orig + fwd + vel in, out
    res["image"] = rate(event_times(lambda: call("df_density_image" + sfx, _ptr(d), _ptr(img), *(dims + [_stream()])), reps), n * 4 + img.numel())
    res["step_order2"] = event_times(lambda: ops.advect(d, v, 0.5, out=out, workspace=fwd.view(-1)), reps)
    if nd == 3:
        j = torch.empty((B,) + shape + (9,), device="cuda"); c = torch.empty((B,) + shape + (3,), device="cuda")
        res["jacobian3d_fwd"] = rate(event_times(lambda: call("df_jacobian3d_fwd", _ptr(v), _ptr(j), _ptr(c), *(dims + [_stream()])), reps), n * 60)
    else:
        j = torch.empty((B,) + shape + (4,), device="cuda"); w = torch.empty((B,) + shape + (1,), device="cuda")
        res["jacobian2d_fwd"] = rate(event_times(lambda: call("df_jacobian2d_fwd", _ptr(v), _ptr(j), _ptr(w), *(dims + [_stream()])), reps), n * 28)
    return res


def sweep(is_3d, frames, test_b_num, tmp):
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset
    from deep_fluids_amd.trainer import Trainer, Trainer3, default_config
    spatial = (32, 64, 112) if is_3d else (128, 96)
    root = os.path.join(tmp, "data3" if is_3d else "data2")
    write_synthetic_dataset(root, (4,) * len(spatial), num_p=(2, 2), num_frames=frames)      # only args.txt and the range are read here
    res = dict(res_x=spatial[-1], res_y=spatial[-2], res_z=spatial[0] if is_3d else 1)
    ops.reset_variables()
    tr = (Trainer3 if is_3d else Trainer)(default_config(is_3d=is_3d, num_samples=4 * frames, test_batch_size=test_b_num, **res))
    bm = BatchManager(SimpleNamespace(random_seed=1, data_path=root, is_3d=is_3d, arch="de", data_type="velocity", batch_size=2, num_worker=1,
                                      **res), device=None)
    src = {"center": (0.5 * spatial[-1], 0.1 * spatial[-2], 0.5 * spatial[0])[:len(spatial)], "radius": 0.08 * spatial[-1]}
    out = {}
    for rep in range(2):                                                           # the first call warms every kernel
        torch.cuda.synchronize(); t0 = time.time()
        tr.advect_(bm, model_dir=os.path.join(tmp, "adv%d" % is_3d), p1=1, p2=1, source=src)
        torch.cuda.synchronize(); out["advect_wall_ms"] = (time.time() - t0) * 1e3
    torch.cuda.synchronize(); t0 = time.time()
    tr.test_(bm, model_dir=os.path.join(tmp, "dump%d" % is_3d), p1=1, p2=1)
    torch.cuda.synchronize(); out["test_wall_ms"] = (time.time() - t0) * 1e3
    z = torch.zeros((test_b_num, 3), device="cuda")
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(frames // test_b_num):
        tr.generate(z)
    torch.cuda.synchronize(); out["generate_only_wall_ms"] = (time.time() - t0) * 1e3
    ops.reset_variables()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-sweeps", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"kernels": {}}
    for shape, B in (((112, 160, 112), 1), ((112, 160, 112), 4), ((64, 96, 64), 16), ((128, 96), 64)):
        res["kernels"]["%s B=%d" % ("x".join(map(str, shape)), B)] = kernels(shape, B, a.reps)
    if not a.skip_sweeps:
        res["sweeps"] = {}
        with tempfile.TemporaryDirectory() as tmp:
            for is_3d, b in ((False, 100), (True, 10)):
                key = "3d 32x64x112" if is_3d else "2d 128x96"
                try:
                    res["sweeps"][key] = sweep(is_3d, 200, b, tmp)
                except Exception as e:                                             # recorded, not hidden: the kernel figures above stand
                    res["sweeps"][key] = {"error": "%s: %s" % (type(e).__name__, e)}
    print(json.dumps(res, indent=1, sort_keys=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
