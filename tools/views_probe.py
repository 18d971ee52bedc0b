#!/usr/bin/env python3
"""Measurements behind profiles/views.md, on one MI355X:

  python tools/views_probe.py [--out views_probe.json] [--skip-sheets]

1. df_velocity_views3d at [16,64,96,64,3]: per-launch HIP-event times over 20 launches after warm-up, against (a) the torch composition
   that yields the same eight views from the same input (ops.curl3, two means, two slices, clamp and a uint8 cast per field) and (b) the
   time to read the field once at the device-to-device copy rate measured here.
2. The count of projected pixels that differ from a float64 mean, per shape.
3. The wall time of one `Trainer.sample_images` call at the 64x96x64 grid (batch 16, filters 128, c_num 3) beside the `<step>_G.npz`
   path of `Trainer.train` it supersedes (the same fields copied to the host at full size and compressed).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_fluids_amd import ops  # noqa: E402


def event_times(fn, n=20, warm=5):
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


def torch_views(f):
    def den(v):
        return ((v + 1) * 127.5).clamp(0, 255).to(torch.uint8)
    Z, X = f.shape[1], f.shape[3]
    return {"xy": den(f.mean(1)), "zy": den(f.mean(3).transpose(1, 2)), "xym": den(f[:, Z // 2]), "zym": den(f[:, :, :, X // 2].transpose(1, 2))}


def torch_composition(u):
    return torch_views(u), torch_views(ops.curl3(u))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-sheets", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {}
    u = (torch.randn((16, 64, 96, 64, 3), generator=torch.Generator().manual_seed(0)) * 0.5).cuda()
    nbytes = u.numel() * 4
    res["fused"] = event_times(lambda: ops.velocity_views3(u))
    res["torch_composition"] = event_times(lambda: torch_composition(u))
    dst = torch.empty_like(u)
    res["d2d_copy"] = event_times(lambda: dst.copy_(u))
    copy_rate = 2 * nbytes / (res["d2d_copy"]["median_ms"] * 1e-3)                      # read + write
    res["copy_rate_GBps"] = copy_rate / 1e9
    res["read_once_ms"] = nbytes / copy_rate * 1e3
    res["fused_over_read_once"] = res["fused"]["median_ms"] / res["read_once_ms"]
    res["speedup_vs_torch"] = res["torch_composition"]["median_ms"] / res["fused"]["median_ms"]
    # same pictures? (mid slices bit for bit; projections within one grey level)
    (fu, fc), (tu, tc) = ops.velocity_views3(u), torch_composition(u)
    res["vs_torch"] = {}
    for name, f, t in (("u", fu, tu), ("curl", fc, tc)):
        for k in f:
            d = (f[k].int() - t[k].int()).abs()
            res["vs_torch"]["%s_%s" % (name, k)] = {"differ": int((d != 0).sum()), "max": int(d.max()), "pixels": d.numel()}
    # projected pixels that differ from a float64 mean
    res["projection_vs_fp64"] = {}
    for shape in ((2, 16, 24, 16, 3), (2, 64, 96, 64, 3), (2, 13, 10, 7, 3)):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(1)) * 0.5
        v = ops.denorm_img3(x.cuda())
        x64 = x.numpy().astype(np.float64)
        for k, w in (("xy", x64.mean(1)), ("zy", x64.mean(3).transpose(0, 2, 1, 3))):
            w8 = np.clip((w.astype(np.float32) + np.float32(1)) * np.float32(127.5), 0, 255).astype(np.uint8)
            d = np.abs(v[k].cpu().numpy().astype(np.int32) - w8)
            res["projection_vs_fp64"]["%s %s" % ("x".join(map(str, shape[1:4])), k)] = {"differ": int((d != 0).sum()), "max": int(d.max()),
                                                                                      "pixels": int(d.size)}
    del u, dst
    if not a.skip_sheets:
        from deep_fluids_amd.trainer import Trainer3, default_config
        ops.reset_variables()
        b = 16
        tr = Trainer3(default_config(is_3d=True, res_x=64, res_y=96, res_z=64, filters=128, batch_size=b, num_samples=1000))
        z_sweeps = []
        for i in range(3):
            zi = np.zeros((b, 3), np.float32)
            zi[:, i] = np.linspace(-1, 1, num=b)
            z_sweeps.append(zi)
        with tempfile.TemporaryDirectory() as tmp:
            for rep in range(2):                                                        # the first call warms every kernel
                torch.cuda.synchronize(); t0 = time.time()
                tr.sample_images(z_sweeps + [z_sweeps[0]], tmp, rep)
                torch.cuda.synchronize(); res["sample_images_wall_s"] = time.time() - t0
            res["sheet_bytes"] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp) if f.startswith("1_") or f.endswith("_1.png"))
            torch.cuda.synchronize(); t0 = time.time()
            G = np.stack([tr.generate(torch.from_numpy(z).to(tr.device)).cpu().numpy() for z in z_sweeps])      # Trainer.train, sample_images=False
            np.savez_compressed(os.path.join(tmp, "0_G.npz"), G=G, z=np.stack(z_sweeps))
            res["g_npz_wall_s"] = time.time() - t0
            res["g_npz_bytes"] = os.path.getsize(os.path.join(tmp, "0_G.npz"))
            torch.cuda.synchronize(); t0 = time.time()
            for z in z_sweeps + [z_sweeps[0]]:
                tr.generate(torch.from_numpy(z).to(tr.device))
            torch.cuda.synchronize(); res["generate_only_wall_s"] = time.time() - t0
        ops.reset_variables()
    print(json.dumps(res, indent=1, sort_keys=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
