"""Timing probe of the noise inflow, the cylinder stamp and the per-entry force (profiles/smoke_inflow.md) on the grid of
scene/smoke3_vel_buo.py, 32 x 64 x 112 at B = 15 (the 5 x 3 scenes as one batch) and B = 1, in the style of tools/smoke_open_probe.py: one
process, the variants interleaved, five runs each.

    python tools/smoke_inflow_probe.py [--calls 200] [--steps 8] [--reps 5] [--out FILE.json]

Per kernel: wall clock around ``calls`` back-to-back launches on one stream, synchronised at both ends, as microseconds per launch
(``df_wall_buoyancy3d_open`` with host scalars beside the ``_dev`` form on the same fields).  Per scene: ms per simulation step of
``simulate_smoke`` with the inflow, the stamp and the force tensor, from rest.  Nothing here is a pass / fail number."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import ops  # noqa: E402
from deep_fluids_amd.data import smoke3_vel_buo_inflow, smoke3_vel_buo_scenes  # noqa: E402


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    X, Y, Z = 112, 64, 32
    shape = (Z, Y, X)
    p_list, _ = smoke3_vel_buo_scenes(1, 5, 5, -2e-4, -10e-4, 3)
    out = []
    for B in (15, 1):
        inflow = smoke3_vel_buo_inflow((X, Y, Z))
        values = torch.tensor([[p[0], 0.0, 0.0] for p in p_list[:B]], dtype=torch.float32, device="cuda")
        forces = ops.buoyancy_forces(shape, 0.5, p_list[:B, 1]).cuda()
        f0 = ops.default_buoyancy_force(shape, 0.5, float(p_list[0, 1]))
        d = torch.rand((B,) + shape, device="cuda") * 0.3
        v = torch.randn((B,) + shape + (3,), device="cuda")
        d2, v2 = torch.empty_like(d), torch.empty_like(v)
        kernels = {
            "df_density_noise_inflow3d": lambda: ops.density_inflow(d, inflow, time=1.0, out=d2),
            "df_mac_cylinder_stamp3d": lambda: ops.stamp_velocity(v, inflow.shape, values, out=v2),
            "df_wall_buoyancy3d_open": lambda: ops.wall_buoyancy(v, d, f0, out=v2, open_bound="XyY"),
            "df_wall_buoyancy3d_open_dev": lambda: ops.wall_buoyancy(v, d, forces, out=v2, open_bound="XyY"),
        }
        runs = {k: [] for k in kernels}
        for _ in range(a.reps):
            for k, fn in kernels.items():                  # interleaved
                runs[k].append(timed(fn, a.calls))
        for k, us in runs.items():
            us = sorted(us)
            rec = dict(shape=list(shape), B=B, what=k, us_median=us[len(us) // 2], us_min=us[0], us_max=us[-1],
                       bytes_per_launch=int(d.numel() * 4 * (2 if "inflow" in k else 6 if "stamp" in k else 7)))
            out.append(rec)
            print(json.dumps(rec))
        d0, v0 = torch.zeros_like(d), torch.zeros_like(v)
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in ops.simulate_smoke(d0, v0, a.steps, dt=0.5, source=inflow, force=forces, open_bound="XyY", inflow_velocity=(inflow.shape, values),
                                        stack=False):
                pass
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / a.steps)
        ms = sorted(ms)
        rec = dict(shape=list(shape), B=B, what="simulate_smoke step", ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1])
        out.append(rec)
        print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
