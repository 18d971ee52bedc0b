"""Timing probe of the smoke solver around obstacles (profiles/smoke_obstacles.md): the scene of the reference's smoke3_obs_buo.py at
64x96x64 with its default spheres, B = 1, 4 and 11 obstacle positions, the masked path (``obstacle=`` flags) beside the unmasked one
(the same scene without the obstacle) in one process, interleaved, ``reps`` runs each: ms per step, CG iterations min / median / max,
wall microseconds per host iteration.  ``--chunk`` also runs one chunk of the default data set (11 scenes x ``--frames`` frames, nothing
written) and reports its wall time and the iterations of the later frames.

    python tools/smoke_obstacle_probe.py [--steps 16] [--warm 8] [--reps 5] [--chunk] [--frames 150] [--out FILE.json]

The two paths solve different problems (the obstacle changes the flow), so their iteration counts differ: the cost of the flags byte
is read from the microseconds per host iteration, not from the milliseconds per step."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import ops  # noqa: E402
from smoke_probe import Counters  # noqa: E402

SHAPE = (64, 96, 64)
BUOYANCY = -8e-3


def scene(B):
    Z, Y, X = SHAPE
    xs = np.linspace(0.2, 0.8, 11)[:B] if B > 1 else [0.5]
    src = ops.sphere_mask(SHAPE, (X * 0.5, Y * 0.13, Z * 0.5), X * 0.12).cuda()
    obs = torch.stack([ops.sphere_mask(SHAPE, (X * x, Y * 0.5, Z * 0.5), X * 0.15) for x in xs]).cuda()
    d = torch.zeros((B,) + SHAPE, device="cuda")
    v = torch.zeros((B,) + SHAPE + (3,), device="cuda")
    return src, ops.obstacle_flags(obs, 1), d, v, ops.default_buoyancy_force(SHAPE, 0.5, gravity=BUOYANCY)


def run(src, flags, d, v, force, steps, stats=None):
    for d, v in ops.simulate_smoke(d, v, steps, dt=0.5, source=src, force=force, obstacle=flags, stats=stats, stack=False):
        pass
    return d.clone(), v.clone()


def timed(src, flags, d, v, force, steps):
    torch.cuda.synchronize()
    stats = []
    with Counters() as c:
        t0 = time.perf_counter()
        run(src, flags, d, v, force, steps, stats)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    k = c.calls.get("df_pressure_cg_direction3d" + ("_flags" if flags is not None else ""), 0)
    it = torch.stack(stats).cpu().numpy()
    return {"ms_per_step": 1e3 * wall / steps, "wall_us_per_host_iteration": 1e6 * wall / max(k, 1), "host_iterations_per_solve": k / float(steps),
            "iterations_min": int(it.min()), "iterations_median": float(np.median(it)), "iterations_max": int(it.max())}


def compare(B, warm, steps, reps):
    src, flags, d0, v0, force = scene(B)
    state = {"masked": run(src, flags, d0, v0, force, warm), "unmasked": run(src, None, d0, v0, force, warm)}
    fl = {"masked": flags, "unmasked": None}
    for k in fl:
        timed(src, fl[k], state[k][0], state[k][1], force, min(steps, 4))       # one untimed run each
    runs = {k: [] for k in fl}
    for _ in range(reps):
        for k in fl:
            runs[k].append(timed(src, fl[k], state[k][0], state[k][1], force, steps))
    out = {"shape": list(SHAPE), "B": B, "warm": warm, "steps": steps, "reps": reps}
    for k in fl:
        mid = sorted(runs[k], key=lambda r: r["wall_us_per_host_iteration"])[reps // 2]
        out[k] = dict(mid, ms_per_step_all=[round(r["ms_per_step"], 3) for r in runs[k]],
                      wall_us_per_host_iteration_all=[round(r["wall_us_per_host_iteration"], 2) for r in runs[k]])
    out["masked_over_unmasked_us_per_iteration"] = out["masked"]["wall_us_per_host_iteration"] / out["unmasked"]["wall_us_per_host_iteration"]
    print(json.dumps(out), flush=True)
    return out


def chunk(frames):
    src, flags, d0, v0, force = scene(11)
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(src, flags, d0, v0, force, frames, stats)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    it = torch.stack(stats).cpu().numpy()
    out = {"chunk": "11 scenes x %d frames, buoyancy %g, nothing written" % (frames, BUOYANCY), "wall_s": wall,
           "slowest_entry_per_frame": it.max(axis=1).tolist(), "median_per_frame": np.median(it, axis=1).tolist()}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", action="store_true")
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "runs": [compare(B, a.warm, a.steps, a.reps) for B in (1, 4, 11)]}
    if a.chunk:
        out["chunk"] = chunk(a.frames)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
