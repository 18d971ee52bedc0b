"""Timing probe of the smoke solver step (profiles/smoke.md): ms per simulation step, CG iterations per solve, microseconds per CG
iteration, launches per iteration and the share of wall time the host spends waiting on the convergence read-back, for the reference's
job (96x128, B = 105) and 64x96x64 at B = 1 and 4; plus the sweep of ``check_every`` behind ops.DEFAULT_CHECK_EVERY.

    python tools/smoke_probe.py [--steps 48] [--warm 8] [--reps 5] [--out FILE.json]

Wall clock around a synchronised run of ``steps`` simulation steps from the state after ``warm`` steps from rest (the plume has to exist
for the solve to have work), ``reps`` times per value of ``check_every`` with the values interleaved; the median run is reported with
the whole spread.  Launches are counted at the C-ABI boundary (``_lib.call``).  profiles/smoke_probe.json is its output."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import _lib, ops  # noqa: E402


class Counters(object):
    def __init__(self):
        self.calls = {}
        self.wait = 0.0
        self.reads = 0
        self._call, self._read = _lib.call, ops._read_word

    def __enter__(self):
        def call(name, *a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return self._call(name, *a)

        def read(t):
            t0 = time.perf_counter()
            v = self._read(t)
            self.wait += time.perf_counter() - t0
            self.reads += 1
            return v
        ops.call, ops._read_word = call, read
        return self

    def __exit__(self, *exc):
        ops.call, ops._read_word = self._call, self._read


def scene(shape, B):
    ext = shape[::-1]
    masks = []
    for e in range(B):
        c = [0.5 * n for n in ext]
        c[0] = (0.2 + 0.6 * (e / max(B - 1, 1))) * ext[0]
        c[1] = 0.1 * ext[1]
        masks.append(ops.sphere_mask(shape, c, (0.04 + 0.08 * ((e * 7) % 5) / 4.0) * ext[0]))
    m = torch.stack(masks).cuda()
    d = torch.zeros((B,) + shape, device="cuda")
    v = torch.zeros((B,) + shape + (len(shape),), device="cuda")
    return m, d, v


def warmed(shape, B, warm):
    """the state after ``warm`` steps from rest (the plume has to exist for the solve to have work), and the iteration counts so far"""
    m, d, v = scene(shape, B)
    stats = []
    for d, v in ops.simulate_smoke(d, v, warm, dt=0.5, source=m, stats=stats, stack=False):
        pass
    return m, d.clone(), v.clone(), stats


def timed(shape, m, d, v, steps, check_every):
    torch.cuda.synchronize()
    with Counters() as c:                                # iterations are counted from the launches
        t0 = time.perf_counter()
        for _ in ops.simulate_smoke(d, v, steps, dt=0.5, source=m, check_every=check_every, stack=False):
            pass
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    nd = len(shape)
    k1 = c.calls.get("df_pressure_cg_direction%dd" % nd, 0)
    k2 = c.calls.get("df_pressure_cg_update%dd" % nd, 0)
    st = c.calls.get("df_pressure_status", 0)
    return {"ms_per_step": 1e3 * wall / steps, "host_iterations_per_solve": k1 / float(steps), "wall_us_per_host_iteration": 1e6 * wall / max(k1, 1),
            "launches_per_iteration": (k1 + k2 + st) / float(max(k1, 1)), "reads_per_solve": c.reads / float(steps), "wait_share": c.wait / wall}


def sweep(shape, B, warm, steps, reps, values):
    """``reps`` rounds over ``values`` of check_every, interleaved so that drift of the machine hits all of them alike; every run starts
    from the same warmed state and so does the same arithmetic.  One untimed run first."""
    m, d, v, stats = warmed(shape, B, warm)
    timed(shape, m, d, v, min(steps, 4), values[0])
    runs = {ce: [] for ce in values}
    for _ in range(reps):
        for ce in values:
            runs[ce].append(timed(shape, m, d, v, steps, ce))
    out = []
    for ce in values:
        ms = sorted(r["ms_per_step"] for r in runs[ce])
        mid = sorted(runs[ce], key=lambda r: r["ms_per_step"])[len(ms) // 2]
        rec = {"shape": list(shape), "B": B, "check_every": ce, "steps": steps, "reps": reps, "ms_per_step_all": [round(x, 4) for x in ms],
               "ms_per_step_median": ms[len(ms) // 2], "ms_per_step_min": ms[0], "ms_per_step_max": ms[-1]}
        rec.update({k: mid[k] for k in mid if k != "ms_per_step"})
        out.append(rec)
        print(json.dumps(rec), flush=True)
    # iteration counts of a run of warm + steps from rest, over all entries and steps
    more = []
    for _ in ops.simulate_smoke(d, v, steps, dt=0.5, source=m, stats=more, stack=False):
        pass
    it = torch.stack(stats + more).cpu().numpy()
    its = {"shape": list(shape), "B": B, "min": int(it.min()), "median": float(np.median(it)), "max": int(it.max()),
           "slowest_entry_per_step": it.max(axis=1).tolist()}
    print(json.dumps(its), flush=True)
    return out, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": [], "iterations": []}
    for shape, B, values in (((128, 96), 105, (1, 4, 16, 64)), ((64, 96, 64), 1, (4, 16, 64)), ((64, 96, 64), 4, (4, 16, 64))):
        runs, its = sweep(shape, B, a.warm, a.steps, a.reps, values)
        out["runs"] += runs
        out["iterations"].append(its)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
