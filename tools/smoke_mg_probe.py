"""Timing probe of the multigrid-preconditioned smoke pressure solve against the plain one (profiles/smoke_mg.md): CG iterations per
solve, launches per simulation step and ms per simulation step for ``preconditioner=None`` and ``"mg"``, on the three jobs of
tools/smoke_probe.py (96x128 at B = 105, 64x96x64 at B = 1 and 4).

    python tools/smoke_mg_probe.py [--steps 48] [--warm 8] [--reps 5] [--out FILE.json]

Wall clock around a synchronised run of ``steps`` simulation steps from the state after ``warm`` plain steps from rest (the plume has to
exist for the solve to have work), ``reps`` times per arm with the two arms interleaved so that drift of the machine hits both alike;
the median run is reported with the whole spread.  Both arms start from the same state.  Launches are kernel launches: the calls at the
C-ABI boundary (``_lib.call``), one launch each, except a V-cycle, which is ``df_mg_cycle_launches``, and a hierarchy build, one per
level; a cycle or an iteration launched for entries that have all stopped still counts.  The iteration counts are the solver's own
(``stats=``), over all entries and steps.  The ``"mg"`` arm builds its hierarchy once per run, inside the timed region, as a sequence
does.  profiles/smoke_mg_probe.json is its output."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import _lib, ops  # noqa: E402
from smoke_probe import Counters, warmed  # noqa: E402

ARMS = (None, "mg")


def launches(calls, shape):
    dims = ([1] if len(shape) == 2 else []) + list(shape)
    per = {"df_pressure_mg_precondition": _lib.query("df_mg_cycle_launches", len(shape), *dims), "df_mg_build": _lib.query("df_mg_levels", len(shape), *dims)}
    return sum(n * per.get(name, 1) for name, n in calls.items())


def timed(m, d, v, steps, arm):
    torch.cuda.synchronize()
    stats = []
    with Counters() as c:
        t0 = time.perf_counter()
        for _ in ops.simulate_smoke(d, v, steps, dt=0.5, source=m, stats=stats, stack=False, preconditioner=arm):
            pass
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    it = torch.stack(stats).cpu().numpy()                  # [steps, B]
    return {"ms_per_step": 1e3 * wall / steps, "launches_per_step": launches(c.calls, tuple(d.shape[1:])) / float(steps),
            "iterations_per_solve_median": float(np.median(it)), "iterations_per_solve_min": int(it.min()),
            "iterations_per_solve_max": int(it.max()), "slowest_entry_per_solve_mean": float(it.max(axis=1).mean()),
            "reads_per_solve": c.reads / float(steps), "wait_share": c.wait / wall}


def job(shape, B, warm, steps, reps):
    m, d, v, _ = warmed(shape, B, warm)
    for arm in ARMS:                                       # one untimed run of each arm first
        timed(m, d, v, min(steps, 4), arm)
    runs = {arm: [] for arm in ARMS}
    for _ in range(reps):
        for arm in ARMS:
            runs[arm].append(timed(m, d, v, steps, arm))
    out = []
    for arm in ARMS:
        ms = sorted(r["ms_per_step"] for r in runs[arm])
        mid = sorted(runs[arm], key=lambda r: r["ms_per_step"])[len(ms) // 2]
        rec = {"shape": list(shape), "B": B, "preconditioner": arm, "steps": steps, "reps": reps, "ms_per_step_all": [round(x, 4) for x in ms],
               "ms_per_step_median": ms[len(ms) // 2], "ms_per_step_min": ms[0], "ms_per_step_max": ms[-1]}
        rec.update({k: mid[k] for k in mid if k != "ms_per_step"})
        out.append(rec)
        print(json.dumps(rec), flush=True)
    a, b = out
    print("%s B %d: plain %.3f [%.3f - %.3f] ms/step, %.0f launches/step, %.0f iterations/solve | mg %.3f [%.3f - %.3f] ms/step, %.0f launches/step, "
          "%.0f iterations/solve | %s wins" % (
              "x".join(map(str, shape)), B, a["ms_per_step_median"], a["ms_per_step_min"], a["ms_per_step_max"], a["launches_per_step"],
              a["iterations_per_solve_median"], b["ms_per_step_median"], b["ms_per_step_min"], b["ms_per_step_max"], b["launches_per_step"],
              b["iterations_per_solve_median"], "mg" if b["ms_per_step_median"] < a["ms_per_step_median"] else "plain"), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": []}
    for shape, B in (((128, 96), 105), ((64, 96, 64), 1), ((64, 96, 64), 4)):
        out["runs"] += job(shape, B, a.warm, a.steps, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
