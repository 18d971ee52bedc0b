"""Timing probe of the smoke solver with open sides (profiles/smoke_open.md): the open path (``open_bound='xXyY'`` / ``'xXyYzZ'``) beside
the closed one on the same scene, in one process, interleaved, five runs each, as tools/smoke_probe.py does: 96x128 at B = 105 and
48x72x48 (the grid of scene/smoke3_rot.py and smoke3_mov.py) at B = 1 and 4.

    python tools/smoke_open_probe.py [--steps 24] [--warm 8] [--reps 5] [--out FILE.json]

Wall clock around a synchronised run of ``steps`` simulation steps from the state after ``warm`` steps from rest of the SAME path; the
median and the range of wall microseconds per host iteration (one direction and one update launch) and the CG iteration counts are
reported.  The two paths solve different problems, so iteration counts and ms / step differ for that reason; the cost of the open
branches is the ratio of the microseconds per host iteration.  Nothing here is a pass / fail number."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import ops  # noqa: E402
from smoke_probe import Counters, scene  # noqa: E402


def run(m, d, v, steps, open_bound):
    stats = []
    with Counters() as c:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in ops.simulate_smoke(d, v, steps, source=m, stack=False, stats=stats, open_bound=open_bound):
            pass
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    iters = torch.stack(stats).cpu().numpy()
    host_iters = sum(n for k, n in c.calls.items() if k.startswith("df_pressure_cg_update"))
    return dict(ms_per_step=1e3 * wall / steps, us_per_host_iteration=1e6 * wall / max(host_iters, 1), host_iterations=host_iters,
                iters_min=int(iters.min()), iters_median=float(np.median(iters)), iters_max=int(iters.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for shape, B in (((128, 96), 105), ((48, 72, 48), 1), ((48, 72, 48), 4)):
        spec = "xXyY" if len(shape) == 2 else "xXyYzZ"
        m, d0, v0 = scene(shape, B)
        state = {}
        for name, ob in (("closed", None), ("open", spec)):
            d, v = d0, v0
            for d, v in ops.simulate_smoke(d0, v0, a.warm, source=m, stack=False, open_bound=ob):
                pass
            state[name] = (d.clone(), v.clone(), ob)
        runs = {"closed": [], "open": []}
        for _ in range(a.reps):
            for name in ("closed", "open"):                # interleaved
                d, v, ob = state[name]
                runs[name].append(run(m, d, v, a.steps, ob))
        for name in ("closed", "open"):
            us = sorted(r["us_per_host_iteration"] for r in runs[name])
            med = sorted(runs[name], key=lambda r: r["us_per_host_iteration"])[len(us) // 2]
            rec = dict(shape=list(shape), B=B, path=name, open_bound=state[name][2], us_min=us[0], us_max=us[-1], **med)
            out.append(rec)
            print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
