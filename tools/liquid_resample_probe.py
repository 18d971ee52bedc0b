"""Timing probe of the liquid step with and without ``resample`` (profiles/liquid_resample.md): the scenes of tools/liquid_probe.py
(scene/liquid_pos_size.py at 128x64 with min_particles 2, scene/liquid3_d_r.py at 96x48x96 with min_particles 3), both variants
started from the SAME state -- the one the default step reaches after ``warm`` steps.  The default variant is the parent commit's step:
with ``resample=None`` nothing new is launched.

    python tools/liquid_resample_probe.py [--steps 16] [--warm 4] [--repeats 5] [--out FILE.json]

Reported per scene and variant: wall milliseconds per step around a synchronised run of ``steps`` steps, repeated ``repeats`` times from
that state after one untimed run (median, min and max of the repeats, in the order default, resample, default, ...: a drift of the
machine shows as a drift of both); the CG iterations per solve; the live particle count before and after the resampled run; and, for
the resampled variant, wall milliseconds per kernel class from a further, instrumented run with a synchronisation around every C-ABI
call (the classes rank, they do not add up; torch's sort and scan are not C-ABI calls and are not in them).  Nothing here is a pass /
fail number."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import liquid_probe as lp  # noqa: E402
from deep_fluids_amd import ops  # noqa: E402

lp.CLASSES[:0] = [("df_particle_levelset_averaged", "levelset"), ("df_levelset_smooth", "levelset_smooth"),
                  ("df_levelset_extrapolate", "levelset_extrapolate"), ("df_resample_count", "resample_count"),
                  ("df_resample_scatter", "resample_scatter")]


def run(state, steps, dt, min_particles):
    stats = []
    rs = None if min_particles is None else ops.Resample(min_particles)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for last in ops.simulate_liquid(state[0], state[1], state[2], steps, dt=dt, stack=False, stats=stats, resample=rs):
        pass
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    live = None if rs is None else int(last[3][-1].item())
    return 1e3 * wall / steps, torch.stack(stats).cpu().numpy(), live


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for name, make, dt, minp in (("128x64", lp.scene2d, 0.5, 2), ("96x48x96", lp.scene3d, 0.8, 3)):
        warm, _ = lp.run(make(), a.warm, dt)
        state = [t.clone() for t in warm]
        ms = {None: [], minp: []}
        iters, live = {}, {}
        for m in (None, minp):
            run(state, a.steps, dt, m)                                    # untimed: allocator, code objects
        for _ in range(a.repeats):
            for m in (None, minp):
                t, iters[m], live[m] = run(state, a.steps, dt, m)
                ms[m].append(t)
        with lp.Timed() as tm:
            run(state, a.steps, dt, minp)
        rec = dict(scene=name, B=int(state[0].shape[0]), N=int(state[0].shape[1]), steps=a.steps, repeats=a.repeats, min_particles=minp,
                   live_before=int(state[0].shape[0] * state[0].shape[1]), live_after=live[minp],
                   resample_ms_per_step_by_class={k: v / a.steps for k, v in tm.ms.items()})
        for m, key in ((None, "default"), (minp, "resample")):
            rec[key] = dict(ms_per_step_median=float(np.median(ms[m])), ms_per_step_min=float(min(ms[m])), ms_per_step_max=float(max(ms[m])),
                            iters_min=int(iters[m].min()), iters_median=float(np.median(iters[m])), iters_max=int(iters[m].max()))
        print(json.dumps(rec))
        out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
