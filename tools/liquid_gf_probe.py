"""Timing probe of the liquid step with and without the ghost-fluid surface (profiles/liquid_gf.md): the scenes of tools/liquid_probe.py
(scene/liquid_pos_size.py at 128x64, scene/liquid3_d_r.py at 96x48x96), both variants started from the SAME state -- the one the
default step reaches after ``warm`` steps.

    python tools/liquid_gf_probe.py [--steps 16] [--warm 4] [--repeats 5] [--out FILE.json]

Reported per scene and variant: wall milliseconds per step around a synchronised run of ``steps`` steps, repeated ``repeats`` times from
that state after one untimed run (median, min and max of the repeats, in the order default, ghost fluid, default, ...: a drift of the
machine shows as a drift of both); the CG iterations per solve; and, for the ghost-fluid variant, wall milliseconds per kernel class
from a further, instrumented run with a synchronisation around every C-ABI call (the classes rank, they do not add up).  Nothing here
is a pass / fail number."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import liquid_probe as lp  # noqa: E402
from deep_fluids_amd import ops  # noqa: E402

lp.CLASSES[:0] = [("df_particle_levelset_averaged", "levelset"), ("df_levelset_smooth", "levelset_smooth")]


def run(state, steps, dt, ghost_fluid):
    import time
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in ops.simulate_liquid(state[0], state[1], state[2], steps, dt=dt, stack=False, stats=stats, ghost_fluid=ghost_fluid):
        pass
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    iters = torch.stack(stats).cpu().numpy()
    return 1e3 * wall / steps, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for name, make, dt in (("128x64", lp.scene2d, 0.5), ("96x48x96", lp.scene3d, 0.8)):
        warm, _ = lp.run(make(), a.warm, dt)
        state = [t.clone() for t in warm]
        ms = {False: [], True: []}
        iters = {}
        for gf in (False, True):
            run(state, a.steps, dt, gf)                                   # untimed: allocator, code objects
        for _ in range(a.repeats):
            for gf in (False, True):
                t, iters[gf] = run(state, a.steps, dt, gf)
                ms[gf].append(t)
        with lp.Timed() as tm:
            run(state, a.steps, dt, True)
        rec = dict(scene=name, B=int(state[0].shape[0]), N=int(state[0].shape[1]), steps=a.steps, repeats=a.repeats,
                   ghost_fluid_ms_per_step_by_class={k: v / a.steps for k, v in tm.ms.items()})
        for gf, key in ((False, "default"), (True, "ghost_fluid")):
            rec[key] = dict(ms_per_step_median=float(np.median(ms[gf])), ms_per_step_min=float(min(ms[gf])), ms_per_step_max=float(max(ms[gf])),
                            iters_min=int(iters[gf].min()), iters_median=float(np.median(iters[gf])), iters_max=int(iters[gf].max()))
        print(json.dumps(rec))
        out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
