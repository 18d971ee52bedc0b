"""Timing probe of the liquid solver step (profiles/liquid.md): the drop-into-a-basin scene of scene/liquid_pos_size.py at 128x64 with one
N-group (B = the scenes that seed as many particles as the first one) and the two-drop scene of scene/liquid3_d_r.py at 96x48x96 with
B = 1.

    python tools/liquid_probe.py [--steps 16] [--warm 4] [--out FILE.json]

Reported: wall milliseconds per step around a synchronised run of ``steps`` steps from the state after ``warm`` steps; wall milliseconds
per kernel class, from wall clock between synchronisations around every C-ABI call of a SECOND, instrumented run (the synchronisations
cost time of their own, so the classes do not add up to the first figure); the CG iterations per solve.  Nothing here is a pass / fail
number."""
import argparse
import collections
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import _lib, ops  # noqa: E402

CLASSES = [("df_particles_advect", "trace"), ("df_particles_cell_keys", "keys"), ("df_particles_gather", "gather"),
           ("df_liquid_p2g", "p2g"), ("df_mac_extrapolate", "extrapolate"), ("df_liquid_flags", "flags"), ("df_liquid_forces", "forces"),
           ("df_pressure_init", "cg_init"), ("df_pressure_cg_direction", "cg_direction"), ("df_pressure_cg_update", "cg_update"),
           ("df_pressure_status", "cg_status"), ("df_pressure_correct", "correct"), ("df_flip_update", "flip_update")]


class Timed(object):
    """every C-ABI call between two synchronisations, wall clock per class"""

    def __enter__(self):
        self.ms = collections.OrderedDict((c, 0.0) for _, c in CLASSES)
        self.ms["other"] = 0.0
        self.real = ops.call

        def call(name, *args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.real(name, *args)
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            for prefix, cls in CLASSES:
                if name.startswith(prefix):
                    self.ms[cls] += dt
                    return
            self.ms["other"] += dt

        ops.call = call
        return self

    def __exit__(self, *exc):
        ops.call = self.real


def scene2d(X=128, Y=64):
    basin = ops.box_levelset((Y, X), (0.0, 0.0), (X * 1.0, Y * 0.2))
    states = []
    for px in np.linspace(0.2, 0.8, 10):
        c = (X * px, Y * 0.6)
        phi = np.minimum(basin, ops.sphere_levelset((Y, X), c, X * 0.06))
        states.append(ops.liquid_initial_state((Y, X), phi, [(c, X * 0.11)]))
    n0 = states[0][0].shape[1]
    group = [s for s in states if s[0].shape[1] == n0]
    return [torch.cat([s[k] for s in group]) for k in range(3)]


def scene3d(X=96, Y=48, Z=96):
    shape = (Z, Y, X)
    phi = ops.box_levelset(shape, (0.0, 0.0, 0.0), (X * 1.0, Y * 0.2, Z * 1.0))
    cs = [(X * 0.5 + X * 0.2, Y * 0.6, Z * 0.5), (X * 0.5 - X * 0.2, Y * 0.6, Z * 0.5)]
    for c in cs:
        phi = np.minimum(phi, ops.sphere_levelset(shape, c, X * 0.1))
    return list(ops.liquid_initial_state(shape, phi, [(c, X * 0.15) for c in cs]))


def run(state, steps, dt):
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for last in ops.simulate_liquid(state[0], state[1], state[2], steps, dt=dt, stack=False, stats=stats):
        pass
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    iters = torch.stack(stats).cpu().numpy()
    return last, dict(ms_per_step=1e3 * wall / steps, iters_min=int(iters.min()), iters_median=float(np.median(iters)), iters_max=int(iters.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for name, make, dt in (("128x64", scene2d, 0.5), ("96x48x96", scene3d, 0.8)):
        state = make()
        warm, _ = run(state, a.warm, dt)
        state = [t.clone() for t in warm]
        _, rec = run(state, a.steps, dt)
        with Timed() as tm:
            run(state, a.steps, dt)
        rec.update(scene=name, B=int(state[0].shape[0]), N=int(state[0].shape[1]), steps=a.steps,
                   ms_per_step_by_class={k: v / a.steps for k, v in tm.ms.items()})
        print(json.dumps(rec))
        out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
