"""Timing probe of the multigrid-preconditioned liquid solves against the plain ones (profiles/liquid_mg.md): the scenes of
tools/liquid_probe.py (scene/liquid_pos_size.py at 128x64, scene/liquid3_d_r.py at 96x48x96), free surface and ghost fluid, and the
diffusion of tools/diffuse_probe.py (96x72x48, B = 4 with the script's four alphas).

    python tools/liquid_mg_probe.py [--steps 16] [--warm 4] [--repeats 5] [--out FILE.json]

Reported per scene and arm (``preconditioner=None``, the parent behaviour, against ``ops.Multigrid()``): wall milliseconds per step
around a synchronised run of ``steps`` steps from the SAME state (the one the default step reaches after ``warm`` steps), repeated
``repeats`` times after one untimed run with the arms interleaved, as median, min and max; the CG iterations per solve; and, separately,
the wall milliseconds of one hierarchy build (``out=``, no allocation).  For the diffusion: the whole solve per arm, the iterations of
every pair, and the build.  Nothing here is a pass / fail number."""
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


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def run(state, steps, dt, pre, ghost_fluid):
    stats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in ops.simulate_liquid(state[0], state[1], state[2], steps, dt=dt, stack=False, stats=stats, ghost_fluid=ghost_fluid, preconditioner=pre):
        pass
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return 1e3 * wall / steps, torch.stack(stats).cpu().numpy()


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    arms = (("plain", None), ("mg", ops.Multigrid()))
    for name, make, dt in (("128x64", lp.scene2d, 0.5), ("96x48x96", lp.scene3d, 0.8)):
        warm, _ = lp.run(make(), a.warm, dt)
        state = [t.clone() for t in warm]
        shape = tuple(state[2].shape[1:-1])
        for gf in (False, True):
            ms, iters = {k: [] for k, _ in arms}, {}
            for _, pre in arms:
                run(state, min(a.steps, 4), dt, pre, gf)                  # untimed: allocator, code objects
            for _ in range(a.repeats):
                for k, pre in arms:
                    t, iters[k] = run(state, a.steps, dt, pre, gf)
                    ms[k].append(t)
            rec = dict(scene=name, system="gf" if gf else "liquid", B=int(state[2].shape[0]), steps=a.steps, repeats=a.repeats)
            for k, _ in arms:
                rec[k] = dict(ms_per_step=spread(ms[k]), iters_min=int(iters[k].min()), iters_median=float(np.median(iters[k])),
                              iters_max=int(iters[k].max()))
            # the build alone: flags (and phi) of the state's own particles
            _, cell_start, _ = ops.particle_cells(state[0], shape)
            flags, _ = ops.liquid_flags(cell_start, shape, state[0].shape[0], state[0].shape[1])
            phi = ops.particle_levelset_averaged(state[0], shape) if gf else None
            h = ops.multigrid_hierarchy_liquid(state[2], flags, phi=phi)
            _, rec["hierarchy_build_ms"] = timed(lambda: ops.multigrid_hierarchy_liquid(state[2], flags, phi=phi, out=h), a.repeats)
            print(json.dumps(rec))
            out.append(rec)
    # the diffusion of tools/diffuse_probe.py
    shape, B = (48, 72, 96), 4
    alphas = [ops.diffusion_alpha(float(v), 0.125, shape[-1]) for v in 2 * np.logspace(-5, -2, 4)]
    vel = torch.from_numpy(np.random.RandomState(0).standard_normal((B,) + shape + (3,)).astype(np.float32)).cuda()
    ws = ops.diffusion_workspace(vel)
    h = ops.multigrid_hierarchy_diffusion(vel, alphas)
    rec = dict(scene="diffusion 96x72x48", B=B, alphas=alphas, repeats=a.repeats)
    for k, pre in (("plain", None), ("mg", h)):
        (_, it), rec[k + "_solve_ms"] = timed(lambda: ops.diffuse_velocity(vel, alphas, workspace=ws, preconditioner=pre), a.repeats)
        rec[k + "_iterations"] = it.cpu().numpy().tolist()
    _, rec["hierarchy_build_ms"] = timed(lambda: ops.multigrid_hierarchy_diffusion(vel, alphas, out=h), a.repeats)
    print(json.dumps(rec))
    out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
