"""Timing probe of the implicit velocity diffusion (profiles/diffuse.md) at the size of scene/liquid3_vis.py: 96x72x48 ([Z,Y,X] =
48x72x96), B = 4 entries with the script's four alphas (0.02304 ... 23.04), a seeded random-normal velocity.

    python tools/diffuse_probe.py [--reps 5] [--iters 64] [--out FILE.json]

Reported, each as min / median / max over ``reps`` synchronised repeats after one warm-up:
  solve        wall milliseconds of ``ops.diffuse_velocity`` at accuracy 1e-4 and the default cap, and the iterations of every pair;
  per iteration  wall milliseconds of a run of exactly ``iters`` iterations (accuracy 0, every entry at alpha = 23.04: no pair stops
               early) over ``iters``, for the diffusion (B*D = 12 systems) and, beside it, for ``ops.solve_pressure_liquid`` on the same
               grid with the scene's box as the liquid (B = 4 systems), and both divided by the unknowns (interior cells x systems;
               liquid cells x entries) and by the cells the kernels walk (all cells x systems).
Host word reads every ``check_every`` iterations are inside all of these, as they are inside a step.  Nothing here is a pass / fail
number."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_fluids_amd import ops  # noqa: E402

SHAPE = (48, 72, 96)
B = 4


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, dict(min=min(ms), median=float(np.median(ms)), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Z, Y, X = SHAPE
    D = 3
    vis_list = 2 * np.logspace(-5, -2, 4)
    alphas = [ops.diffusion_alpha(float(v), 0.125, X) for v in vis_list]
    rng = np.random.RandomState(0)
    vel = torch.from_numpy(rng.standard_normal((B,) + SHAPE + (D,)).astype(np.float32)).cuda()
    ws = ops.diffusion_workspace(vel)
    ncell = Z * Y * X
    interior = (Z - 2) * (Y - 2) * (X - 2)
    rec = dict(shape=list(SHAPE), B=B, alphas=alphas, reps=a.reps, iters=a.iters)

    (_, it), rec["solve_ms"] = timed(lambda: ops.diffuse_velocity(vel, alphas, workspace=ws), a.reps)
    rec["solve_iterations"] = it.cpu().numpy().tolist()
    rec["default_cap"] = ops.default_diffusion_max_iter(SHAPE)

    # every entry at the largest alpha: at the small ones the recurrence's residual underflows to 0 within ``iters`` and the pair stops
    (_, it), t = timed(lambda: ops.diffuse_velocity(vel, alphas[-1], accuracy=0.0, max_iter=a.iters, workspace=ws), a.reps)
    assert int(it.min()) == a.iters == int(it.max()), it
    d = {k: v / a.iters for k, v in t.items()}
    rec["diffusion_ms_per_iteration"] = d
    rec["diffusion_ns_per_iteration_per_unknown"] = 1e6 * d["median"] / (B * D * interior)
    rec["diffusion_ns_per_iteration_per_cell"] = 1e6 * d["median"] / (B * D * ncell)

    # the pressure solve beside it: the scene's box as the liquid, a walled random velocity
    phi = ops.box_levelset(SHAPE, (X * 0.3, 0.0, Z * 0.3), (X * 0.7, Y * 0.8, Z * 0.7))
    p, _, _ = ops.liquid_initial_state(SHAPE, phi)
    p = torch.cat([p] * B)
    _, cell_start, _ = ops.particle_cells(p, SHAPE)
    flags, _ = ops.liquid_flags(cell_start, SHAPE, B, p.shape[1])
    liquid = int((flags & 1).sum().item()) // B
    walled = ops.liquid_forces(vel, flags, (0.0, 0.0, 0.0))
    pws = ops.pressure_workspace(vel)
    (_, _, it), t = timed(lambda: ops.solve_pressure_liquid(walled, flags, accuracy=0.0, max_iter=a.iters, workspace=pws), a.reps)
    assert int(it.min()) == a.iters == int(it.max()), it
    q = {k: v / a.iters for k, v in t.items()}
    rec["pressure_ms_per_iteration"] = q
    rec["pressure_liquid_cells_per_entry"] = liquid
    rec["pressure_ns_per_iteration_per_unknown"] = 1e6 * q["median"] / (B * liquid)
    rec["pressure_ns_per_iteration_per_cell"] = 1e6 * q["median"] / (B * ncell)
    rec["ratio_per_iteration"] = d["median"] / q["median"]
    rec["ratio_per_iteration_per_unknown"] = rec["diffusion_ns_per_iteration_per_unknown"] / rec["pressure_ns_per_iteration_per_unknown"]
    rec["ratio_per_iteration_per_cell"] = rec["diffusion_ns_per_iteration_per_cell"] / rec["pressure_ns_per_iteration_per_cell"]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
