"""Timing probe of the surface mesher (profiles/liquid_mesh.md): the count and emit passes of ``ops.extract_surface`` on the union level
set of a dam-break state -- the 3-D scene of tools/liquid_probe.py after ``warm`` liquid steps -- at 96x48x96 (B = 1) and 128^3 (B = 4:
the one simulated entry's level set four times; the kernels do not look across entries).

    python tools/liquid_mesh_probe.py [--warm 4] [--launches 20] [--repeats 5] [--out FILE.json]

Per scene: HIP-event milliseconds per launch of ``df_mesh_count`` and ``df_mesh_emit`` (closed, bnd = 1, without and with normals), each
window ``launches`` back-to-back launches after one untimed launch, the windows interleaved count, emit, emit+normals, count, ... and
repeated ``repeats`` times: median [min - max].  Beside each the algorithmic bytes -- phi once per pass, the mask byte, the two count
bytes resp. the two int32 offsets, the outputs -- and bytes / time against the 8 TB/s of the specification.  The emit pass reads phi only
at samples that own a vertex, so its real traffic is below that accounting; the figure is the issue's yardstick, not a counter.  Also
the wall time of one whole ``extract_surface`` (count, two scans, the host's read of the totals, allocation, emit).  Nothing here is a
pass / fail number."""
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
from deep_fluids_amd._lib import call  # noqa: E402
from deep_fluids_amd.ops import _ptr, _stream  # noqa: E402

SPEC_BYTES_PER_S = 8e12


def level_set(X, Y, Z, warm, dt, copies):
    state = lp.scene3d(X, Y, Z)
    if warm:
        state, _ = lp.run(state, warm, dt)
    phi = ops.particle_levelset(state[0], (Z, Y, X))
    return phi.repeat(copies, 1, 1, 1).contiguous()


def window(fn, launches):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def summary(ms, nbytes):
    med = float(np.median(ms))
    return dict(ms_median=med, ms_min=float(min(ms)), ms_max=float(max(ms)), bytes=int(nbytes), gb_per_s=nbytes / (med * 1e-3) / 1e9,
                share_of_spec=nbytes / (med * 1e-3) / SPEC_BYTES_PER_S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for name, (X, Y, Z), copies in (("96x48x96", (96, 48, 96), 1), ("128x128x128", (128, 128, 128), 4)):
        phi = level_set(X, Y, Z, a.warm, 0.8, copies)
        dims = [int(v) for v in phi.shape]
        n = int(phi.numel())
        tail = [1, 1, 0.5, _stream()]
        t0 = time.perf_counter()
        mesh = ops.extract_surface(phi, bnd=1, closed=True, normals=True)
        torch.cuda.synchronize()
        first_wall = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        mesh = ops.extract_surface(phi, bnd=1, closed=True, normals=True)
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        V, T = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        mask = torch.empty((n,), dtype=torch.uint8, device=phi.device)
        counts = torch.empty((2, n), dtype=torch.uint8, device=phi.device)
        off = torch.zeros((2, n + 1), dtype=torch.int32, device=phi.device)
        call("df_mesh_count", _ptr(phi), _ptr(mask), _ptr(counts[0]), _ptr(counts[1]), *(dims + tail))
        off[:, 1:] = torch.cumsum(counts, 1, dtype=torch.int32)
        verts, nrm = torch.empty_like(mesh.vertices), torch.empty_like(mesh.vertices)
        faces = torch.empty_like(mesh.faces)

        def count():
            call("df_mesh_count", _ptr(phi), _ptr(mask), _ptr(counts[0]), _ptr(counts[1]), *(dims + tail))

        def emit(normals):
            call("df_mesh_emit", _ptr(phi), _ptr(mask), _ptr(off[0]), _ptr(off[1]), _ptr(verts), _ptr(nrm) if normals else None, _ptr(faces),
                 V, T, *(dims + tail))

        passes = (("count", count), ("emit", lambda: emit(False)), ("emit_normals", lambda: emit(True)))
        ms = {k: [] for k, _ in passes}
        for _ in range(a.repeats):
            for k, fn in passes:
                ms[k].append(window(fn, a.launches))
        assert torch.equal(verts, mesh.vertices) and torch.equal(faces, mesh.faces) and torch.equal(nrm, mesh.normals)
        emit_bytes = 4 * n + n + 8 * (n + 1) + 12 * V + 12 * T
        rec = dict(scene=name, B=dims[0], samples=n, vertices=V, faces=T, launches=a.launches, repeats=a.repeats,
                   extract_surface_wall_ms=wall, extract_surface_first_wall_ms=first_wall,
                   count=summary(ms["count"], 4 * n + 3 * n), emit=summary(ms["emit"], emit_bytes),
                   emit_normals=summary(ms["emit_normals"], emit_bytes + 12 * V))
        print(json.dumps(rec))
        out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
