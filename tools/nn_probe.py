#!/usr/bin/env python
"""Measures the latent-space integrator (csrc/nn.hip; the table of profiles/nn.md).

    python tools/nn_probe.py resources
        compiles nn.hip with -Rpass-analysis=kernel-resource-usage and prints registers, LDS and spills per kernel (needs no GPU)
    python tools/nn_probe.py time [--iters 20] [--warmup 5] [--scenes 10] [--frames 400]
        on an MI355X, at the reference's shape (z_num 16, p_num 2, filters 512, B 1024, w_size 30): ms per train step, split by a
        KernelTimer into the linear layers (df_linear_*) and the new kernels (df_nn_*); the same graph composed from PyTorch-ROCm's own
        ops; ms for the rollout as one launch and as a host loop over the inference ops.  Median of --iters after --warmup, HIP events.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, P, FILTERS, B, W = 16, 2, 512, 1024, 30


def resources():
    src = os.path.join(ROOT, "deep_fluids_amd", "csrc", "nn.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True, check=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"\d+([a-z_]+_kernel)", m.group(1))
            cur = {"kernel": name.group(1) if name else m.group(1)}
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    print("| kernel | VGPRs | SGPRs | static LDS (B) | scratch (B/lane) | spills (V/S) | waves/SIMD |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if r["kernel"] != "zero_words_kernel":
            print("| `%(kernel)s` | %(vgpr)d | %(sgpr)d | %(lds)d | %(scratch)d | %(vspill)d / %(sspill)d | %(occ)d |" % r)


def _median_ms(torch, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def _torch_step(torch, filters):
    """the same graph from PyTorch-ROCm's own ops (its dropout draws its own masks): forward, backward, Adam"""
    nn, F = torch.nn, torch.nn.functional
    net = nn.Sequential(nn.Linear(Z + P, 2 * filters), nn.BatchNorm1d(2 * filters, eps=1e-5, momentum=0.1), nn.ELU(), nn.Dropout(0.9),
                        nn.Linear(2 * filters, filters), nn.BatchNorm1d(filters, eps=1e-5, momentum=0.1), nn.ELU(), nn.Dropout(0.9),
                        nn.Linear(filters, Z)).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.999))

    def step(xw, yw, ratio):
        opt.zero_grad(set_to_none=True)
        x_, ys = xw[:, 0], []
        for i in range(W):
            y = net(x_)
            ys.append(y)
            if i < W - 1:
                x_ = torch.cat([x_[:, :Z] + y * ratio, xw[:, i + 1, Z:]], dim=1)
        F.mse_loss(torch.stack(ys, dim=1), yw).backward()
        opt.step()
    return step


def timing(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from deep_fluids_amd import _lib, ops
    from deep_fluids_amd.trainer import NNTrainer, default_config
    bm = SimpleNamespace(code_std=np.float32(1.5), out_std=np.float32(0.3), p_num=P, epochs_per_step=1e-3)
    tr = NNTrainer(default_config(arch="nn", z_num=Z, filters=FILTERS, w_size=W, batch_size=B), bm)
    gen = torch.Generator(device="cuda").manual_seed(1)
    xw = torch.randn((B, W, Z + P), device="cuda", generator=gen)
    yw = torch.randn((B, W, Z), device="cuda", generator=gen)
    ours = _median_ms(torch, lambda: tr.train_step(xw, yw), a.iters, a.warmup)
    _lib.TIMER = _lib.KernelTimer(lambda name, args: (("linear" if name.startswith("df_linear") else "nn" if name.startswith("df_nn") else "other"), 0.0))
    tr.train_step(xw, yw)
    split = {k: v["seconds"] * 1e3 for k, v in _lib.TIMER.summary().items()}
    _lib.TIMER = None
    step = _torch_step(torch, FILTERS)
    theirs = _median_ms(torch, lambda: step(xw, yw, tr.ratio), a.iters, a.warmup)
    S, Fr = a.scenes, a.frames
    bm.x_test = torch.randn((S * (Fr - 1), Z + P), generator=torch.Generator().manual_seed(2)).numpy() * 0.5
    bm.y_test = torch.randn((S * (Fr - 1), Z), generator=torch.Generator().manual_seed(3)).numpy() * 0.5
    bm.num_test_scenes, bm.num_frames = S, Fr
    one = _median_ms(torch, lambda: tr.rollout(bm), max(a.iters // 4, 3), 1)
    xt, yt = torch.from_numpy(bm.x_test).cuda(), torch.from_numpy(bm.y_test).cuda()
    cs, os_ = float(bm.code_std), float(bm.out_std)

    def loop():          # every scene at once, one step per frame: the device work of the reference's loop, batched over the scenes
        rows = torch.arange(S, device="cuda") * (Fr - 1)
        xin = xt[rows]
        for t in range(Fr - 1):
            pred = tr.predict(xin) * os_ + xin[:, :Z] * cs
            pred[:, Z - P:] = (yt[rows + t] * os_ + xt[rows + t, :Z] * cs)[:, Z - P:]
            xin = torch.cat([pred / cs, xt[rows + min(t + 1, Fr - 2), Z:]], dim=1)
    host = _median_ms(torch, loop, max(a.iters // 4, 3), 1)
    print("| train step, ms | df_linear_*, ms | df_nn_*, ms | other C-ABI calls, ms | PyTorch-ROCm ops, ms |")
    print("|---|---|---|---|---|")
    print("| %.2f | %.2f | %.2f | %.2f | %.2f |" % (ours, split.get("linear", 0.0), split.get("nn", 0.0), split.get("other", 0.0), theirs))
    print("| rollout %d x %d, one launch, ms | host loop over the inference ops, ms |" % (S, Fr))
    print("|---|---|")
    print("| %.2f | %.2f |" % (one, host))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["resources", "time"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=10)
    ap.add_argument("--frames", type=int, default=400)
    args = ap.parse_args()
    resources() if args.what == "resources" else timing(args)
