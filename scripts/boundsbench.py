#!/usr/bin/env python3
"""Continuous-bounds benchmark: tgms_bounds_batch_device against the sampled check
tgms_extrema_batch_device at dt = 0.01 on the same two synthetic batches, 4,096 x M = 10 and
1,048,576 x M = 10, both solved on the device.  The two kernels are timed in alternating
windows of the same run (device events around BB_ITERS launches, BB_ROUNDS windows each; the
median window is reported with the spread), after a warm-up of both.  The continuous record
is also compared with the sampled one: it must dominate it (peaks not below, extents not
inside) up to 1e-9.  One JSON line per result on stdout and in BB_OUT (default
profiles/bounds_bench.jsonl, rewritten).

Work per segment of the continuous check, worst case (every interval of every ladder level
bisected): BISECTIONS * sum_d d^2 Horner FMAs = 40 * (3 * 91 + 506 + 285 + 140) = 48,160; an
interval with no sign change costs one Horner evaluation instead of 41."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import Limits
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("BB_OUT", os.path.join(ROOT, "profiles", "bounds_bench.jsonl"))
SIZES = [(int(os.environ.get("BB_N", 4096)), int(os.environ.get("BB_ITERS", 50))),
         (int(os.environ.get("BB_NBIG", 1 << 20)), int(os.environ.get("BB_ITERS_BIG", 3)))]
ROUNDS = int(os.environ.get("BB_ROUNDS", 5))
M = 10; dt = 0.01
WORST_FMAS_PER_SEGMENT = 40 * (3 * 91 + 506 + 285 + 140)
results = []


def emit(d):
    print(json.dumps(d), flush=True)
    results.append(d)


def window(run, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


s = Solver(0)
lim = Limits(pmin=[-5.5, -5.5, 0.0], pmax=[5.5, 5.5, 5.5], v_max=3.0, a_max=6.0, j_max=30.0)
for n, iters in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    d_so = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * M).cuda()
    ext = {k: torch.empty((n, 10), dtype=torch.float64, device="cuda") for k in ("bounds", "extrema")}
    fl = {k: torch.empty((n,), dtype=torch.int32, device="cuda") for k in ("bounds", "extrema")}
    runs = {"bounds": lambda: s.bounds_device(n, d_so, dT, dC, lim, ext["bounds"], fl["bounds"]),
            "extrema": lambda: s.extrema_device(n, d_so, dW, dT, dC, dt, lim, ext["extrema"], fl["extrema"])}
    for r in runs.values():  # warm-up of both
        for _ in range(2):
            r()
    torch.cuda.synchronize()
    c, e = ext["bounds"], ext["extrema"]
    slack = 1e-9 * c[:, 0:6].abs().max(dim=1, keepdim=True).values
    emit({"check": "continuous record dominates the sampled one", "B": n,
          "peaks_ok": bool((c[:, 6:9] >= e[:, 6:9] * (1 - 1e-9)).all()),
          "extents_ok": bool((c[:, 0:3] <= e[:, 0:3] + slack).all() and (c[:, 3:6] >= e[:, 3:6] - slack).all()),
          "duration_equal": bool(torch.equal(c[:, 9], e[:, 9])),
          "peaks_max_rel_gain": float(((c[:, 6:9] - e[:, 6:9]) / e[:, 6:9]).max()),
          "flagged_bounds": int((fl["bounds"] != 0).sum()), "flagged_extrema": int((fl["extrema"] != 0).sum())})
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):  # alternating windows
        for k, r in runs.items():
            ms[k].append(window(r, iters))
    for k, v in ms.items():
        d = {"kernel": k, "B": n, "M": M, "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v),
             "iters": iters, "rounds": ROUNDS}
        if k == "extrema":
            d["dt"] = dt
        else:
            d["worst_case_fma_frac"] = n * M * WORST_FMAS_PER_SEGMENT / (78.6e12 / 2) / (d["ms"] * 1e-3)
        emit(d)
    emit({"B": n, "sampled_over_continuous": float(np.median(ms["extrema"]) / np.median(ms["bounds"]))})
    del dW, dT, dC, d_so, ext, fl
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
