#!/usr/bin/env python3
"""Feasibility-check benchmark: the fused extrema kernel (tgms_extrema_batch_device) against
the sampler kernel alone (tgms_sample_batch_device) on the sampler line's batch, 4,096 x
M = 10 at dt = 0.01.  The sampler alone is the baseline: before the fused kernel the only
route to extents and peaks was to sample (112 B per sample to HBM) and reduce afterwards.
The two are timed in alternating windows of the same run (device events around FB_ITERS
launches, FB_ROUNDS windows each; the median window is reported with the spread), after a
warm-up of both.  Then B = 1,048,576 x M = 10 runs once: its samples (~650 GB) could not
be stored at all.  One JSON line per result on stdout, and appended to FB_OUT if set.

Work per sample counted from the kernel: 66 Horner FMAs (4 chains x 3 axes), 9 for the
squared norms, 15 min / max, 3 for the sample time: 93 FP64 lane operations, against the
vector FP64 peak of 78.6 TFLOP/s = 39.3 T FMA lane-operations per second."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import Limits
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver, sample_offsets

ITERS = int(os.environ.get("FB_ITERS", 100)); ROUNDS = int(os.environ.get("FB_ROUNDS", 5))
N = int(os.environ.get("FB_N", 4096)); NBIG = int(os.environ.get("FB_NBIG", 1 << 20))
M = 10; dt = float(os.environ.get("FB_DT", 0.01))
PEAK_LANE_OPS = 78.6e12 / 2; OPS = 93; FMA_OPS = 66
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


def batch(s, n):
    _, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    so = np.arange(n + 1, dtype=np.int32) * M
    offs = sample_offsets(so, T.reshape(-1), dt)
    return torch.from_numpy(so).cuda(), dW, dT, dC, offs


s = Solver(0)
lim = Limits(pmin=[-5.5, -5.5, 0.0], pmax=[5.5, 5.5, 5.5], v_max=3.0, a_max=6.0, j_max=30.0)
d_so, dW, dT, dC, offs = batch(s, N)
ns = int(offs[-1])
d_offs = torch.from_numpy(offs).cuda()
out = torch.empty((ns, 14), dtype=torch.float64, device="cuda")
ext = torch.empty((N, 10), dtype=torch.float64, device="cuda")
fl = torch.empty((N,), dtype=torch.int32, device="cuda")
runs = {"sampler": lambda: s.sample_device(N, d_so, dW, dT, dC, dt, d_offs, out),
        "extrema": lambda: s.extrema_device(N, d_so, dW, dT, dC, dt, lim, ext, fl)}
for r in runs.values():  # warm-up of both shapes
    for _ in range(3):
        r()
torch.cuda.synchronize()
# the fused record against a reduction of the stored samples (same inputs, the timed size)
idx = torch.repeat_interleave(torch.arange(N, device="cuda"), torch.from_numpy(np.diff(offs)).cuda())
i3 = idx[:, None].expand(-1, 3)
lo = torch.full((N, 3), float("inf"), dtype=torch.float64, device="cuda").scatter_reduce_(0, i3, out[:, 0:3], "amin")
hi = torch.full((N, 3), float("-inf"), dtype=torch.float64, device="cuda").scatter_reduce_(0, i3, out[:, 0:3], "amax")
pk = torch.stack([torch.zeros(N, dtype=torch.float64, device="cuda").scatter_reduce_(
    0, idx, (out[:, 3 + 3 * q:6 + 3 * q] ** 2).sum(dim=1), "amax").sqrt() for q in range(3)], dim=1)
emit({"check": "extrema vs reduction of the sampler output", "extents_equal": bool(torch.equal(ext[:, 0:3], lo) and torch.equal(ext[:, 3:6], hi)),
      "peaks_max_rel": float(((ext[:, 6:9] - pk).abs() / pk).max()), "flagged": int((fl != 0).sum()), "B": N})
del idx, i3, lo, hi, pk
ms = {k: [] for k in runs}
for _ in range(ROUNDS):  # alternating windows
    for k, r in runs.items():
        ms[k].append(window(r, ITERS))
for k, v in ms.items():
    med = float(np.median(v))
    d = {"kernel": k, "B": N, "M": M, "dt": dt, "samples": ns, "ms": med, "ms_min": min(v), "ms_max": max(v),
         "iters": ITERS, "rounds": ROUNDS}
    if k == "sampler":
        d["GBs"] = ns * 112 / med / 1e6
    else:
        d["fp64_lane_ops_frac"] = ns * OPS / PEAK_LANE_OPS / (med * 1e-3)
        d["fp64_fma_frac"] = ns * FMA_OPS / PEAK_LANE_OPS / (med * 1e-3)
    emit(d)
emit({"speedup_fused_over_sampler_alone": float(np.median(ms["sampler"]) / np.median(ms["extrema"]))})
del out
if NBIG > 0:  # the batch whose samples could not be stored: once
    d_so, dW, dT, dC, offs = batch(s, NBIG)
    ns = int(offs[-1])
    ext = torch.empty((NBIG, 10), dtype=torch.float64, device="cuda")
    fl = torch.empty((NBIG,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t = window(lambda: s.extrema_device(NBIG, d_so, dW, dT, dC, dt, lim, ext, fl), 1)
    emit({"kernel": "extrema", "B": NBIG, "M": M, "dt": dt, "samples": ns, "ms": t, "runs": 1,
          "samples_bytes_if_stored": ns * 112, "fp64_lane_ops_frac": ns * OPS / PEAK_LANE_OPS / (t * 1e-3),
          "finite": bool(torch.isfinite(ext).all()), "flagged": int((fl != 0).sum())})
if os.environ.get("FB_OUT"):
    with open(os.environ["FB_OUT"], "a") as f:
        for d in results:
            f.write(json.dumps(d) + "\n")
