#!/usr/bin/env python3
"""Thrust and tilt benchmark: tgms_thrust_batch_device against what a caller had to do before it,
tgms_sample_batch_device at 100 Hz plus a torch reduction of ||a + g e_z|| and of the tilt per
trajectory, on the same two synthetic batches, 4,096 x M = 10 and 1,048,576 x M = 10, both solved
on the device.  The samples of a batch do not fit the device at once (about 5,500 samples of
112 B per trajectory), so the sampled path runs in chunks of TB_CHUNK trajectories into one
reused buffer; its time is the sum over the chunks of the sampler launch and the reduction
(device events per chunk; the sample offsets and the segment index of the reduction are built
outside the timed part).  The two paths are timed in alternating windows of the same run after a
warm-up of both, TB_ROUNDS windows each at the small size and TB_ROUNDS_BIG at the large one; the
median window is reported with the spread.  The sampled extremes are compared with the
continuous record: how far the sampled f_max and tilt_max fall short and the sampled f_min
stays above.  One JSON line per result on stdout and in TB_OUT (default
profiles/thrust_bench.jsonl, rewritten).

Work per segment of the continuous check, worst case (every interval of every level of both
ladders bisected): BISECTIONS * sum_d d^2 Horner FMAs = 40 * (285 + 819) = 44,160."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import ThrustLimits
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver, sample_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("TB_OUT", os.path.join(ROOT, "profiles", "thrust_bench.jsonl"))
SIZES = [(int(os.environ.get("TB_N", 4096)), int(os.environ.get("TB_ITERS", 50)), int(os.environ.get("TB_ROUNDS", 5))),
         (int(os.environ.get("TB_NBIG", 1 << 20)), int(os.environ.get("TB_ITERS_BIG", 3)),
          int(os.environ.get("TB_ROUNDS_BIG", 2)))]
CHUNK = int(os.environ.get("TB_CHUNK", 4096))
M = 10; dt = 0.01; g = 9.80665
WORST_FMAS_PER_SEGMENT = 40 * (285 + 819)
results = []


def emit(d):
    print(json.dumps(d), flush=True)
    results.append(d)


s = Solver(0)
lim = ThrustLimits(f_min=4.0, f_max=16.0, tilt_max=0.5)
for n, iters, rounds in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    d_so = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * M).cuda()
    rec = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    fl = torch.empty((n,), dtype=torch.int32, device="cuda")
    # the chunks of the sampled path: offsets on the host once, one output buffer for the largest
    so_c = np.arange(CHUNK + 1, dtype=np.int32) * M
    chunks = []
    for n0 in range(0, n, CHUNK):
        n1 = min(n, n0 + CHUNK)
        offs = sample_offsets(so_c[:n1 - n0 + 1], T[n0:n1].reshape(-1), dt)
        chunks.append((n0, n1, offs))
    out = torch.empty((max(int(c[2][-1]) for c in chunks), 14), dtype=torch.float64, device="cuda")
    smp = torch.empty((n, 3), dtype=torch.float64, device="cuda")  # sampled f_min f_max tilt_max
    total_samples = int(sum(int(c[2][-1]) for c in chunks))

    def sampled_pass():
        """Sampler + reduction over every chunk; returns the summed device time in ms."""
        ms = 0.0
        for n0, n1, offs in chunks:
            nc, ns = n1 - n0, int(offs[-1])
            d_offs = torch.from_numpy(offs).cuda()
            idx = torch.repeat_interleave(torch.arange(nc, device="cuda"), torch.from_numpy(np.diff(offs)).cuda())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.sample_device(nc, d_so[:nc + 1], dW[n0:n1], dT[n0:n1], dC[n0:n1], dt, d_offs, out)
            a = out[:ns, 6:9]
            fz = a[:, 2] + g
            h = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
            f = torch.sqrt(h + fz * fz)
            th = torch.atan2(torch.sqrt(h), fz)
            r = smp[n0:n1]
            r[:, 0] = torch.full((nc,), float("inf"), dtype=torch.float64, device="cuda").scatter_reduce_(0, idx, f, "amin")
            r[:, 1] = torch.zeros((nc,), dtype=torch.float64, device="cuda").scatter_reduce_(0, idx, f, "amax")
            r[:, 2] = torch.zeros((nc,), dtype=torch.float64, device="cuda").scatter_reduce_(0, idx, th, "amax")
            e1.record(); torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            del idx, d_offs, a, fz, h, f, th
        return ms

    def thrust_window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            s.thrust_device(n, d_so, dT, dC, g, lim, rec, fl)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    thrust_window()  # warm-up of both
    if n <= CHUNK:
        sampled_pass()
    ms = {"thrust": [], "sampled": []}
    for _ in range(rounds):  # alternating windows
        ms["thrust"].append(thrust_window())
        ms["sampled"].append(sampled_pass())
    short_hi = rec[:, 2] - smp[:, 1]
    short_tilt = rec[:, 4] - smp[:, 2]
    above_lo = smp[:, 0] - rec[:, 0]
    emit({"check": "how far the sampled extremes at 100 Hz fall short of the continuous record", "B": n,
          "finite": bool(torch.isfinite(rec).all()), "flagged": int((fl != 0).sum()),
          "f_max_short_max": float(short_hi.max()), "f_max_short_rel_max": float((short_hi / rec[:, 2]).max()),
          "f_min_above_max": float(above_lo.max()), "f_min_above_rel_max": float((above_lo / rec[:, 0]).max()),
          "tilt_short_max_rad": float(short_tilt.max()),
          "continuous_below_sampled_worst": float(min(short_hi.min(), short_tilt.min(), above_lo.min())),
          "f_min_least": float(rec[:, 0].min()), "f_max_largest": float(rec[:, 2].max()),
          "tilt_max_largest_rad": float(rec[:, 4].max())})
    v = ms["thrust"]
    emit({"kernel": "thrust", "B": n, "M": M, "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v),
          "iters": iters, "rounds": rounds,
          "worst_case_fma_frac": n * M * WORST_FMAS_PER_SEGMENT / (78.6e12 / 2) / (float(np.median(v)) * 1e-3)})
    v = ms["sampled"]
    emit({"kernel": "sample + torch reduction", "B": n, "M": M, "dt": dt, "ms": float(np.median(v)), "ms_min": min(v),
          "ms_max": max(v), "rounds": rounds, "chunk": CHUNK, "chunks": len(chunks), "samples": total_samples})
    emit({"B": n, "sampled_over_continuous": float(np.median(ms["sampled"]) / np.median(ms["thrust"]))})
    del dW, dT, dC, d_so, rec, fl, out, smp
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
