#!/usr/bin/env python3
"""Body-rate benchmark: tgms_rate_batch_device against tgms_thrust_batch_device on the same
batches and against what a caller had to do before it, tgms_sample_batch_device at 100 Hz plus a
torch reduction of ||f x j|| / ||f||^2 per trajectory, on two synthetic batches, 4,096 x M = 10
and 1,048,576 x M = 10, both solved on the device.  The samples of a batch do not fit the device
at once, so the sampled path runs in chunks of RB_CHUNK trajectories into one reused buffer; its
time is the sum over the chunks of the sampler launch and the reduction (device events per chunk;
the sample offsets and the segment index of the reduction are built outside the timed part).  The
three paths are timed in alternating windows of the same run after a warm-up, RB_ROUNDS windows
each at the small size and RB_ROUNDS_BIG at the large one; the median window is reported with the
spread.  Also reported: how far the sampled omega_max falls short of the continuous one, and how
far the bound a caller had without either, j_peak / f_min from the bounds and thrust records,
sits above it (median and worst ratio).  One JSON line per result on stdout and in RB_OUT
(default profiles/rate_bench.jsonl, rewritten).

Work per segment, worst case (every interval of every level bisected): BISECTIONS * sum_d d^2
Horner FMAs = 40 * 5,525 = 221,000, against the thrust call's 40 * (285 + 819) = 44,160: 5.0
times."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver, sample_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("RB_OUT", os.path.join(ROOT, "profiles", "rate_bench.jsonl"))
SIZES = [(int(os.environ.get("RB_N", 4096)), int(os.environ.get("RB_ITERS", 50)), int(os.environ.get("RB_ROUNDS", 5))),
         (int(os.environ.get("RB_NBIG", 1 << 20)), int(os.environ.get("RB_ITERS_BIG", 3)),
          int(os.environ.get("RB_ROUNDS_BIG", 2)))]
CHUNK = int(os.environ.get("RB_CHUNK", 4096))
M = 10; dt = 0.01; g = 9.80665
WORST_FMAS_PER_SEGMENT = 40 * 5525
results = []


def emit(d):
    print(json.dumps(d), flush=True)
    results.append(d)


s = Solver(0)
for n, iters, rounds in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    d_so = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * M).cuda()
    rec = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    seg = torch.empty((n * M, 2), dtype=torch.float64, device="cuda")
    fl = torch.empty((n,), dtype=torch.int32, device="cuda")
    trec = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    brec = torch.empty((n, 10), dtype=torch.float64, device="cuda")
    # the chunks of the sampled path: offsets on the host once, one output buffer for the largest
    so_c = np.arange(CHUNK + 1, dtype=np.int32) * M
    chunks = []
    for n0 in range(0, n, CHUNK):
        n1 = min(n, n0 + CHUNK)
        chunks.append((n0, n1, sample_offsets(so_c[:n1 - n0 + 1], T[n0:n1].reshape(-1), dt)))
    out = torch.empty((max(int(c[2][-1]) for c in chunks), 14), dtype=torch.float64, device="cuda")
    smp = torch.empty((n,), dtype=torch.float64, device="cuda")  # sampled omega_max
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
            a, j = out[:ns, 6:9], out[:ns, 9:12]
            fx, fy, fz = a[:, 0], a[:, 1], a[:, 2] + g
            cx, cy, cz = fy * j[:, 2] - fz * j[:, 1], fz * j[:, 0] - fx * j[:, 2], fx * j[:, 1] - fy * j[:, 0]
            w = torch.sqrt(cx * cx + cy * cy + cz * cz) / (fx * fx + fy * fy + fz * fz)
            smp[n0:n1] = torch.zeros((nc,), dtype=torch.float64, device="cuda").scatter_reduce_(0, idx, w, "amax")
            e1.record(); torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            del idx, d_offs, a, j, fx, fy, fz, cx, cy, cz, w
        return ms

    def window(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    rate_call = lambda: s.rate_device(n, d_so, dT, dC, g, 3.0, rec, seg, fl)
    thrust_call = lambda: s.thrust_device(n, d_so, dT, dC, g, None, trec, None)
    window(rate_call); window(thrust_call)  # warm-up
    if n <= CHUNK:
        sampled_pass()
    ms = {"rate": [], "thrust": [], "sampled": []}
    for _ in range(rounds):  # alternating windows
        ms["rate"].append(window(rate_call))
        ms["thrust"].append(window(thrust_call))
        ms["sampled"].append(sampled_pass())
    s.bounds_device(n, d_so, dT, dC, None, brec, None)
    torch.cuda.synchronize()
    short = rec[:, 0] - smp
    loose = (brec[:, 8] / trec[:, 0]) / rec[:, 0]
    emit({"check": "the sampled omega_max at 100 Hz and the bound j_peak / f_min against the continuous omega_max",
          "B": n, "finite": bool(torch.isfinite(rec).all() and torch.isfinite(seg).all()),
          "flagged_over_3_rad_s": int((fl != 0).sum()), "omega_max_median": float(rec[:, 0].median()),
          "omega_max_largest": float(rec[:, 0].max()), "sampled_short_max": float(short.max()),
          "sampled_short_rel_max": float((short / rec[:, 0]).max()),
          "continuous_below_sampled_worst": float(short.min()),
          "j_peak_over_f_min_ratio_median": float(loose.median()), "j_peak_over_f_min_ratio_max": float(loose.max()),
          "j_peak_over_f_min_ratio_min": float(loose.min())})
    v = ms["rate"]
    emit({"kernel": "rate", "B": n, "M": M, "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v),
          "iters": iters, "rounds": rounds,
          "worst_case_fma_frac": n * M * WORST_FMAS_PER_SEGMENT / (78.6e12 / 2) / (float(np.median(v)) * 1e-3)})
    v = ms["thrust"]
    emit({"kernel": "thrust", "B": n, "M": M, "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v),
          "iters": iters, "rounds": rounds})
    v = ms["sampled"]
    emit({"kernel": "sample + torch reduction", "B": n, "M": M, "dt": dt, "ms": float(np.median(v)), "ms_min": min(v),
          "ms_max": max(v), "rounds": rounds, "chunk": CHUNK, "chunks": len(chunks), "samples": total_samples})
    emit({"B": n, "rate_over_thrust": float(np.median(ms["rate"]) / np.median(ms["thrust"])),
          "sampled_over_continuous": float(np.median(ms["sampled"]) / np.median(ms["rate"]))})
    del dW, dT, dC, d_so, rec, seg, fl, trec, brec, out, smp
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
