#!/usr/bin/env python3
"""Swarm-separation benchmark: tgms_separation_batch_device on
  (a) all 523,776 pairs of a 1,024-trajectory x M = 10 swarm (pairs == NULL, decoded on the device),
  (b) 1,048,576 explicit random pairs over 65,536 x M = 10,
both solved on the device, all start times 0.  In the same run, as the comparison, the sampled
formulation a caller has today on case (a)'s swarm: tgms_sample_batch_device at 100 Hz, the
samples padded per trajectory with its held end point, and a torch min over the per-sample
distances of SB_SAMPLED_PAIRS pairs at once (default 8,192: the gathered positions of a pair are
2 x 24 B per sample, 3.2 GB here, and the temporaries as much again; the cost per pair is what
is compared).  Timed
in alternating windows (device events around SB_ITERS launches, SB_ROUNDS windows each; the
median window is reported with the spread) after a warm-up.  The continuous d_min must not
exceed the sampled one by more than 1e-9.  One JSON line per result on stdout and in SB_OUT
(default profiles/separation_bench.jsonl, rewritten).

Work per (pair, interval) item, worst case (every interval of every ladder level bisected):
BISECTIONS * sum_{d<=13} d^2 = 40 * 819 = 32,760 Horner FMAs; M = 10 on both sides with
distinct knots is 21 items a pair."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver, sample_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("SB_OUT", os.path.join(ROOT, "profiles", "separation_bench.jsonl"))
ROUNDS = int(os.environ.get("SB_ROUNDS", 5))
ITERS = int(os.environ.get("SB_ITERS", 3))
N_A = int(os.environ.get("SB_N", 1024))
N_B, P_B = int(os.environ.get("SB_NBIG", 65536)), int(os.environ.get("SB_PBIG", 1 << 20))
P_S = int(os.environ.get("SB_SAMPLED_PAIRS", 8192))
M = 10; dt = 0.01
WORST_FMAS_PER_ITEM = 40 * 819
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


def solved(n):
    so, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    return so, T, dW, dT, dC, torch.from_numpy(so).cuda()


def stats(name, v, P, items, extra=None):
    d = {"case": name, "P": P, "M": M, "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v),
         "iters": ITERS, "rounds": ROUNDS}
    d["us_per_pair"] = d["ms"] * 1e3 / P
    if items:
        d["items"] = items
        d["worst_case_fma_frac"] = items * WORST_FMAS_PER_ITEM / (78.6e12 / 2) / (d["ms"] * 1e-3)
    d.update(extra or {})
    emit(d)
    return d


s = Solver(0)
# ---- (a) all pairs of N_A trajectories, and the sampled formulation on the same swarm ----
so, T, dW, dT, dC, d_so = solved(N_A)
P_A = N_A * (N_A - 1) // 2
sep = torch.empty((P_A, 2), dtype=torch.float64, device="cuda")
fl = torch.empty((P_A,), dtype=torch.int32, device="cuda")
run_a = lambda: s.separation_device(N_A, d_so, dT, dC, P_A, None, None, None, 0.5, sep, fl)

offs = sample_offsets(so, T.reshape(-1), dt)
d_offs = torch.from_numpy(offs).cuda()
smp = torch.empty((int(offs[-1]), 14), dtype=torch.float64, device="cuda")
cnt = torch.from_numpy(np.diff(offs)).cuda()
Lmax = int(cnt.max())
iu = torch.triu_indices(N_A, N_A, offset=1, device="cuda")  # the all-pairs order
P_S = min(P_S, P_A)
pi, pj = iu[0, :P_S], iu[1, :P_S]
k = torch.arange(Lmax, device="cuda")
d_smp = torch.empty((P_S,), dtype=torch.float64, device="cuda")


def run_sampled():
    s.sample_device(N_A, d_so, dW, dT, dC, dt, d_offs, smp)
    # sample k of trajectory b, its last sample held past its end: [P_S, Lmax, 3] per side
    gi = d_offs[pi][:, None] + torch.minimum(k[None, :], cnt[pi][:, None] - 1)
    gj = d_offs[pj][:, None] + torch.minimum(k[None, :], cnt[pj][:, None] - 1)
    d = smp[:, :3][gi] - smp[:, :3][gj]
    d_smp.copy_((d * d).sum(dim=2).min(dim=1).values)


for r in (run_a, run_sampled):
    for _ in range(2):
        r()
torch.cuda.synchronize()
# every padded sample is the held position at its grid time (the last sample's time is >= the duration)
dc, ds = sep[:P_S, 0], d_smp.sqrt()
emit({"check": "continuous d_min <= sampled d_min + 1e-9", "pairs": P_S,
      "ok": bool((dc <= ds + 1e-9).all()), "nonfinite": int((fl != 0).sum() - (fl == 1).sum()),
      "close_at_0.5": int((fl == 1).sum()), "max_gain": float((ds - dc).max()), "median_gain": float((ds - dc).median())})
ms = {"a": [], "sampled": []}
for _ in range(ROUNDS):
    ms["a"].append(window(run_a, ITERS))
    ms["sampled"].append(window(run_sampled, ITERS))
items_a = P_A * (2 * M + 1)
ra = stats("all pairs of %d x M=%d (pairs NULL)" % (N_A, M), ms["a"], P_A, items_a)
rs = stats("sampled at 100 Hz + torch min, %d x M=%d swarm" % (N_A, M), ms["sampled"], P_S, 0,
           {"dt": dt, "samples": int(offs[-1]), "longest": Lmax})
emit({"sampled_over_continuous_per_pair": rs["us_per_pair"] / ra["us_per_pair"]})
del sep, fl, smp, dW, dT, dC

# ---- (b) explicit random pairs over N_B trajectories ----
so, T, dW, dT, dC, d_so = solved(N_B)
rng = np.random.default_rng(12)
pairs = rng.integers(0, N_B, (P_B, 2)).astype(np.int32)
d_pairs = torch.from_numpy(pairs).cuda()
sep = torch.empty((P_B, 2), dtype=torch.float64, device="cuda")
fl = torch.empty((P_B,), dtype=torch.int32, device="cuda")
run_b = lambda: s.separation_device(N_B, d_so, dT, dC, P_B, d_pairs, None, None, 0.5, sep, fl)
for _ in range(2):
    run_b()
torch.cuda.synchronize()
msb = [window(run_b, ITERS) for _ in range(ROUNDS)]
stats("%d random pairs over %d x M=%d" % (P_B, N_B, M), msb, P_B, P_B * (2 * M + 1),
      {"flagged_nonfinite": int((fl == 16).sum()), "close_at_0.5": int((fl == 1).sum())})
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
