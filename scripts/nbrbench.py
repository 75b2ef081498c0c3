#!/usr/bin/env python3
"""Swarm neighbour-search benchmark: tgms_neighbors_batch_device on
  (a) the README separation swarm, 1,024 x M = 10 in one 10 m room, r_min = 0.5, against what a
      caller does without it, in the same run: tgms_separation_batch_device over all 523,776
      unordered pairs plus a torch per-row reduction (count, nearest, lowest-j ties);
  (b) 65,536 x M = 10 at the same vehicle density: 64 such rooms on an 8 x 8 grid, 1,024
      vehicles each.  The all-pairs call is not run at this size; its time is an extrapolation
      from (a)'s time per pair and is labelled as one;
  (c) the worst case: swarm (a) with a horizon above every distance, so nothing is culled,
      against the same all-pairs call plus reduction.
All solved on the device, all start times 0.  Timed in alternating windows (device events
around NB_ITERS launches, NB_ROUNDS windows each, after a warm-up); the median window is
reported with its range.  The rows of (a) and (c) must equal the all-pairs reduction (count and
nbr exactly, d_min to 1e-9 L^2).  One JSON line per result on stdout and in NB_OUT (default
profiles/neighbors_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("NB_OUT", os.path.join(ROOT, "profiles", "neighbors_bench.jsonl"))
ROUNDS = int(os.environ.get("NB_ROUNDS", 5))
ITERS = int(os.environ.get("NB_ITERS", 3))
N_A, N_B = int(os.environ.get("NB_N", 1024)), int(os.environ.get("NB_NBIG", 65536))
R_MIN = float(os.environ.get("NB_RMIN", 0.5))
M = 10
ROOM = 10.0  # synthetic.uniform_batch: x, y in [-5, 5]
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


def solved(n, rooms=1):
    so, W, T = S.uniform_batch(n, M)
    if rooms > 1:  # vehicle b lives in room b // (n / rooms^2) of a rooms x rooms grid
        room = np.arange(n) // (n // (rooms * rooms))
        W[..., 0] += ROOM * (room % rooms)[:, None]
        W[..., 1] += ROOM * (room // rooms)[:, None]
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    return dT, dC, torch.from_numpy(so).cuda()


class Outs:
    def __init__(self, n):
        self.near = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        self.nbr, self.count, self.tested, self.flags = (torch.empty((n,), dtype=torch.int32, device="cuda")
                                                         for _ in range(4))

    def args(self):
        return self.near, self.nbr, self.count, self.tested, self.flags


def stats(name, v, extra=None):
    d = {"case": name, "M": M, "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "rounds": len(v)}
    d.update(extra or {})
    emit(d)
    return d


s = Solver(0)
# ---- (a), (c): one room ----
dT, dC, d_so = solved(N_A)
P_A = N_A * (N_A - 1) // 2
sep = torch.empty((P_A, 2), dtype=torch.float64, device="cuda")
iu = torch.triu_indices(N_A, N_A, offset=1, device="cuda")
o = Outs(N_A)
ref = {}


def all_pairs(r_min):
    s.separation_device(N_A, d_so, dT, dC, P_A, None, None, None, r_min, sep, None)
    D = torch.full((N_A, N_A), float("inf"), dtype=torch.float64, device="cuda")
    D[iu[0], iu[1]] = sep[:, 0]
    D[iu[1], iu[0]] = sep[:, 0]
    close = D < r_min
    ref["count"] = close.sum(dim=1).to(torch.int32)
    d, j = torch.where(close, D, float("inf")).min(dim=1)  # the first minimum: the lowest j
    ref["d"], ref["nbr"] = d, torch.where(ref["count"] > 0, j.to(torch.int32), -1)


for tag, r_min in (("a", R_MIN), ("c", 1.0e3)):
    run_n = lambda: s.neighbors_device(N_A, d_so, dT, dC, r_min, None, None, *o.args())
    run_p = lambda: all_pairs(r_min)
    for r in (run_n, run_p):
        for _ in range(2):
            r()
    torch.cuda.synchronize()
    ok = bool((o.count == ref["count"]).all()) and bool((o.nbr == ref["nbr"]).all())
    m = ref["count"] > 0
    err = float((o.near[m, 0] ** 2 - ref["d"][m] ** 2).abs().max()) if bool(m.any()) else 0.0
    share = float(o.tested.sum()) / (N_A * (N_A - 1))
    emit({"check": tag, "rows_equal_all_pairs": ok, "d2_abs_err": err, "within_r_min_rows": int(m.sum()),
          "tested_share": share, "r_min": r_min})
    ms = {"n": [], "p": []}
    for _ in range(ROUNDS):
        ms["n"].append(window(run_n, ITERS))
        ms["p"].append(window(run_p, ITERS))
    what = "one room, r_min %.3g" % r_min if tag == "a" else "one room, nothing culled"
    rn = stats("neighbors %d x M=%d, %s" % (N_A, M, what), ms["n"], {"tested_share": share, "iters": ITERS})
    rp = stats("all pairs + torch row reduction %d x M=%d" % (N_A, M), ms["p"], {"P": P_A, "iters": ITERS})
    emit({"case": tag, "all_pairs_over_neighbors": rp["ms"] / rn["ms"]})
    if tag == "a":
        ns_per_pair = rp["ms"] * 1e6 / P_A
del sep, o, dT, dC, d_so, iu
ref.clear()

# ---- (b): 64 rooms ----
rooms = int(round((N_B // N_A) ** 0.5))
dT, dC, d_so = solved(N_B, rooms)
o = Outs(N_B)
run_b = lambda: s.neighbors_device(N_B, d_so, dT, dC, R_MIN, None, None, *o.args())
run_b()
torch.cuda.synchronize()
share = float(o.tested.sum().to(torch.float64)) / (float(N_B) * (N_B - 1))
msb = [window(run_b, 1) for _ in range(min(ROUNDS, 3))]
P_B = N_B * (N_B - 1) // 2
stats("neighbors %d x M=%d, %d rooms, r_min %.3g" % (N_B, M, rooms * rooms, R_MIN), msb,
      {"tested_share": share, "tested": int(o.tested.sum().to(torch.int64)), "rows_close": int((o.count > 0).sum()),
       "nonfinite_rows": int((o.flags == 16).sum()), "iters": 1,
       "all_pairs_extrapolated_s": P_B * ns_per_pair * 1e-9,
       "extrapolated_from": "%.1f ns per pair measured in case a; the all-pairs call was not run at this size" % ns_per_pair})
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
