#!/usr/bin/env python3
"""Time-dilation benchmark: tgms_dilate_batch_device on two synthetic batches, 4,096 x M = 10 and
1,048,576 x M = 10, both solved on the device, against
  (floor)  one tgms_bounds_batch_device + one tgms_thrust_batch_device call on the same batch: one
           evaluation of what the search evaluates, which the call cannot beat; reported with the
           mean and maximum number of evaluations per trajectory (flags >> DIL_EVALS_SHIFT);
  (before) what a caller had before the call: per step a torch pass that rescales the
           coefficients (c_k / s^k) and the times, both checks, and a per-trajectory bisection in
           lambda = 1 / s^2 updated in torch, until every bracket is 2^-41 wide like the call's.
Two sets of limits: "nominal" (v 3, a 6, j 30, f 4 / 16, tilt 0.5, s_lo = 1), under which most
synthetic rows are feasible or speed-limited and finish after one evaluation, and "hover" (f 9 /
10.5, tilt 0.1, s_lo = 0.25), under which every row runs the root search.  The three paths are
timed with device events in alternating windows of one run after a warm-up of each (DB_ROUNDS /
DB_ROUNDS_BIG windows; the median with the spread).  The output of the call is then checked with the
library's own bounds and thrust calls: the worst excess over a limit and the worst distance of the
active quantity from its limit.  One JSON line per result on stdout and in DB_OUT (default
profiles/dilate_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import DIL_EVALS_SHIFT, DIL_FLAG_MASK, Limits, ThrustLimits
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DB_OUT", os.path.join(ROOT, "profiles", "dilate_bench.jsonl"))
SIZES = [(int(os.environ.get("DB_N", 4096)), int(os.environ.get("DB_ITERS", 20)), int(os.environ.get("DB_ROUNDS", 5))),
         (int(os.environ.get("DB_NBIG", 1 << 20)), int(os.environ.get("DB_ITERS_BIG", 2)),
          int(os.environ.get("DB_ROUNDS_BIG", 2)))]
M = 10; g = 9.80665; S_HI = 100.0; INF = float("inf")
SETS = {"nominal": (3.0, 6.0, 30.0, 4.0, 16.0, 0.5, 1.0), "hover": (INF, INF, INF, 9.0, 10.5, 0.1, 0.25)}
results = []


def emit(d):
    print(json.dumps(d), flush=True)
    results.append(d)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


s = Solver(0)
for n, iters, rounds in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    d_so = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * M).cuda()
    ext = torch.empty((n, 10), dtype=torch.float64, device="cuda")
    rec = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    sc = torch.empty((n,), dtype=torch.float64, device="cuda")
    act = torch.empty((n,), dtype=torch.int32, device="cuda")
    fl = torch.empty((n,), dtype=torch.int32, device="cuda")
    dT2, dC2 = torch.empty_like(dT), torch.empty_like(dC)
    kpow = torch.arange(8, dtype=torch.float64, device="cuda")
    for name, (v, a, j, f_lo, f_hi, tilt, s_lo) in SETS.items():
        lk, lt = Limits(v_max=v, a_max=a, j_max=j), ThrustLimits(f_lo, f_hi, tilt)

        def call():
            s.dilate_device(n, d_so, dT, dC, g, lk, lt, s_lo, S_HI, sc, act, fl, dT2, dC2)

        def floor():
            s.bounds_device(n, d_so, dT, dC, None, ext, None)
            s.thrust_device(n, d_so, dT, dC, g, None, rec, None)

        def feasible(lam):
            """The caller's step: rescale in torch, run both checks, compare with the limits."""
            r = torch.sqrt(lam)
            torch.mul(dC, (r[:, None, None, None] ** kpow), out=dC2)
            torch.div(dT, r[:, None], out=dT2)
            s.bounds_device(n, d_so, dT2, dC2, None, ext, None)
            s.thrust_device(n, d_so, dT2, dC2, g, None, rec, None)
            return ((ext[:, 6] <= v) & (ext[:, 7] <= a) & (ext[:, 8] <= j) & (rec[:, 0] >= f_lo) & (rec[:, 2] <= f_hi)
                    & (rec[:, 4] <= tilt))

        steps = [0]

        def before():
            """Bisection per trajectory in lambda on [1 / s_hi^2, 1 / s_lo^2], all rows per step."""
            hi = torch.full((n,), 1.0 / s_lo ** 2, dtype=torch.float64, device="cuda")
            lo = torch.full((n,), 1.0 / S_HI ** 2, dtype=torch.float64, device="cuda")
            done = feasible(hi)          # feasible at s_lo
            lo = torch.where(done, hi, lo)
            done |= ~feasible(lo)        # capped
            k = 2
            while not bool(done.all()):
                mid = torch.where(hi > 4.0 * lo, torch.sqrt(lo * hi), 0.5 * (lo + hi))
                ok = feasible(mid)
                lo = torch.where(~done & ok, mid, lo)
                hi = torch.where(~done & ~ok, mid, hi)
                done |= (hi - lo) <= 2.0 ** -41 * hi
                k += 1
            steps[0] = k
            return lo

        call(); floor(); lam_before = before()  # warm-up of the three
        ms = {"call": [], "floor": [], "before": []}
        for _ in range(rounds):  # alternating windows
            ms["call"].append(window(call, iters))
            ms["floor"].append(window(floor, iters))
            ms["before"].append(window(before, 1))
        call(); torch.cuda.synchronize()
        ev = (fl >> DIL_EVALS_SHIFT).double()
        low = fl & DIL_FLAG_MASK
        usable = low == 0
        s_before = 1.0 / torch.sqrt(lam_before)
        # the output against the limits, by the library's own records of it
        s.bounds_device(n, d_so, dT2, dC2, None, ext, None)
        s.thrust_device(n, d_so, dT2, dC2, g, None, rec, None)
        F, fmin = rec[:, 2], rec[:, 0]
        exc = torch.stack([ext[:, 6] / v - 1, ext[:, 7] / a - 1, ext[:, 8] / j - 1, F / f_hi - 1, (f_lo - fmin) / F,
                           (rec[:, 4] - tilt) * fmin / F], dim=1)
        rel = exc.clone()
        rel[:, 4] = (f_lo - fmin) / f_lo
        col = torch.tensor([0, 0, 1, 2, 3, 4, 5], device="cuda")[act.long().clamp(min=0)]
        tight = torch.where(usable & (act > 0), rel.gather(1, col[:, None])[:, 0].abs(), torch.zeros_like(sc))
        emit({"check": "the call's output by the library's bounds and thrust records of it", "limits": name, "B": n,
              "usable": int(usable.sum()), "capped": int((low == 1).sum()), "nonfinite": int((low == 16).sum()),
              "feasible_excess_max": float(exc[usable].max()), "tight_deviation_max": float(tight.max()),
              "scale_min": float(sc[usable].min()), "scale_max": float(sc[usable].max()),
              "active_counts": [int((act == c).sum()) for c in range(7)],
              "scale_vs_torch_bisection_rel_max": float(((sc / s_before - 1).abs())[usable].max())})
        c, f, b = (float(np.median(ms[k])) for k in ("call", "floor", "before"))
        emit({"kernel": "dilate", "limits": name, "B": n, "M": M, "s_lo": s_lo, "s_hi": S_HI, "ms": c,
              "ms_min": min(ms["call"]), "ms_max": max(ms["call"]), "iters": iters, "rounds": rounds,
              "evals_mean": float(ev.mean()), "evals_max": int(ev.max()), "one_evaluation_share": float((ev == 1).double().mean())})
        emit({"kernel": "bounds + thrust, one evaluation", "limits": name, "B": n, "M": M, "ms": f, "ms_min": min(ms["floor"]),
              "ms_max": max(ms["floor"]), "iters": iters, "rounds": rounds})
        emit({"kernel": "torch rescale + bounds + thrust per bisection step", "limits": name, "B": n, "M": M, "ms": b,
              "ms_min": min(ms["before"]), "ms_max": max(ms["before"]), "rounds": rounds, "steps": steps[0]})
        emit({"limits": name, "B": n, "dilate_over_one_evaluation": c / f, "torch_loop_over_dilate": b / c,
              "dilate_loses_to_torch_loop": bool(c > b)})
    del dW, dT, dC, d_so, ext, rec, sc, act, fl, dT2, dC2
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
