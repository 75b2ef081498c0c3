#!/usr/bin/env python3
"""Segment re-timing benchmark: tgms_retime_batch_dev on two synthetic batches, 4,096 x M = 10 and
1,048,576 x M = 10 (config 3's shapes), both solved on the device.
  (call)   the call next to tgms_bounds_batch_device on the same batch, alternating windows of one
           run: medians of RB_ROUNDS = 5 windows of RB_ITERS = 10 calls, device events.  From the
           ladder FMA counts in csrc/tgms_bounds.hip the call does 37,240 of the bounds call's 48,160
           FMAs per segment; 0.77 of the bounds time is a supposition, not a target.
  (chains) what the feature buys: (a) solve + dilate, against (b) rounds = 1, 2, 4 of solve + retime
           (s_lo = 1 and 0.8, s_hi = 4), a final solve and the same dilate.  Per chain the mean final
           duration, the share of trajectories with RT_OVER in every round's solve and in the final
           solve (before the dilation makes every one feasible), and the device time of the chain.
The limits are 1.1 x the medians of the solved batch's v / a peaks and 2.2 x that of its jerk peaks,
so about half the trajectories carry RT_OVER; the actual share is reported.  One JSON line per result
on stdout and in RB_OUT (default profiles/retime_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import DIL_CAPPED, RT_OVER, Limits
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("RB_OUT", os.path.join(ROOT, "profiles", "retime_bench.jsonl"))
SIZES = [int(os.environ.get("RB_N", 4096)), int(os.environ.get("RB_NBIG", 1 << 20))]
ITERS, ROUNDS = int(os.environ.get("RB_ITERS", 10)), int(os.environ.get("RB_ROUNDS", 5))
M = 10; g = 9.80665; S_HI = 4.0
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
for n in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    dW, dT0 = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT0, dC)
    d_so = torch.from_numpy(np.arange(n + 1, dtype=np.int32) * M).cuda()
    ext = torch.empty((n, 10), dtype=torch.float64, device="cuda")
    seg = torch.empty((n * M, 4), dtype=torch.float64, device="cuda")
    rec = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    fl = torch.empty((n,), dtype=torch.int32, device="cuda")
    dfl = torch.empty((n,), dtype=torch.int32, device="cuda")
    dT, dT2, dC2 = dT0.clone(), torch.empty_like(dT0), torch.empty_like(dC)
    s.bounds_device(n, d_so, dT0, dC, None, ext, None)
    med = ext[:, 6:9].median(dim=0).values.cpu().numpy()
    lim = Limits(v_max=1.1 * med[0], a_max=1.1 * med[1], j_max=2.2 * med[2])

    # ---- the call next to the bounds call ----
    def call():
        s.retime_device(n, d_so, dT0, dC, lim, 1.0, S_HI, dT2, seg, rec, fl)

    def call_lean():  # what a loop needs: times, record and flags, no per-segment rows
        s.retime_device(n, d_so, dT0, dC, lim, 1.0, S_HI, dT2, None, rec, fl)

    def bounds():
        s.bounds_device(n, d_so, dT0, dC, lim, ext, dfl)

    call(); call_lean(); bounds()
    ms = {"retime": [], "retime_lean": [], "bounds": []}
    for _ in range(ROUNDS):
        ms["retime"].append(window(call, ITERS))
        ms["retime_lean"].append(window(call_lean, ITERS))
        ms["bounds"].append(window(bounds, ITERS))
    call(); torch.cuda.synchronize()
    over0 = float(((fl & RT_OVER) != 0).double().mean())
    c, l, b = (float(np.median(ms[k])) for k in ("retime", "retime_lean", "bounds"))
    for name, key, v in (("retime, all outputs", "retime", c), ("retime, no seg_rec", "retime_lean", l), ("bounds", "bounds", b)):
        emit({"kernel": name, "B": n, "M": M, "ms": v, "ms_min": min(ms[key]), "ms_max": max(ms[key]), "iters": ITERS,
              "windows": ROUNDS})
    emit({"B": n, "retime_over_bounds": c / b, "retime_lean_over_bounds": l / b, "expected_from_fma_counts": 37240 / 48160,
          "retime_slower_than_bounds": bool(c > b), "over_share_of_the_input": over0,
          "limits": [lim.v_max, lim.a_max, lim.j_max]})

    # ---- what the feature buys ----
    def chain(rounds, s_lo, shares=None):
        dT.copy_(dT0)
        for _ in range(rounds):
            s.solve_uniform_device(n, M, dW, dT, dC2)
            s.retime_device(n, d_so, dT, dC2, lim, s_lo, S_HI, dT, None, None, fl)  # in place
            if shares is not None:
                shares.append(float(((fl & RT_OVER) != 0).double().mean()))
        s.solve_uniform_device(n, M, dW, dT, dC2)
        if shares is not None:
            s.retime_device(n, d_so, dT, dC2, lim, 1.0, S_HI, None, None, None, fl)
            shares.append(float(((fl & RT_OVER) != 0).double().mean()))
        s.dilate_device(n, d_so, dT, dC2, g, lim, None, 1.0, 100.0, None, None, dfl, dT2, None)

    base = None
    for rounds, s_lo in [(0, 1.0)] + [(r, sl) for sl in (1.0, 0.8) for r in (1, 2, 4)]:
        shares = []
        chain(rounds, s_lo, shares)  # the warm-up, with the shares read back
        torch.cuda.synchronize()
        dur = dT2.view(n, M).sum(dim=1)
        capped = float(((dfl & DIL_CAPPED) != 0).double().mean())
        t = float(np.median([window(lambda: chain(rounds, s_lo), 1 if n > 65536 else ITERS) for _ in range(ROUNDS)]))
        d = {"chain": "solve + dilate" if rounds == 0 else "%d x (solve + retime) + solve + dilate" % rounds, "B": n,
             "M": M, "rounds": rounds, "s_lo": s_lo, "s_hi": S_HI, "mean_final_duration": float(dur.mean()),
             "over_share_per_round_then_final": shares, "feasible_share_before_the_dilation": 1.0 - shares[-1],
             "capped_share_after_the_dilation": capped, "chain_ms": t}
        if rounds == 0:
            base = d
        else:
            d["duration_over_dilation_alone"] = d["mean_final_duration"] / base["mean_final_duration"]
            d["chain_ms_over_dilation_alone"] = t / base["chain_ms"]
            d["pays"] = bool(d["mean_final_duration"] < base["mean_final_duration"])
        emit(d)
    del dW, dT0, dT, dT2, dC, dC2, d_so, ext, seg, rec, fl, dfl
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
