#!/usr/bin/env python3
"""Corridor re-route benchmark: tgms_corridor_reroute_batch_dev on the scene of inflbench.py and
subdivbench.py (the exact distance field of 64 seeded boxes on a 128^3 grid, r_free = 0.3), margin
in {4, 8}, max_pieces = 8, on
  - the headline batch, RB_SIZES[0] x M = 10 room-crossing paths (synthetic.uniform_batch), and
  - batches of short legs, RB_SIZES x M = 4 with legs of at most 2 m,
Per case the time of the call (device events around RB_ITERS calls, RB_ROUNDS windows after a
warm-up; median with its range), the share of every flag among the input legs, ns per candidate,
and window by window in the same loop one inflation call on the output.  On the smallest size the
host backend's queue search runs on the same batch in the same run (wall clock, RB_HOST_REPS
repeats, the table build included: it is the only formulation a caller had) and its output is
checked equal to the device's.  The stages are not timed apart: the call is timed whole.
One JSON line per result on stdout and in RB_OUT (default profiles/reroute_bench.jsonl, rewritten)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import (FEAS_NONFINITE, RRT_BLOCKED, RRT_DONE, RRT_ENDS, RRT_FULL, RRT_LONG, RRT_NOPATH,
                                           RRT_OUTSIDE, RRT_WINDOW)
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("RB_OUT", os.path.join(ROOT, "profiles", "reroute_bench.jsonl"))
ROUNDS = int(os.environ.get("RB_ROUNDS", 5))
ITERS = int(os.environ.get("RB_ITERS", 4))
SIZES = [int(x) for x in os.environ.get("RB_SIZES", "4096,65536").split(",")]
HOST_REPS = int(os.environ.get("RB_HOST_REPS", 2))
GRID, R_FREE, K, PIECES = 128, 0.3, 64, 8
MARGINS = (4, 8)
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


def stats(ms, iters, key="ms"):
    return {key: float(np.median(ms)), key + "_min": min(ms), key + "_max": max(ms), "rounds": len(ms), "iters": iters}


def boxes(k, seed):  # fldbench.py's
    rng = np.random.default_rng(seed)
    c = np.c_[rng.uniform(-5, 5, k), rng.uniform(-5, 5, k), rng.uniform(0.5, 5, k)]
    h = rng.uniform(0.1, 0.5, (k, 3))
    return np.concatenate([c - h, c + h], axis=1)


def short_legs(N, M, reach, seed):
    rng = np.random.default_rng(seed)
    W = np.empty((N, M + 1, 3))
    W[:, 0] = np.c_[rng.uniform(-4.5, 4.5, N), rng.uniform(-4.5, 4.5, N), rng.uniform(0.5, 4.5, N)]
    for i in range(M):
        d = rng.normal(size=(N, 3))
        d *= (rng.uniform(0.3, reach, N) / np.linalg.norm(d, axis=1))[:, None]
        W[:, i + 1] = np.clip(W[:, i] + d, (-5.0, -5.0, 0.0), (5.0, 5.0, 5.0))
    return (M * np.arange(N + 1)).astype(np.int32), W.reshape(-1, 3), rng.uniform(0.5, 4.0, N * M)


ORIGIN = (-6.0, -6.0, -0.5)
H = 12.0 / (GRID - 1)
N3 = (GRID, GRID, GRID)
values = S.box_field(boxes(K, 64), ORIGIN, H, N3)
d_values = torch.from_numpy(values).cuda()
s = Solver(0)
table = torch.empty((GRID + 1,) * 3, dtype=torch.int32, device="cuda")
s.field_occupancy_device(ORIGIN, H, N3, d_values, R_FREE, table)
torch.cuda.synchronize()
FLAGS = (("window", RRT_WINDOW), ("ends", RRT_ENDS), ("nopath", RRT_NOPATH), ("long", RRT_LONG), ("outside", RRT_OUTSIDE),
         ("nonfinite", FEAS_NONFINITE))

cases = [("room-crossing", SIZES[0], 10, None)] + [("short legs <= 2 m", N, 4, 2.0) for N in SIZES]
for name, N, M, reach in cases:
    if reach is None:
        so, W, T = S.uniform_batch(N, M)
        W, T = W.reshape(-1, 3), T.reshape(-1)
    else:
        so, W, T = short_legs(N, M, reach, seed=N)
    Sg = N * M
    d_so, dW, dT = torch.from_numpy(so).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    cap = min(PIECES * Sg, 16 * N)
    i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    so2, W2, T2 = torch.empty(N + 1, **i32), torch.empty((cap + N, 3), **f64), torch.empty(cap, **f64)
    parent, seg_fl, hops, flags = torch.empty(cap, **i32), torch.empty(cap, **i32), torch.empty(Sg, **i32), torch.empty(N, **i32)
    tot = torch.empty(2, dtype=torch.int64, device="cuda")
    inf_seg = torch.empty(cap, **i32)
    for margin in MARGINS:
        run = lambda: s.corridor_reroute_device(N, d_so, dW, ORIGIN, H, N3, table, margin, PIECES, so2, W2, tot, d_seg_times=dT,
                                                d_seg_times_out=T2, d_parent=parent, d_seg_flags_out=seg_fl, d_hops=hops,
                                                d_flags=flags)
        infl = lambda: s.corridor_inflate_device(N, so2, W2, ORIGIN, H, N3, table, 8, d_seg_flags=inf_seg)
        for f in (run, infl):
            f(); f()
        torch.cuda.synchronize()
        ms_call, ms_inf = [], []
        for _ in range(ROUNDS):  # the windows alternate
            ms_call.append(window(run, ITERS))
            ms_inf.append(window(infl, ITERS))
        S1 = int(tot[0])
        sf, par, hp, fl = seg_fl[:S1].cpu().numpy(), parent[:S1].cpu().numpy(), hops.cpu().numpy(), flags.cpu().numpy()
        pieces = np.bincount(par, minlength=Sg)
        leg_fl = np.zeros(Sg, np.int64)
        np.bitwise_or.at(leg_fl, par, sf)
        full_legs = np.repeat((fl & RRT_FULL) != 0, M)
        cand = (pieces > 1) | ((leg_fl & RRT_BLOCKED) != 0)
        r = {"case": "re-route %s, %d x M=%d, %d^3, margin %d, max_pieces %d" % (name, N, M, GRID, margin, PIECES), "N": N,
             "legs": Sg, "margin": margin, "segments_out": S1, "candidates": int(cand.sum()), "candidate_share": float(cand.mean()),
             "rerouted_share_of_candidates": float((pieces > 1).sum() / max(1, cand.sum())),
             "full_share_of_candidates": float((cand & full_legs).sum() / max(1, cand.sum())),
             "searched": int((hp >= 0).sum()), "hops_mean": float(hp[hp >= 0].mean()) if (hp >= 0).any() else 0.0,
             "hops_max": int(hp.max()), "rows_done": int(((fl & RRT_DONE) != 0).sum())}
        for key, bit in FLAGS:
            r[key + "_share_of_candidates"] = float(((leg_fl & bit) != 0).sum() / max(1, cand.sum()))
        r.update(stats(ms_call, ITERS))
        r["ns_per_candidate"] = r["ms"] * 1e6 / max(1, int(cand.sum()))
        r.update(stats(ms_inf, ITERS, "inflate_ms"))
        r["call_over_inflate"] = r["ms"] / r["inflate_ms"]
        if N == min(SIZES):
            with Solver(host=True) as sh:
                a = (so, W, ORIGIN, H, values, R_FREE, margin, PIECES, T)
                ref = sh.corridor_reroute(*a)
                sec = []
                for _ in range(HOST_REPS):
                    t0 = time.perf_counter()
                    sh.corridor_reroute(*a)
                    sec.append(time.perf_counter() - t0)
            same = (np.array_equal(ref[0], so2.cpu().numpy()) and np.array_equal(ref[1], W2[:S1 + N].cpu().numpy(), equal_nan=True)
                    and np.array_equal(ref[2], T2[:S1].cpu().numpy()) and np.array_equal(ref[4], sf) and np.array_equal(ref[5], hp))
            assert same, "host backend and device differ"
            r.update({"host_ms": float(np.median(sec)) * 1e3, "host_over_call": float(np.median(sec)) * 1e3 / r["ms"]})
        emit(r)
    del W2, T2, parent, seg_fl, inf_seg
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
