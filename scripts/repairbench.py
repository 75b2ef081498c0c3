#!/usr/bin/env python3
"""Waypoint repair benchmark on the scene of edtbench.py and reroutebench.py (the exact distance field
of 64 seeded boxes on a 128^3 grid, r_free = 0.3).  In one run:
  - the map build, tgms_field_nearest_free_dev at max_shift 4 and 16, window by window next to
    tgms_field_edt_device on the occupancy of the same nodes (capped at the same reach);
  - the repair, tgms_waypoints_repair_batch_dev at max_shift 4, on the short-leg batches of
    reroutebench.py, PB_SIZES x M = 4, and on its own output (nothing left to move: the cost a
    planner pays that already keeps its waypoints clear);
  - the same batch through the host backend (wall clock, map build included and apart), equal bits
    asserted on the smallest size;
  - a torch formulation a caller would write: cell corners from the free mask, then for every blocked
    waypoint the masked squared distances over the (2R+1)^3 window around its nearest node and an
    argmin with the lowest index on ties; equal waypoints and flags asserted;
  - the re-route (margin 4, max_pieces 8) on the batch before and after the repair: the share of
    every flag among its candidates.
Times are device events around PB_ITERS calls, PB_ROUNDS windows after a warm-up; median with its
range.  One JSON line per result on stdout and in PB_OUT (default profiles/repair_bench.jsonl)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import (FEAS_NONFINITE, RPR_KEPT, RPR_MOVED, RPR_OUTSIDE, RPR_STUCK, RRT_BLOCKED, RRT_ENDS,
                                           RRT_LONG, RRT_NOPATH, RRT_OUTSIDE, RRT_WINDOW)
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("PB_OUT", os.path.join(ROOT, "profiles", "repair_bench.jsonl"))
ROUNDS = int(os.environ.get("PB_ROUNDS", 5))
ITERS = int(os.environ.get("PB_ITERS", 10))
SIZES = [int(x) for x in os.environ.get("PB_SIZES", "4096,65536").split(",")]
HOST_REPS = int(os.environ.get("PB_HOST_REPS", 2))
GRID, R_FREE, K, M, REACH, MARGIN, PIECES = 128, 0.3, 64, 4, 4, 4, 8
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


def short_legs(N, M, reach, seed):  # reroutebench.py's
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
NN = GRID ** 3
values = S.box_field(boxes(K, 64), ORIGIN, H, N3)
d_values = torch.from_numpy(values).cuda()
s = Solver(0)
i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")

# ---- the map build next to the distance-field build ----
occ = torch.from_numpy((values < np.float32(R_FREE)).astype(np.uint8)).cuda()
near, work = torch.empty(NN, **i32), torch.empty(NN, **i32)
dsq = torch.empty(NN, **i32)
edt_vals = torch.empty(NN, dtype=torch.float32, device="cuda")
edt_work = torch.empty(s.field_edt_work_size(ORIGIN, H, N3) // 4, **i32)
for reach in (4, 16):
    build = lambda: s.field_nearest_free_device(ORIGIN, H, N3, d_values, R_FREE, reach, near, work, dsq)
    edt = lambda: s.field_edt_device(ORIGIN, H, N3, occ, reach * H, edt_work, d_values=edt_vals)
    for f in (build, edt):
        f(); f()
    torch.cuda.synchronize()
    ms_b, ms_e = [], []
    for _ in range(ROUNDS):  # the windows alternate
        ms_b.append(window(build, ITERS))
        ms_e.append(window(edt, ITERS))
    r = {"case": "nearest-free map, %d^3, max_shift %d, next to the EDT capped at the same reach" % (GRID, reach),
         "max_shift": reach, "free_share": float((values >= np.float32(R_FREE)).mean()),
         "none_share": float((near == -1).float().mean())}
    r.update(stats(ms_b, ITERS))
    r.update(stats(ms_e, ITERS, "edt_ms"))
    r["build_over_edt"] = r["ms"] / r["edt_ms"]
    emit(r)
build_ms = {x["max_shift"]: x["ms"] for x in results}
s.field_nearest_free_device(ORIGIN, H, N3, d_values, R_FREE, REACH, near, work)
table = torch.empty((GRID + 1,) * 3, **i32)
s.field_occupancy_device(ORIGIN, H, N3, d_values, R_FREE, table)
torch.cuda.synchronize()


# ---- a torch formulation of the repair ----
def torch_repair(dW, free, R):
    o = torch.tensor(ORIGIN, **f64)
    n = torch.tensor(N3, dtype=torch.int64, device="cuda")
    q = (dW - o) / H
    lo, hi = torch.floor(q).long(), torch.ceil(q).long()
    inside = ((lo >= 0) & (hi <= n - 1)).all(dim=1)
    lin = lambda i: (i[:, 2] * GRID + i[:, 1]) * GRID + i[:, 0]  # noqa: E731
    clear = torch.ones(len(dW), dtype=torch.bool, device="cuda")
    for cz in (lo, hi):
        for cy in (lo, hi):
            for cx in (lo, hi):
                c = torch.stack([cx[:, 0], cy[:, 1], cz[:, 2]], dim=1).clamp(min=0).minimum(n - 1)
                clear &= free[lin(c)]
    blocked = inside & ~clear
    nn = torch.floor(q[blocked] + 0.5).long().clamp(min=0).minimum(n - 1)
    r = torch.arange(-R, R + 1, device="cuda")
    off = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3).flip(1)  # z slowest: ascending index
    D = (off * off).sum(1)
    out, flags = dW.clone(), torch.zeros(len(dW), **i32)
    flags[~inside] = RPR_OUTSIDE
    rows = torch.nonzero(blocked).flatten()
    for a in range(0, len(rows), 1 << 15):
        c = nn[a:a + (1 << 15), None, :] + off[None]
        ok = ((c >= 0) & (c <= n - 1)).all(dim=2) & (D <= R * R)[None]
        cl = c.clamp(min=0).minimum(n - 1)
        ok &= free[(cl[..., 2] * GRID + cl[..., 1]) * GRID + cl[..., 0]]
        key = torch.where(ok, D[None] * len(off) + torch.arange(len(off), device="cuda")[None], torch.iinfo(torch.int64).max)
        best = key.argmin(dim=1)
        found = ok.gather(1, best[:, None]).flatten()
        site = cl[torch.arange(len(best), device="cuda"), best]
        rr = rows[a:a + (1 << 15)]
        out[rr[found]] = o + H * site[found].double()
        flags[rr] = torch.where(found, RPR_MOVED, RPR_STUCK).to(torch.int32)
    return out, flags


free_mask = torch.from_numpy((values >= np.float32(R_FREE)).reshape(-1)).cuda()
RRT = (("window", RRT_WINDOW), ("ends", RRT_ENDS), ("nopath", RRT_NOPATH), ("long", RRT_LONG), ("outside", RRT_OUTSIDE),
       ("nonfinite", FEAS_NONFINITE))

for N in SIZES:
    so, W, T = short_legs(N, M, 2.0, seed=N)
    Sg, rows = N * M, N * (M + 1)
    d_so, dW, dT = torch.from_numpy(so).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    W2, T2, wp, sh, fl = torch.empty((rows, 3), **f64), torch.empty(Sg, **f64), torch.empty(rows, **i32), torch.empty(rows, **i32), torch.empty(N, **i32)
    W3, T3, wp3 = torch.empty((rows, 3), **f64), torch.empty(Sg, **f64), torch.empty(rows, **i32)
    run = lambda: s.waypoints_repair_device(N, d_so, dW, ORIGIN, H, N3, near, 0, W2, d_seg_times=dT, d_seg_times_out=T2,
                                            d_wp_flags=wp, d_shift=sh, d_flags=fl)
    again = lambda: s.waypoints_repair_device(N, d_so, W2, ORIGIN, H, N3, near, 0, W3, d_seg_times=T2, d_seg_times_out=T3,
                                              d_wp_flags=wp3)
    tch = lambda: torch_repair(dW, free_mask, REACH)
    for f in (run, again, tch):
        f(); f()
    torch.cuda.synchronize()
    ms_run, ms_again, ms_t = [], [], []
    for _ in range(ROUNDS):
        ms_run.append(window(run, ITERS))
        ms_again.append(window(again, ITERS))
        ms_t.append(window(tch, 2))
    h_wp, h_wp3 = wp.cpu().numpy(), wp3.cpu().numpy()
    tW, tfl = tch()
    assert torch.equal(tW, W2) and np.array_equal(tfl.cpu().numpy(), h_wp), "the torch formulation and the call differ"
    r = {"case": "repair short legs <= 2 m, %d x M=%d, %d^3, max_shift %d" % (N, M, GRID, REACH), "N": N, "waypoints": rows}
    for key, bit in (("moved", RPR_MOVED), ("stuck", RPR_STUCK), ("kept", RPR_KEPT), ("outside", RPR_OUTSIDE)):
        r[key + "_share"] = float((h_wp == bit).mean())
    r["clear_share"] = float((h_wp == 0).mean())
    r["moved_share_on_own_output"] = float((h_wp3 == RPR_MOVED).mean())
    r.update(stats(ms_run, ITERS))
    r.update(stats(ms_again, ITERS, "own_output_ms"))
    r.update(stats(ms_t, ITERS, "torch_ms"))  # two calls a window, not ITERS
    r["torch_iters"] = 2
    r["torch_over_call"] = r["torch_ms"] / r["ms"]
    r["map_build_ms"] = build_ms[REACH]
    r["map_build_over_call"] = build_ms[REACH] / r["ms"]
    r["ns_per_waypoint"] = r["ms"] * 1e6 / rows
    with Solver(host=True) as hs:
        a = (so, W, ORIGIN, H, values, R_FREE, REACH, 0, T)
        sec, sec_map = [], []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            ref = hs.waypoints_repair(*a)
            sec.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            hs.field_nearest_free(values, ORIGIN, H, R_FREE, REACH)
            sec_map.append(time.perf_counter() - t0)
    if N == min(SIZES):
        same = (np.array_equal(ref[0], W2.cpu().numpy()) and np.array_equal(ref[1], T2.cpu().numpy())
                and np.array_equal(ref[2], h_wp) and np.array_equal(ref[3], fl.cpu().numpy()) and np.array_equal(ref[4], sh.cpu().numpy()))
        assert same, "host backend and device differ"
    r.update({"host_ms": float(np.median(sec)) * 1e3, "host_map_ms": float(np.median(sec_map)) * 1e3, "host_reps": HOST_REPS})
    r["host_over_map_and_call"] = r["host_ms"] / (r["ms"] + build_ms[REACH])
    # the re-route on the batch before and after
    cap = min(PIECES * Sg, 16 * N)
    so2, Wr, Tr = torch.empty(N + 1, **i32), torch.empty((cap + N, 3), **f64), torch.empty(cap, **f64)
    par, sf, tot = torch.empty(cap, **i32), torch.empty(cap, **i32), torch.empty(2, dtype=torch.int64, device="cuda")
    good = (h_wp == 0) | (h_wp == RPR_MOVED)
    leg_rows = np.arange(Sg) + np.repeat(np.arange(N), M)
    leg_ok = good[leg_rows] & good[leg_rows + 1]
    for tag, w_in, t_in in (("before", dW, dT), ("after", W2, T2)):
        s.corridor_reroute_device(N, d_so, w_in, ORIGIN, H, N3, table, MARGIN, PIECES, so2, Wr, tot, d_seg_times=t_in,
                                  d_seg_times_out=Tr, d_parent=par, d_seg_flags_out=sf)
        torch.cuda.synchronize()
        S1 = int(tot[0])
        p, f = par[:S1].cpu().numpy(), sf[:S1].cpu().numpy()
        pieces = np.bincount(p, minlength=Sg)
        leg_fl = np.zeros(Sg, np.int64)
        np.bitwise_or.at(leg_fl, p, f)
        cand = (pieces > 1) | ((leg_fl & RRT_BLOCKED) != 0)
        r["candidates_" + tag] = int(cand.sum())
        r["rerouted_share_of_candidates_" + tag] = float((pieces > 1).sum() / max(1, cand.sum()))
        for key, bit in RRT:
            r["%s_share_of_candidates_%s" % (key, tag)] = float(((leg_fl & bit) != 0).sum() / max(1, cand.sum()))
        r["ends_legs_" + tag] = int(((leg_fl & RRT_ENDS) != 0).sum())
        if tag == "after":  # the lattice of this scene is not dyadic: guarantee 2 is not promised, so it is counted
            r["ends_legs_with_both_ends_clear_or_moved_after"] = int((((leg_fl & RRT_ENDS) != 0) & leg_ok).sum())
    emit(r)
    del W2, T2, W3, T3, Wr, Tr
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
