#!/usr/bin/env python3
"""Distance-field clearance benchmark: tgms_field_clearance_batch_device on FB_SIZES (4,096 and
65,536) x M = 10 candidates in one 10 m room (synthetic.uniform_batch, solved on the device)
against the exact distance field of 64 seeded boxes with sides of 0.2 to 1 m
(synthetic.box_field) on a 128^3 grid over the room, r_min = 0.3:
  - tol in {1e-2, 1e-3}, each with lip = 0 (the bound reduced from the values by the call) and
    with the bound given; per case the time (device events around FB_ITERS launches, FB_ROUNDS
    windows after a warm-up; median with its range), the mean and the largest evals, the rows
    within r_min and the rows that spent the budget;
  - the formulation a caller had before, on the same batch: tgms_sample_batch_device at 100 Hz
    into a reused buffer, 4,096 trajectories at a time, a torch trilinear gather and a min per
    trajectory; its time, and how far its minimum lies above the certified one;
  - tgms_clearance_batch_device on the same 64 boxes, the exact answer for a world that is a
    list: its d_min of the rows within r_min against the field's (the field is the boxes'
    distance interpolated, so the two differ by the interpolation error of the grid, which is
    reported, not asserted).
One JSON line per result on stdout and in FB_OUT (default profiles/field_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import FLD_UNRESOLVED, SEP_CLOSE, SEP_NONFINITE
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver, sample_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("FB_OUT", os.path.join(ROOT, "profiles", "field_bench.jsonl"))
ROUNDS = int(os.environ.get("FB_ROUNDS", 5))
ITERS = int(os.environ.get("FB_ITERS", 2))
SIZES = [int(x) for x in os.environ.get("FB_SIZES", "4096,65536").split(",")]
GRID = int(os.environ.get("FB_GRID", 128))
R_MIN = float(os.environ.get("FB_RMIN", 0.3))
TOLS = (1e-2, 1e-3)
M, DT, CHUNK, K = 10, 0.01, 4096, 64
MAX_EVALS = 1 << 20
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


def timed(run, iters):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = [window(run, iters) for _ in range(ROUNDS)]
    return {"ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "rounds": ROUNDS, "iters": iters}


def boxes(k, seed):
    rng = np.random.default_rng(seed)
    c = np.c_[rng.uniform(-5, 5, k), rng.uniform(-5, 5, k), rng.uniform(0.5, 5, k)]
    h = rng.uniform(0.1, 0.5, (k, 3))
    return np.concatenate([c - h, c + h], axis=1)


# the map: the room with a margin, so that a trajectory that overshoots a wall stays inside
ORIGIN = (-6.0, -6.0, -0.5)
H = 12.0 / (GRID - 1)
ob = boxes(K, 64)
values = S.box_field(ob, ORIGIN, H, (GRID, GRID, GRID))
d_values, d_ob = torch.from_numpy(values).cuda(), torch.from_numpy(ob).cuda()
g = [float(np.abs(np.diff(values.astype(np.float64), axis=a)).max()) / H for a in (2, 1, 0)]
LIP = float(np.sqrt(sum(x * x for x in g)))
emit({"field": "box_field of %d boxes on %d^3, h %.4g" % (K, GRID, H), "lip_from_values": LIP, "max_value": float(values.max())})

s = Solver(0)
o3 = torch.tensor(ORIGIN, dtype=torch.float64, device="cuda")
flat = d_values.reshape(-1).to(torch.float64)  # the gather's table, converted once outside the timing


def trilinear(p):
    q = torch.clamp((p - o3) / H, min=0.0, max=float(GRID - 1))
    i = torch.clamp(q.floor().to(torch.int64), max=GRID - 2)
    f = q - i
    at = (i[:, 2] * GRID + i[:, 1]) * GRID + i[:, 0]
    out = torch.zeros(len(p), dtype=torch.float64, device="cuda")
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                out += w * flat[at + (dz * GRID + dy) * GRID + dx]
    return out


for N in SIZES:
    so, W, T = S.uniform_batch(N, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((N, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(N, M, dW, dT, dC)
    d_so = torch.from_numpy(so).cuda()
    near = torch.empty((N, 2), dtype=torch.float64, device="cuda")
    evals, flags = (torch.empty((N,), dtype=torch.int32, device="cuda") for _ in range(2))
    cert = {}
    for tol in TOLS:
        for lip, how in ((0.0, "reduced by the call"), (LIP, "given")):
            run = lambda: s.field_clearance_device(N, d_so, dT, dC, ORIGIN, H, (GRID, GRID, GRID), d_values, lip, R_MIN, tol,
                                                   MAX_EVALS, near, evals, flags)
            r = {"case": "field clearance %d x M=%d, %d^3, r_min %.3g, tol %.0e, lip %s" % (N, M, GRID, R_MIN, tol, how),
                 "N": N, "tol": tol, "lip": how}
            r.update(timed(run, ITERS))
            ev = evals.to(torch.float64)
            r.update({"evals_mean": float(ev.mean()), "evals_max": int(evals.max()), "evals_total": float(ev.sum()),
                      "rows_close": int(((flags & SEP_CLOSE) != 0).sum()), "rows_unresolved": int(((flags & FLD_UNRESOLVED) != 0).sum()),
                      "rows_nonfinite": int((flags == SEP_NONFINITE).sum())})
            r["ns_per_eval"] = r["ms"] * 1e6 / max(r["evals_total"], 1.0)
            r["ns_per_trajectory"] = r["ms"] * 1e6 / N
            emit(r)
            if lip > 0.0:
                cert[tol] = (near[:, 0].clone(), flags.clone(), r["ms"])

    # ---- the sampled chain: 100 Hz into a reused buffer, CHUNK trajectories at a time ----
    Tn = T.reshape(N, M)
    chunks = []
    for c0 in range(0, N, CHUNK):
        n = min(CHUNK, N - c0)
        offs = sample_offsets(so[:n + 1], Tn[c0:c0 + n].reshape(-1), DT)
        row = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(np.diff(offs)).cuda())
        chunks.append((c0, n, torch.from_numpy(offs).cuda(), row, int(offs[-1])))
    smp = torch.empty((max(c[4] for c in chunks), 14), dtype=torch.float64, device="cuda")
    d_smp = torch.empty(N, dtype=torch.float64, device="cuda")

    def run_sampled():
        for c0, n, d_offs, row, total in chunks:
            s.sample_device(n, d_so[:n + 1], dW[c0:c0 + n], dT[c0:c0 + n], dC[c0:c0 + n], DT, d_offs, smp)
            v = trilinear(smp[:total, :3])
            d_smp[c0:c0 + n] = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda").scatter_reduce(
                0, row, v, reduce="amin")

    rs = {"case": "sampled at 100 Hz + torch trilinear gather + min, %d x M=%d in chunks of %d" % (N, M, CHUNK), "N": N,
          "samples": int(sum(c[4] for c in chunks))}
    rs.update(timed(run_sampled, 1))
    rs["ns_per_sample"] = rs["ms"] * 1e6 / rs["samples"]
    rs["ns_per_trajectory"] = rs["ms"] * 1e6 / N
    emit(rs)
    for tol in TOLS:
        d_c, fl, ms = cert[tol]
        m = ((fl & SEP_CLOSE) != 0) & ((fl & FLD_UNRESOLVED) == 0)  # where d_min is within tol of the minimum
        gain = (d_smp - d_c)[m]
        hid = (d_smp >= R_MIN) & m  # the sampled check passes a row that comes within r_min
        emit({"N": N, "tol": tol, "sampled_over_certified_time": rs["ms"] / ms, "rows_compared": int(m.sum()),
              "sampled_minus_certified_max": float(gain.max()) if len(gain) else None,
              "sampled_minus_certified_median": float(gain.median()) if len(gain) else None,
              "certified_above_sampled_by_more_than_tol": int((gain < -tol).sum()),
              "rows_within_r_min_the_samples_miss": int(hid.sum())})

    # ---- the list formulation: the exact clearance from the same 64 boxes ----
    c_near = torch.empty((N, 2), dtype=torch.float64, device="cuda")
    c_obs, c_cnt, c_tst, c_fl = (torch.empty((N,), dtype=torch.int32, device="cuda") for _ in range(4))
    run = lambda: s.clearance_device(N, d_so, dT, dC, K, d_ob, R_MIN, None, c_near, c_obs, c_cnt, c_tst, c_fl)
    rc = {"case": "clearance %d x M=%d against the same %d boxes, r_min %.3g" % (N, M, K, R_MIN), "N": N}
    rc.update(timed(run, ITERS))
    rc["ns_per_trajectory"] = rc["ms"] * 1e6 / N
    rc["rows_close"] = int((c_cnt > 0).sum())
    d_c, fl, ms = cert[TOLS[-1]]
    m = (c_cnt > 0) & ((fl & SEP_CLOSE) != 0)
    rc["field_minus_boxes_max_abs"] = float((d_c - c_near[:, 0])[m].abs().max()) if int(m.sum()) else None
    rc["clearance_over_field_time"] = rc["ms"] / ms
    emit(rc)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
