#!/usr/bin/env python3
"""Corridor inflation benchmark: tgms_field_occupancy_device and tgms_corridor_inflate_batch_device on
IB_SIZES (4,096 and 1,048,576) x M = 10 waypoint paths in one 10 m room (synthetic.uniform_batch)
against the field scene of fldbench.py: the exact distance field of 64 seeded boxes on a 128^3
grid over the room, r_free = 0.3, max_grow in {8, 32}.  Per case the time (device events around
IB_ITERS launches, IB_ROUNDS windows after a warm-up; median with its range), the share of
blocked, capped and fully closed legs and the mean number of layers a grown leg took.  In the
same run, to measure against:
  - the table build on its own (its three launches together), a device-to-device copy of the
    table's bytes and the torch threshold with three cumsums;
  - the formulation a caller had before, in torch on the device: a threshold, three cumsums, the
    seed in fp64, then 6 max_grow steps of eight-corner gathers over all legs with masks; checked
    for equality with the call before it is timed;
  - one tgms_corridor_batch_device call on the produced faces (the batch solved on the device
    first), to say what share of a loop round the new step costs.
One JSON line per result on stdout and in IB_OUT (default profiles/inflate_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import FEAS_NONFINITE, INF_BLOCKED, INF_CAPPED, INF_OUTSIDE
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("IB_OUT", os.path.join(ROOT, "profiles", "inflate_bench.jsonl"))
ROUNDS = int(os.environ.get("IB_ROUNDS", 5))
ITERS = int(os.environ.get("IB_ITERS", 4))
SIZES = [int(x) for x in os.environ.get("IB_SIZES", "4096,1048576").split(",")]
GRID = int(os.environ.get("IB_GRID", 128))
R_FREE = float(os.environ.get("IB_RFREE", 0.3))
GROWS = (8, 32)
M, K = 10, 64
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


def timed(run, iters, rounds=ROUNDS):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = [window(run, iters) for _ in range(rounds)]
    return {"ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "rounds": rounds, "iters": iters}


def boxes(k, seed):  # fldbench.py's
    rng = np.random.default_rng(seed)
    c = np.c_[rng.uniform(-5, 5, k), rng.uniform(-5, 5, k), rng.uniform(0.5, 5, k)]
    h = rng.uniform(0.1, 0.5, (k, 3))
    return np.concatenate([c - h, c + h], axis=1)


ORIGIN = (-6.0, -6.0, -0.5)
H = 12.0 / (GRID - 1)
N3 = (GRID, GRID, GRID)
values = S.box_field(boxes(K, 64), ORIGIN, H, N3)
d_values = torch.from_numpy(values).cuda()
s = Solver(0)
table = torch.empty((GRID + 1,) * 3, dtype=torch.int32, device="cuda")
o3 = torch.tensor(ORIGIN, dtype=torch.float64, device="cuda")

# ---- the table: the call, the torch cumsums, a copy of its bytes ----
build = lambda: s.field_occupancy_device(ORIGIN, H, N3, d_values, R_FREE, table)


def torch_table():
    t = torch.zeros((GRID + 1,) * 3, dtype=torch.int32, device="cuda")
    m = ~(d_values >= torch.tensor(R_FREE, dtype=torch.float32, device="cuda"))
    t[1:, 1:, 1:] = m.to(torch.int32).cumsum(0, dtype=torch.int32).cumsum(1, dtype=torch.int32).cumsum(2, dtype=torch.int32)
    return t


build()
torch.cuda.synchronize()
assert torch.equal(table, torch_table()), "the table differs from the cumsums"
tb = table.numel() * 4
other = torch.empty_like(table)
r = {"case": "table build %d^3 (three launches)" % GRID, "table_bytes": tb, "nonfree_nodes": int(table[-1, -1, -1])}
r.update(timed(build, 20))
emit(r)
rc = {"case": "device-to-device copy of the table's bytes", "table_bytes": tb}
rc.update(timed(lambda: other.copy_(table), 20))
rc["build_over_copy"] = r["ms"] / rc["ms"]
emit(rc)
rt = {"case": "torch threshold + three cumsums"}
rt.update(timed(torch_table, 5))
rt["torch_over_build"] = rt["ms"] / r["ms"]
emit(rt)


# ---- the torch formulation of the growth ----
def seed_torch(W0, W1):
    mn, mx = torch.where(W1 < W0, W1, W0), torch.where(W1 > W0, W1, W0)
    lo = torch.floor((mn - o3) / H)
    lo = lo - (o3 + H * lo > mn).to(torch.float64)
    hi = torch.ceil((mx - o3) / H)
    hi = hi + (o3 + H * hi < mx).to(torch.float64)
    return lo.to(torch.int64), hi.to(torch.int64)


flat = None


def count(lo, hi):
    """Non-free nodes of the boxes lo..hi [n,3] (inside the grid) from the table: eight gathers."""
    w = GRID + 1
    x0, y0, z0 = lo[:, 0], lo[:, 1], lo[:, 2]
    x1, y1, z1 = hi[:, 0] + 1, hi[:, 1] + 1, hi[:, 2] + 1
    at = lambda x, y, z: flat[(z * w + y) * w + x]
    return (at(x1, y1, z1) - at(x0, y1, z1) - at(x1, y0, z1) + at(x0, y0, z1)
            - at(x1, y1, z0) + at(x0, y1, z0) + at(x1, y0, z0) - at(x0, y0, z0))


def torch_inflate(W0, W1, max_grow):
    """The batch is inside the grid and finite (the room lies inside the map): no OUTSIDE, no NaN."""
    lo, hi = seed_torch(W0, W1)
    blocked = count(lo, hi) != 0
    open_ = (~blocked).unsqueeze(1).repeat(1, 6)
    for _ in range(max_grow):
        for d in range(6):
            a, up = d >> 1, d % 2 == 0
            layer = hi[:, a] + 1 if up else lo[:, a] - 1
            inside = (layer <= GRID - 1) if up else (layer >= 0)
            l2, h2 = lo.clone(), hi.clone()
            safe = torch.where(inside, layer, hi[:, a] if up else lo[:, a])  # any in-grid layer for the masked lanes
            l2[:, a], h2[:, a] = safe, safe
            take = open_[:, d] & inside & (count(l2, h2) == 0)
            open_[:, d] &= take
            if up:
                hi[:, a] = torch.where(take, layer, hi[:, a])
            else:
                lo[:, a] = torch.where(take, layer, lo[:, a])
    fl = torch.where(blocked, INF_BLOCKED, torch.where(open_.any(dim=1), INF_CAPPED, 0)).to(torch.int32)
    return torch.cat([lo, hi], dim=1).to(torch.int32), fl


for N in SIZES:
    so, W, T = S.uniform_batch(N, M)
    Sg = N * M
    dW, dT, d_so = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(so).cuda()
    W0, W1 = dW[:, :-1].reshape(-1, 3).contiguous(), dW[:, 1:].reshape(-1, 3).contiguous()
    box = torch.empty((Sg, 6), dtype=torch.int32, device="cuda")
    faces = torch.empty((6 * Sg, 4), dtype=torch.float64, device="cuda")
    fo = torch.empty((Sg + 1,), dtype=torch.int64, device="cuda")
    seg_flags = torch.empty((Sg,), dtype=torch.int32, device="cuda")
    flags = torch.empty((N,), dtype=torch.int32, device="cuda")
    flat = table.reshape(-1).to(torch.int64)  # the gather's table, converted once outside the timing
    seed_lo, seed_hi = seed_torch(W0, W1)
    per = {}
    for mg in GROWS:
        run = lambda: s.corridor_inflate_device(N, d_so, dW, ORIGIN, H, N3, table, mg, box, faces, fo, seg_flags, flags)
        run()
        tbox, tfl = torch_inflate(W0, W1, mg)
        torch.cuda.synchronize()
        assert torch.equal(seg_flags, tfl) and torch.equal(box, tbox), "the torch formulation differs from the call"
        r = {"case": "inflate %d x M=%d, %d^3, r_free %.3g, max_grow %d" % (N, M, GRID, R_FREE, mg), "N": N, "legs": Sg,
             "max_grow": mg}
        r.update(timed(run, ITERS))
        grown = (seg_flags & (INF_BLOCKED | INF_OUTSIDE | FEAS_NONFINITE)) == 0
        layers = ((box[:, 3:].to(torch.int64) - seed_hi) + (seed_lo - box[:, :3].to(torch.int64))).sum(dim=1)[grown]
        r.update({"blocked": float(((seg_flags & INF_BLOCKED) != 0).double().mean()),
                  "capped": float(((seg_flags & INF_CAPPED) != 0).double().mean()),
                  "closed": float((seg_flags == 0).double().mean()),
                  "outside": float(((seg_flags & INF_OUTSIDE) != 0).double().mean()),
                  "layers_per_grown_leg": float(layers.double().mean()), "layers_max": int(layers.max()),
                  "ns_per_leg": r["ms"] * 1e6 / Sg})
        r["table_build_over_inflate"] = results[0]["ms"] / r["ms"]
        emit(r)
        rt = {"case": "torch gathers with masks, %d x M=%d, max_grow %d" % (N, M, mg), "N": N, "max_grow": mg}
        rt.update(timed(lambda: torch_inflate(W0, W1, mg), 1, rounds=3))
        rt["torch_over_call"] = rt["ms"] / r["ms"]
        emit(rt)
        per[mg] = r["ms"]
        del tbox, tfl
    # ---- one corridor call on the produced faces: the share of a loop round ----
    dC = torch.empty((N, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(N, M, dW, dT, dC)
    rec = torch.empty((N, 2), dtype=torch.float64, device="cuda")
    cfl = torch.empty((N,), dtype=torch.int32, device="cuda")
    run = lambda: s.corridor_device(N, d_so, dT, dC, 6 * Sg, faces, fo, 0.0, d_rec=rec, d_flags=cfl)
    rc = {"case": "corridor containment %d x M=%d on the produced faces (max_grow %d)" % (N, M, GROWS[-1]), "N": N}
    rc.update(timed(run, ITERS))
    rc["inflate_over_corridor"] = {str(mg): per[mg] / rc["ms"] for mg in GROWS}
    rs = timed(lambda: s.solve_uniform_device(N, M, dW, dT, dC), ITERS)
    rc["solve_ms"] = rs["ms"]
    emit(rc)
    del dC, faces, box, flat

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
