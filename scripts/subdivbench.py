#!/usr/bin/env python3
"""Corridor subdivision benchmark: tgms_corridor_subdivide_batch_device on SB_SIZES (4,096 and
1,048,576) x M = 10 waypoint paths in one 10 m room (synthetic.uniform_batch) against the scene of
inflbench.py: the exact distance field of 64 seeded boxes on a 128^3 grid, r_free = 0.3, max_depth
in {2, 4}.  Per case the time of the call (device events around SB_ITERS calls, SB_ROUNDS windows
after a warm-up; median with its range) and, window by window in the same loop so that a drift of
the machine meets all three alike:
  - a device-to-device copy whose traffic is the bytes the call must move (the waypoints, times and
    offsets it reads plus the rows it writes: a copy of half that many bytes reads and writes them);
  - the formulation a caller would write in torch on the device: the seventeen points per leg, per
    depth the seeds and masked eight-corner gathers from the table, the demands and the depth per
    trajectory, then cumsum / repeat_interleave / index_select for the rows; checked equal to the
    call's output on the small batch before anything is timed.
Also the share of legs the inflation reports BLOCKED before and after the call, the share of output
segments that stay SUB_BLOCKED in a trajectory without SUB_FULL, and the rows that set SUB_FULL.
One JSON line per result on stdout and in SB_OUT (default profiles/subdivide_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import INF_BLOCKED, SUB_BLOCKED, SUB_DONE, SUB_FULL
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("SB_OUT", os.path.join(ROOT, "profiles", "subdivide_bench.jsonl"))
ROUNDS = int(os.environ.get("SB_ROUNDS", 5))
ITERS = int(os.environ.get("SB_ITERS", 4))
SIZES = [int(x) for x in os.environ.get("SB_SIZES", "4096,1048576").split(",")]
TORCH_MAX = int(os.environ.get("SB_TORCH_MAX", 1048576))  # the torch chain is not run above this size
GRID = int(os.environ.get("SB_GRID", 128))
R_FREE = float(os.environ.get("SB_RFREE", 0.3))
DEPTHS = (2, 4)
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


def stats(ms, iters):
    return {"ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "rounds": len(ms), "iters": iters}


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
s.field_occupancy_device(ORIGIN, H, N3, d_values, R_FREE, table)
torch.cuda.synchronize()
flat = table.reshape(-1).to(torch.int64)  # the gathers' table, converted once outside the timing
o3 = torch.tensor(ORIGIN, dtype=torch.float64, device="cuda")
FR = (torch.arange(17, dtype=torch.float64, device="cuda") / 16.0)[None, :, None]


def count(lo, hi):
    w = GRID + 1
    x0, y0, z0 = lo[..., 0], lo[..., 1], lo[..., 2]
    x1, y1, z1 = hi[..., 0] + 1, hi[..., 1] + 1, hi[..., 2] + 1
    at = lambda x, y, z: flat[(z * w + y) * w + x]
    return (at(x1, y1, z1) - at(x0, y1, z1) - at(x1, y0, z1) + at(x0, y0, z1)
            - at(x1, y1, z0) + at(x0, y1, z0) + at(x1, y0, z0) - at(x0, y0, z0))


def torch_subdivide(W0, W1, T, N, max_depth):
    """The batch is inside the grid and finite (the room lies inside the map): no OUTSIDE, no NaN.
    Returns so', W', T', seg_flags', flags."""
    Sg = W0.shape[0]
    P = W0[:, None, :] + FR * (W1 - W0)[:, None, :]
    P[:, 0], P[:, 16] = W0, W1
    reached = torch.ones((Sg, 1), dtype=torch.bool, device="cuda")
    need = [torch.ones(Sg, dtype=torch.int64, device="cuda")]
    done = torch.zeros(Sg, dtype=torch.int64, device="cuda")  # clear pieces above the level
    levels = []
    for k in range(max_depth + 1):
        step = 16 >> k
        a, b = P[:, 0:16:step], P[:, step:17:step]
        mn, mx = torch.minimum(a, b), torch.maximum(a, b)
        lo = torch.floor((mn - o3) / H)
        lo = lo - (o3 + H * lo > mn).to(torch.float64)
        hi = torch.ceil((mx - o3) / H)
        hi = hi + (o3 + H * hi < mx).to(torch.float64)
        inside = ((lo >= 0) & (hi <= GRID - 1)).all(dim=2)
        lo, hi = lo.clamp(0, GRID - 1).to(torch.int64), hi.clamp(0, GRID - 1).to(torch.int64)
        clear = reached & inside & (count(lo, hi) == 0)  # the masked gathers
        levels.append((reached, clear))
        if k:
            need.append(done + reached.sum(dim=1))
        done = done + clear.sum(dim=1)
        reached = (reached & ~clear).repeat_interleave(2, dim=1)
    sums = torch.stack(need, dim=1).reshape(N, M, -1).sum(dim=1)  # [N, max_depth + 1]
    fits = sums <= 16
    D = (fits * torch.arange(max_depth + 1, device="cuda")).max(dim=1).values
    Dl = D.repeat_interleave(M)
    start = torch.zeros((Sg, 16), dtype=torch.bool, device="cuda")
    blocked = torch.zeros((Sg, 16), dtype=torch.bool, device="cuda")
    for k, (r, c) in enumerate(levels):
        use = (Dl >= k)[:, None]
        start[:, ::16 >> k] |= r & use
        blocked[:, ::16 >> k] |= r & ~c & (Dl == k)[:, None]
    cnt = start.sum(dim=1)
    so2 = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    so2[1:] = cnt.reshape(N, M).sum(dim=1).cumsum(0)
    leg, i0 = start.nonzero(as_tuple=True)  # row-major: the output order
    nxt = torch.where(start, torch.arange(16, device="cuda")[None, :], 99).flip(1).cummin(dim=1).values.flip(1)
    nxt = torch.cat([nxt[:, 1:], torch.full((Sg, 1), 99, device="cuda")], dim=1).clamp(max=16)
    ln = nxt[leg, i0] - i0
    T2 = torch.where(ln == 16, T[leg], T[leg] * (ln.to(torch.float64) / 16.0))
    traj = leg // M
    rows = torch.arange(leg.numel(), device="cuda") + traj
    W2 = torch.empty((leg.numel() + N, 3), dtype=torch.float64, device="cuda")
    W2[rows] = P[leg, i0]
    W2[so2[1:].to(torch.int64) + torch.arange(N, device="cuda")] = W1[M - 1::M]
    sf = torch.where(blocked[leg, i0], SUB_BLOCKED, 0).to(torch.int32)
    any_b = torch.zeros(N, dtype=torch.int32, device="cuda").index_put_((traj,), sf, accumulate=True) > 0
    fl = (torch.where(cnt.reshape(N, M).sum(dim=1) > M, SUB_DONE, 0) | torch.where(D < max_depth, SUB_FULL, 0)
          | torch.where(any_b, SUB_BLOCKED, 0)).to(torch.int32)
    return so2, W2, T2, sf, fl


for N in SIZES:
    so, W, T = S.uniform_batch(N, M)
    Sg = N * M
    dW, dT, d_so = torch.from_numpy(W).cuda().reshape(-1, 3), torch.from_numpy(T).cuda().reshape(-1), torch.from_numpy(so).cuda()
    W0 = dW.reshape(N, M + 1, 3)[:, :-1].reshape(-1, 3).contiguous()
    W1 = dW.reshape(N, M + 1, 3)[:, 1:].reshape(-1, 3).contiguous()
    cap = 16 * N
    so2 = torch.empty(N + 1, dtype=torch.int32, device="cuda")
    W2 = torch.empty((cap + N, 3), dtype=torch.float64, device="cuda")
    T2 = torch.empty(cap, dtype=torch.float64, device="cuda")
    parent = torch.empty(cap, dtype=torch.int32, device="cuda")
    seg_fl = torch.empty(cap, dtype=torch.int32, device="cuda")
    tot = torch.empty(2, dtype=torch.int64, device="cuda")
    flags = torch.empty(N, dtype=torch.int32, device="cuda")
    inf_seg = torch.empty(cap, dtype=torch.int32, device="cuda")
    s.corridor_inflate_device(N, d_so, dW, ORIGIN, H, N3, table, 0, d_seg_flags=inf_seg)
    torch.cuda.synchronize()
    before = float(((inf_seg[:Sg] & INF_BLOCKED) != 0).double().mean())
    for depth in DEPTHS:
        run = lambda: s.corridor_subdivide_device(N, d_so, dW, ORIGIN, H, N3, table, depth, so2, W2, tot, d_seg_times=dT,
                                                  d_seg_times_out=T2, d_parent=parent, d_seg_flags_out=seg_fl, d_flags=flags)
        run()
        torch.cuda.synchronize()
        S1 = int(tot[0])
        with_torch = N <= TORCH_MAX
        chain = lambda: torch_subdivide(W0, W1, dT, N, depth)
        if N == min(SIZES):
            t_so, t_W, t_T, t_sf, t_fl = chain()
            torch.cuda.synchronize()
            assert torch.equal(t_so, so2) and torch.equal(t_W, W2[:S1 + N]) and torch.equal(t_T, T2[:S1]), "torch chain differs"
            assert torch.equal(t_sf, seg_fl[:S1]) and torch.equal(t_fl, flags), "torch chain's flags differ"
            del t_so, t_W, t_T, t_sf, t_fl
        in_bytes = (Sg + N) * 24 + Sg * 8 + (N + 1) * 4
        out_bytes = (S1 + N) * 24 + S1 * 16 + (N + 1) * 4 + N * 4
        half = (in_bytes + out_bytes) // 2
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        copy = lambda: dst.copy_(src)
        for f in (run, copy) + ((chain,) if with_torch else ()):
            f(); f()
        torch.cuda.synchronize()
        ms_call, ms_copy, ms_torch = [], [], []
        for _ in range(ROUNDS):  # the windows alternate
            ms_call.append(window(run, ITERS))
            ms_copy.append(window(copy, ITERS))
            if with_torch:
                ms_torch.append(window(chain, 1))
        s.corridor_inflate_device(N, so2, W2, ORIGIN, H, N3, table, 0, d_seg_flags=inf_seg)
        torch.cuda.synchronize()
        full = (flags & SUB_FULL) != 0
        seg_full = full.repeat_interleave((so2[1:] - so2[:-1]).to(torch.int64))
        r = {"case": "subdivide %d x M=%d, %d^3, r_free %.3g, max_depth %d" % (N, M, GRID, R_FREE, depth), "N": N,
             "legs": Sg, "max_depth": depth, "segments_out": S1, "bytes_in": in_bytes, "bytes_out": out_bytes}
        r.update(stats(ms_call, ITERS))
        r.update({"ns_per_leg": r["ms"] * 1e6 / Sg, "rows_full": int(full.sum()), "rows_done": int(((flags & SUB_DONE) != 0).sum()),
                  "inflate_blocked_before": before,
                  "inflate_blocked_after": float(((inf_seg[:S1] & INF_BLOCKED) != 0).double().mean()),
                  "sub_blocked_without_full": float((((seg_fl[:S1] & SUB_BLOCKED) != 0) & ~seg_full).double().mean())})
        emit(r)
        rc = {"case": "device-to-device copy of (bytes in + bytes out) / 2, %d x M=%d, max_depth %d" % (N, M, depth), "N": N,
              "bytes": half}
        rc.update(stats(ms_copy, ITERS))
        rc["call_over_copy"] = r["ms"] / rc["ms"]
        emit(rc)
        if with_torch:
            rt = {"case": "torch chain (masked gathers per depth, cumsum, repeat_interleave), %d x M=%d, max_depth %d"
                  % (N, M, depth), "N": N}
            rt.update(stats(ms_torch, 1))
            rt["torch_over_call"] = rt["ms"] / r["ms"]
            emit(rt)
        del src, dst
    del W2, T2, parent, seg_fl, inf_seg, W0, W1
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
