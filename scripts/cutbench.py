#!/usr/bin/env python3
"""Cut benchmark: tgms_cut_batch_device on two synthetic batches, 4,096 x M = 10 and 1,048,576 x
M = 10, solved on the device and cut at times uniform in [0, 1.05 D] (so a twentieth of the rows
finish), min_frac 0.25.  Reported, all from the same run, in alternating windows after a warm-up,
medians with the spread:
  - the cut call with and without coeffs_out;
  - the floor of each: one device-to-device hipMemcpyAsync whose traffic equals the bytes the call
    must move, its inputs read once (the coefficients too: the call has to see every one of them
    to tell a usable trajectory) and its outputs (S' segments) written once.  A copy of n bytes
    reads n and writes n, so the copy is of (inputs + outputs) / 2 bytes;
  - what a caller had before, in torch on the device: cumsum for the knots, a comparison count for
    the segment, Horner and the binomial shift for the state and the first row, cumsum of the new
    counts, the total through the host, repeat_interleave and index_select for the rows.  It
    evaluates the state itself where a caller with tgms_sample_batch_device would sample the whole
    trajectory and gather one sample, applies no min_frac and holds no finished row, so it does
    less than the call;
  - one tick (cut + solve of the tail) beside the solve of the tail alone.
One JSON line per result on stdout and in CB_OUT (default profiles/cut_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from math import comb
import numpy as np
import torch
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("CB_OUT", os.path.join(ROOT, "profiles", "cut_bench.jsonl"))
SIZES = [(int(os.environ.get("CB_N", 4096)), int(os.environ.get("CB_ITERS", 50)), int(os.environ.get("CB_ROUNDS", 5))),
         (int(os.environ.get("CB_NBIG", 1 << 20)), int(os.environ.get("CB_ITERS_BIG", 3)),
          int(os.environ.get("CB_ROUNDS_BIG", 3)))]
MIN_FRAC, M = 0.25, 10
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


def stats(v):
    return {"ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)}


s = Solver(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(20261020)
f64, i32, i64 = (dict(dtype=t, device="cuda") for t in (torch.float64, torch.int32, torch.int64))
BINOM = torch.tensor([[float(comb(j, k)) for j in range(8)] for k in range(8)], **f64)  # [k, j]
POW = torch.tensor([[max(j - k, 0) for j in range(8)] for k in range(8)], **f64)
for n, iters, rounds in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    Sg = n * M
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), **f64)
    d_so = torch.arange(n + 1, **i32) * M
    s.solve_uniform_device(n, M, dW, dT, dC)
    t_cut = torch.rand((n,), generator=gen, **f64) * 1.05 * dT.sum(1)
    so2, W2, T2 = torch.empty((n + 1,), **i32), torch.empty((Sg + n, 3), **f64), torch.empty((Sg,), **f64)
    ED2, C2, parent = torch.empty((n, 18), **f64), torch.empty((Sg, 3, 8), **f64), torch.empty((Sg,), **i32)
    t0, totals, fl = torch.empty((n,), **f64), torch.zeros((1,), **i64), torch.empty((n,), **i32)
    cut = lambda: s.cut_device(n, d_so, dW, dT, dC, t_cut, MIN_FRAC, so2, W2, T2, ED2, totals, d_coeffs_out=C2,
                               d_parent=parent, d_t0_out=t0, d_flags=fl)
    cut_nc = lambda: s.cut_device(n, d_so, dW, dT, dC, t_cut, MIN_FRAC, so2, W2, T2, ED2, totals, d_parent=parent,
                                  d_t0_out=t0, d_flags=fl)
    cut(); torch.cuda.synchronize()
    S1 = int(totals[0])
    h_so2 = so2.cpu().numpy()
    C3, st3 = torch.empty((S1, 3, 8), **f64), torch.empty((n,), **i32)
    solve_tail = lambda: s.solve_batch_device(h_so2, so2, W2, T2, C3, st3, d_end_derivs=ED2)
    solve_tail(); torch.cuda.synchronize()
    assert not st3.any()
    err = float(((C3 - C2[:S1]).abs().amax(2) / C2[:S1].abs().amax(2).clamp(min=1e-300)).median())
    in_bytes = 4 * (n + 1) + 24 * (Sg + n) + 8 * Sg + 192 * Sg + 8 * n
    out_nc = 4 * (n + 1) + 24 * (S1 + n) + 8 * S1 + 144 * n + 4 * S1 + 8 * n + 8 + 4 * n
    half = {"coeffs": (in_bytes + out_nc + 192 * S1) // 2, "no coeffs": (in_bytes + out_nc) // 2}
    bufs = {k: (torch.empty((v,), dtype=torch.uint8, device="cuda"), torch.empty((v,), dtype=torch.uint8, device="cuda"))
            for k, v in half.items()}
    floor = lambda: bufs["coeffs"][1].copy_(bufs["coeffs"][0], non_blocking=True)  # hipMemcpyAsync, device to device
    floor_nc = lambda: bufs["no coeffs"][1].copy_(bufs["no coeffs"][0], non_blocking=True)

    def torch_chain():
        knot = torch.cumsum(dT, 1)
        D = knot[:, -1]
        tc = torch.minimum(t_cut.clamp(min=0.0), D)
        sidx = (knot[:, :-1] <= tc[:, None]).sum(1)
        rows = torch.arange(n, device="cuda")
        k_s = torch.where(sidx > 0, knot[rows, (sidx - 1).clamp(min=0)], torch.zeros_like(D))
        tl = (tc - k_s).clamp(min=0.0)
        c = dC[rows, sidx]                                                  # [n, 3, 8]
        sh = (c[:, :, None, :] * (BINOM * tl[:, None, None] ** POW)[:, None]).sum(3)  # the Taylor shift [n, 3, 8]
        ed = torch.zeros((n, 18), **f64)
        ed[:, 0:3], ed[:, 3:6], ed[:, 6:9] = sh[:, :, 1], 2.0 * sh[:, :, 2], 6.0 * sh[:, :, 3]
        cnt = M - sidx
        so_t = torch.zeros((n + 1,), **i64)
        so_t[1:] = torch.cumsum(cnt, 0)
        total = int(so_t[-1])  # through the host: the sizes of everything below
        tr = torch.repeat_interleave(rows, cnt, output_size=total)
        par = torch.arange(total, device="cuda") - so_t[tr] + sidx[tr] + tr * M
        Tn = torch.index_select(dT.reshape(-1), 0, par)
        Tn[so_t[:-1]] = dT[rows, sidx] - tl
        Cn = torch.index_select(dC.reshape(Sg, 3, 8), 0, par)
        Cn[so_t[:-1]] = sh
        Wn = torch.empty((total + n, 3), **f64)
        Wn[torch.arange(total, device="cuda") + tr] = dW[tr, par - tr * M]
        Wn[so_t[:-1] + rows] = sh[:, :, 0]
        Wn[so_t[1:] + rows] = dW[:, -1]
        return so_t, Wn, Tn, ed, Cn, par

    tcn = torch_chain()
    assert int(tcn[0][-1]) >= S1  # without min_frac and the hold rows it keeps no fewer segments
    del tcn
    for fn in (cut, cut_nc, floor, floor_nc, solve_tail):
        window(fn, 2)
    ms = {k: [] for k in ("cut", "cut_nc", "floor", "floor_nc", "torch", "solve", "tick")}
    for _ in range(rounds):  # alternating windows
        ms["cut"].append(window(cut, iters))
        ms["floor"].append(window(floor, iters))
        ms["cut_nc"].append(window(cut_nc, iters))
        ms["floor_nc"].append(window(floor_nc, iters))
        ms["torch"].append(window(torch_chain, max(1, iters // 5)))
        ms["solve"].append(window(solve_tail, iters))
        ms["tick"].append(window(lambda: (cut(), solve_tail()), iters))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    base = {"B": n, "M": M}
    emit(dict(base, what="batch", S=Sg, S_out=S1, in_bytes=in_bytes, out_bytes=out_nc + 192 * S1,
              out_bytes_no_coeffs=out_nc, done_rows=int(((fl & 1) != 0).sum()), snapped_rows=int(((fl & 2) != 0).sum()),
              finished_rows=int(((fl & 4) != 0).sum()), resolve_median_rel_err=err))
    emit(dict(base, kernel="cut", iters=iters, rounds=rounds, **stats(ms["cut"]),
              tb_per_s=(in_bytes + out_nc + 192 * S1) / (med["cut"] * 1e-3) / 1e12))
    emit(dict(base, kernel="memcpy floor", copy_bytes=half["coeffs"], **stats(ms["floor"])))
    emit(dict(base, kernel="cut, no coeffs_out", **stats(ms["cut_nc"]),
              tb_per_s=(in_bytes + out_nc) / (med["cut_nc"] * 1e-3) / 1e12))
    emit(dict(base, kernel="memcpy floor, no coeffs_out", copy_bytes=half["no coeffs"], **stats(ms["floor_nc"])))
    emit(dict(base, kernel="torch chain", **stats(ms["torch"])))
    emit(dict(base, kernel="solve of the tail", **stats(ms["solve"])))
    emit(dict(base, kernel="cut + solve", **stats(ms["tick"])))
    emit(dict(base, cut_over_floor=med["cut"] / med["floor"], cut_nc_over_floor=med["cut_nc"] / med["floor_nc"],
              torch_over_cut=med["torch"] / med["cut"], tick_over_solve=med["tick"] / med["solve"]))
    del dW, dT, dC, d_so, t_cut, so2, W2, T2, ED2, C2, parent, t0, totals, fl, C3, st3, bufs
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
