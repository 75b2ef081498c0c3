#!/usr/bin/env python3
"""Split benchmark: tgms_corridor_split_batch_device on two synthetic batches, 4,096 x M = 10 and
1,048,576 x M = 10, solved and checked against their corridors on the device, with 6 faces per
segment (synthetic.box_corridor's, built here on the device as in corbench.py) and with 24, at
the README's width and radius.  Reported, all from the same run, in alternating windows after a
warm-up, medians with the spread:
  - the split call (PULL mode, min_frac 0.1);
  - the floor: one device-to-device hipMemcpyAsync whose traffic equals the bytes the call must
    move, its inputs read once and its outputs (S' segments, F' faces) written once.  A copy of n
    bytes reads n and writes n, so the copy is of (inputs + outputs) / 2 bytes;
  - what a caller had before, in torch on the device: the wanted mask from seg_rec, cumsum of the
    new counts, repeat_interleave of segments and of face rows, index_select, and Horner at t_s
    for the inserted waypoints.  It applies neither the segment cap nor the at-a-waypoint rule
    (M = 10 leaves room for 6 splits), so it does a little less than the call;
  - one loop round (solve + corridor + split) beside the solve alone.
One JSON line per result on stdout and in SB_OUT (default profiles/split_bench.jsonl, rewritten)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import SPLIT_PULL, synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("SB_OUT", os.path.join(ROOT, "profiles", "split_bench.jsonl"))
SIZES = [(int(os.environ.get("SB_N", 4096)), int(os.environ.get("SB_ITERS", 50)), int(os.environ.get("SB_ROUNDS", 5))),
         (int(os.environ.get("SB_NBIG", 1 << 20)), int(os.environ.get("SB_ITERS_BIG", 3)),
          int(os.environ.get("SB_ROUNDS_BIG", 3)))]
WIDTH = float(os.environ.get("SB_WIDTH", 2.5))
RADIUS, MIN_FRAC, M = 0.5, 0.1, 10
results = []


def emit(d):
    print(json.dumps(d), flush=True)
    results.append(d)


def device_faces(dW, extra, gen):
    """[n*M, 6 + extra, 4] on the device: box_corridor's six faces, then `extra` slanted ones."""
    w0, w1 = dW[:, :-1].reshape(-1, 3), dW[:, 1:].reshape(-1, 3)
    lo, hi = torch.minimum(w0, w1) - WIDTH, torch.maximum(w0, w1) + WIDTH
    f = torch.zeros((w0.shape[0], 6 + extra, 4), dtype=torch.float64, device="cuda")
    for ax in range(3):
        f[:, 2 * ax, ax], f[:, 2 * ax, 3] = 1.0, hi[:, ax]
        f[:, 2 * ax + 1, ax], f[:, 2 * ax + 1, 3] = -1.0, -lo[:, ax]
    if extra:
        nrm = torch.randn((w0.shape[0], extra, 3), dtype=torch.float64, device="cuda", generator=gen)
        nrm = nrm / nrm.norm(dim=2, keepdim=True)
        f[:, 6:, :3] = nrm
        f[:, 6:, 3] = torch.maximum((nrm * w0[:, None, :]).sum(2), (nrm * w1[:, None, :]).sum(2)) + WIDTH
    return f


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
gen.manual_seed(20251015)
f64, i32, i64 = (dict(dtype=t, device="cuda") for t in (torch.float64, torch.int32, torch.int64))
for n, iters, rounds in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    Sg = n * M
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), **f64)
    d_so = torch.arange(n + 1, **i32) * M
    seg_rec, seg_face, fl = torch.empty((Sg, 2), **f64), torch.empty((Sg,), **i32), torch.empty((n,), **i32)
    so2, W2, T2 = torch.empty((n + 1,), **i32), torch.empty((2 * Sg + n, 3), **f64), torch.empty((2 * Sg,), **f64)
    fo2, parent = torch.empty((2 * Sg + 1,), **i64), torch.empty((2 * Sg,), **i32)
    totals, sfl = torch.zeros((2,), **i64), torch.empty((n,), **i32)
    solve = lambda: s.solve_uniform_device(n, M, dW, dT, dC)
    solve()
    for extra in (0, 18):
        Fs = 6 + extra
        faces = device_faces(dW, extra, gen).reshape(-1, 4)
        d_fo = torch.arange(Sg + 1, **i64) * Fs
        F = Sg * Fs
        faces2 = torch.empty((2 * F, 4), **f64)
        corridor = lambda: s.corridor_device(n, d_so, dT, dC, F, faces, d_fo, RADIUS, d_seg_rec=seg_rec,
                                             d_seg_face=seg_face, d_flags=fl)
        split = lambda: s.corridor_split_device(n, d_so, dW, dT, dC, F, faces, d_fo, seg_rec, seg_face, RADIUS,
                                                SPLIT_PULL, MIN_FRAC, so2, W2, T2, faces2, fo2, parent, totals, sfl)
        corridor(); split(); torch.cuda.synchronize()
        S1, F1 = (int(x) for x in totals.tolist())
        in_bytes = 4 * (n + 1) + 24 * (Sg + n) + 8 * Sg + 192 * Sg + 32 * F + 8 * (Sg + 1) + 16 * Sg + 4 * Sg
        out_bytes = 4 * (n + 1) + 24 * (S1 + n) + 8 * S1 + 32 * F1 + 8 * (S1 + 1) + 4 * S1 + 16 + 4 * n
        half = (in_bytes + out_bytes) // 2
        src, dst = torch.empty((half,), dtype=torch.uint8, device="cuda"), torch.empty((half,), dtype=torch.uint8, device="cuda")
        floor = lambda: dst.copy_(src, non_blocking=True)  # hipMemcpyAsync, device to device

        def torch_chain():
            m, ts = seg_rec[:, 0], seg_rec[:, 1]
            want = m > -RADIUS
            cnt = 1 + want.to(torch.int64)
            so_t = torch.zeros((n + 1,), **i64)
            so_t[1:] = torch.cumsum(cnt.view(n, M).sum(1), 0)
            par = torch.repeat_interleave(torch.arange(Sg, device="cuda"), cnt)
            first = torch.cumsum(cnt, 0) - cnt  # a segment's first child
            Tf = dT.reshape(-1)
            knot = (torch.cumsum(dT, 1) - dT).reshape(-1)
            tl = torch.minimum(torch.maximum(torch.clamp(ts - knot, min=0.0), MIN_FRAC * Tf), Tf - MIN_FRAC * Tf)
            Tn = Tf[par]
            w = torch.nonzero(want).reshape(-1)
            Tn[first[w]] = tl[w]
            Tn[first[w] + 1] = Tf[w] - tl[w]
            c = dC.reshape(Sg, 3, 8)[w]
            x = c[:, :, 7]
            for j in range(6, -1, -1):
                x = x * tl[w, None] + c[:, :, j]
            f = faces[seg_face[w].to(torch.int64)]
            q = (f[:, :3] * x).sum(1) - f[:, 3]
            x = x - (torch.clamp(q + RADIUS, min=0.0) / (f[:, :3] ** 2).sum(1))[:, None] * f[:, :3]
            Wn = torch.empty((int(so_t[-1]) + n, 3), **f64)
            tr = torch.arange(Sg, device="cuda") // M
            Wn[first + tr] = dW[:, :-1].reshape(-1, 3)
            Wn[first[w] + tr[w] + 1] = x
            Wn[so_t[1:] + torch.arange(n, device="cuda")] = dW[:, -1]
            fo_t = torch.zeros((par.shape[0] + 1,), **i64)
            fo_t[1:] = torch.cumsum(torch.full_like(par, Fs), 0)
            rows = (par[:, None] * Fs + torch.arange(Fs, device="cuda")[None, :]).reshape(-1)
            return so_t, Wn, Tn, torch.index_select(faces, 0, rows), fo_t, par

        tc = torch_chain()
        assert int(tc[0][-1]) >= S1 and tc[3].shape[0] >= F1  # without the cap it splits no fewer
        del tc
        for fn in (split, floor, solve, corridor):
            window(fn, 2)
        ms = {k: [] for k in ("split", "floor", "torch", "solve", "corridor", "round")}
        for _ in range(rounds):  # alternating windows
            ms["split"].append(window(split, iters))
            ms["floor"].append(window(floor, iters))
            ms["torch"].append(window(torch_chain, max(1, iters // 5)))
            ms["solve"].append(window(solve, iters))
            ms["corridor"].append(window(corridor, iters))
            ms["round"].append(window(lambda: (solve(), corridor(), split()), iters))
        base = {"B": n, "M": M, "faces_per_segment": Fs}
        emit(dict(base, what="batch", S=Sg, S_out=S1, F=F, F_out=F1, in_bytes=in_bytes, out_bytes=out_bytes,
                  split_rows=int(((sfl & 1) != 0).sum()), full_rows=int(((sfl & 2) != 0).sum()),
                  at_end_rows=int(((sfl & 4) != 0).sum()), outside_rows=int(((fl & 1) != 0).sum())))
        emit(dict(base, kernel="split", iters=iters, rounds=rounds, **stats(ms["split"]),
                  tb_per_s=(in_bytes + out_bytes) / (float(np.median(ms["split"])) * 1e-3) / 1e12))
        emit(dict(base, kernel="memcpy floor", copy_bytes=half, **stats(ms["floor"])))
        emit(dict(base, kernel="torch chain", **stats(ms["torch"])))
        emit(dict(base, kernel="solve", **stats(ms["solve"])))
        emit(dict(base, kernel="corridor", **stats(ms["corridor"])))
        emit(dict(base, kernel="solve + corridor + split", **stats(ms["round"])))
        emit(dict(base, split_over_floor=float(np.median(ms["split"]) / np.median(ms["floor"])),
                  torch_over_split=float(np.median(ms["torch"]) / np.median(ms["split"])),
                  round_over_solve=float(np.median(ms["round"]) / np.median(ms["solve"]))))
        del faces, faces2, d_fo, src, dst
    del dW, dT, dC, d_so, seg_rec, seg_face, fl, so2, W2, T2, fo2, parent, totals, sfl
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
