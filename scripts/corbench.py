#!/usr/bin/env python3
"""Corridor benchmark: tgms_corridor_batch_device with 6 and with 24 faces per segment against
the bounds call on the same batch and against what a caller had to do before it,
tgms_sample_batch_device at 100 Hz plus a torch reduction of n . p - d per segment, on two
synthetic batches, 4,096 x M = 10 and 1,048,576 x M = 10, both solved on the device.  The 6
faces are synthetic.box_corridor's (the bounding box of the segment's two waypoints grown by
CB_WIDTH), built here on the device and compared with the helper at the small size; the 24 add
18 slanted faces per segment, random unit normals with both waypoints inside by CB_WIDTH.

The samples of a batch do not fit the device at once (about 5,500 samples of 112 B per
trajectory), so the sampled path runs in chunks of CB_CHUNK trajectories into one reused
buffer; its time is the sum over the chunks of the sampler launch and the reduction (device
events per chunk; the sample offsets and each sample's segment index are built outside the timed
part).  The reduction takes the faces of a sample's segment one slot at a time (a gather of
[samples, 4], a dot product, a running maximum), then a scatter amax per segment.  The calls are
timed in alternating windows of the same run after a warm-up; the median window is reported with
the spread.  The sampled margins are compared with the continuous ones: how far they fall
short.  One JSON line per result on stdout and in CB_OUT (default
profiles/corridor_bench.jsonl, rewritten).

Work per (segment, face) item of the continuous check, worst case (every interval of every level
of the degree-6 ladder bisected): BISECTIONS * sum_{d<=6} d^2 = 40 * 91 = 3,640 Horner FMAs."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver, sample_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("CB_OUT", os.path.join(ROOT, "profiles", "corridor_bench.jsonl"))
SIZES = [(int(os.environ.get("CB_N", 4096)), int(os.environ.get("CB_ITERS", 50)), int(os.environ.get("CB_ROUNDS", 5)),
          int(os.environ.get("CB_ROUNDS_SAMPLED", 3))),
         (int(os.environ.get("CB_NBIG", 1 << 20)), int(os.environ.get("CB_ITERS_BIG", 3)),
          int(os.environ.get("CB_ROUNDS_BIG", 2)), int(os.environ.get("CB_ROUNDS_SAMPLED_BIG", 1)))]
CHUNK = int(os.environ.get("CB_CHUNK", 4096))
WIDTH = float(os.environ.get("CB_WIDTH", 2.5))
RADIUS = 0.5
M = 10; dt = 0.01
WORST_FMAS_PER_ITEM = 40 * 91
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


s = Solver(0)
gen = torch.Generator(device="cuda")
gen.manual_seed(20251015)
for n, iters, rounds, rounds_sampled in SIZES:
    if n <= 0:
        continue
    _, W, T = S.uniform_batch(n, M)
    dW, dT = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
    dC = torch.empty((n, M, 3, 8), dtype=torch.float64, device="cuda")
    s.solve_uniform_device(n, M, dW, dT, dC)
    so_h = np.arange(n + 1, dtype=np.int32) * M
    d_so = torch.from_numpy(so_h).cuda()
    ext = torch.empty((n, 10), dtype=torch.float64, device="cuda")
    rec = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    where = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    seg_rec = torch.empty((n * M, 2), dtype=torch.float64, device="cuda")
    seg_face = torch.empty((n * M,), dtype=torch.int32, device="cuda")
    fl = torch.empty((n,), dtype=torch.int32, device="cuda")
    fl_b = torch.empty((n,), dtype=torch.int32, device="cuda")  # the bounds call's
    # the chunks of the sampled path: offsets on the host once, one output buffer for the largest
    so_c = np.arange(CHUNK + 1, dtype=np.int32) * M
    chunks = []
    for n0 in range(0, n, CHUNK):
        n1 = min(n, n0 + CHUNK)
        chunks.append((n0, n1, sample_offsets(so_c[:n1 - n0 + 1], T[n0:n1].reshape(-1), dt)))
    out = torch.empty((max(int(c[2][-1]) for c in chunks), 14), dtype=torch.float64, device="cuda")
    total_samples = int(sum(int(c[2][-1]) for c in chunks))
    ends = torch.cumsum(dT, dim=1)  # [n, M]: the right end of every segment

    def bounds_window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            s.bounds_device(n, d_so, dT, dC, None, ext, fl_b)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for extra in (0, 18):
        Fs = 6 + extra
        faces = device_faces(dW, extra, gen)  # [n*M, Fs, 4]
        d_fo = torch.arange(n * M + 1, dtype=torch.int64, device="cuda") * Fs
        if extra == 0 and n <= CHUNK:
            fh, foh = S.box_corridor(so_h, W.reshape(-1, 3), WIDTH)
            assert np.array_equal(faces.reshape(-1, 4).cpu().numpy(), fh) and np.array_equal(d_fo.cpu().numpy(), foh)
        smp = torch.empty((n * M,), dtype=torch.float64, device="cuda")  # sampled m_s

        def corridor_window():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                s.corridor_device(n, d_so, dT, dC, n * M * Fs, faces, d_fo, RADIUS, rec, where, seg_rec, seg_face, fl)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters

        def sampled_pass():
            """Sampler + reduction over every chunk; returns the summed device time in ms."""
            ms = 0.0
            for n0, n1, offs in chunks:
                nc, ns = n1 - n0, int(offs[-1])
                d_offs = torch.from_numpy(offs).cuda()
                cnt = torch.from_numpy(np.diff(offs)).cuda()
                tr = torch.repeat_interleave(torch.arange(nc, device="cuda"), cnt)
                t = (torch.arange(ns, device="cuda") - d_offs[:-1][tr]).to(torch.float64) * dt
                seg = tr * M + (t[:, None] >= ends[n0:n1][tr][:, :-1]).sum(1)  # each sample's segment in the chunk
                fc = faces[n0 * M:n1 * M]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s.sample_device(nc, d_so[:nc + 1], dW[n0:n1], dT[n0:n1], dC[n0:n1], dt, d_offs, out)
                p = out[:ns, 0:3]
                m = torch.full((ns,), float("-inf"), dtype=torch.float64, device="cuda")
                for j in range(Fs):
                    f = fc[:, j, :][seg]
                    m = torch.maximum(m, (p * f[:, :3]).sum(1) - f[:, 3])
                smp[n0 * M:n1 * M] = torch.full((nc * M,), float("-inf"), dtype=torch.float64,
                                                device="cuda").scatter_reduce_(0, seg, m, "amax")
                e1.record(); torch.cuda.synchronize()
                ms += e0.elapsed_time(e1)
                del d_offs, cnt, tr, t, seg, p, m, f
            return ms

        corridor_window(); bounds_window()  # warm-up
        if n <= CHUNK:
            sampled_pass()
        ms = {"corridor": [], "bounds": [], "sampled": []}
        for k in range(rounds):  # alternating windows
            ms["corridor"].append(corridor_window())
            ms["bounds"].append(bounds_window())
            if k < rounds_sampled:
                ms["sampled"].append(sampled_pass())
        short = seg_rec[:, 0] - smp
        emit({"check": "how far the sampled margins at 100 Hz fall short of the continuous ones", "B": n,
              "faces_per_segment": Fs, "finite": bool(torch.isfinite(seg_rec).all()),
              "outside": int(((fl & 1) != 0).sum()), "nonfinite_or_bad_face": int(((fl & ~1) != 0).sum()),
              "short_max": float(short.max()), "short_mean": float(short.mean()),
              "continuous_below_sampled_worst": float(short.min()),
              "segments_sampled_inside_continuous_outside": int(((seg_rec[:, 0] > -RADIUS) & ~(smp > -RADIUS)).sum()),
              "m_max_largest": float(rec[:, 0].max()), "m_max_least": float(rec[:, 0].min())})
        v = ms["corridor"]
        emit({"kernel": "corridor", "B": n, "M": M, "faces_per_segment": Fs, "ms": float(np.median(v)), "ms_min": min(v),
              "ms_max": max(v), "iters": iters, "rounds": rounds, "ns_per_item": float(np.median(v)) * 1e6 / (n * M * Fs),
              "worst_case_fma_frac": n * M * Fs * WORST_FMAS_PER_ITEM / (78.6e12 / 2) / (float(np.median(v)) * 1e-3)})
        v = ms["bounds"]
        emit({"kernel": "bounds", "B": n, "M": M, "beside_faces_per_segment": Fs, "ms": float(np.median(v)),
              "ms_min": min(v), "ms_max": max(v), "iters": iters, "rounds": rounds})
        v = ms["sampled"]
        emit({"kernel": "sample + torch reduction", "B": n, "M": M, "faces_per_segment": Fs, "dt": dt,
              "ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "rounds": len(v), "chunk": CHUNK,
              "chunks": len(chunks), "samples": total_samples})
        emit({"B": n, "faces_per_segment": Fs,
              "corridor_over_bounds": float(np.median(ms["corridor"]) / np.median(ms["bounds"])),
              "sampled_over_continuous": float(np.median(ms["sampled"]) / np.median(ms["corridor"]))})
        del faces, d_fo, smp
    del dW, dT, dC, d_so, ext, rec, where, seg_rec, seg_face, fl, fl_b, out, ends
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
