#!/usr/bin/env python3
"""Distance-field build benchmark: tgms_field_edt_device on the field scene of fldbench.py (64
seeded boxes rasterised by synthetic.box_occupancy on EB_GRID^3 = 128^3 nodes over the room, h =
94 mm), unsigned and signed, with max_dist = 1 m and with a cap above the grid's diagonal (nothing
capped: every line pass folds whole lines).  Per case the time (device events around EB_ITERS
launches, EB_ROUNDS windows after a warm-up; median with its range).  In the same run, to measure
against:
  - device-to-device copies that move the bytes each pass must move (x: N occupancy bytes in, 4 N
    out; y: 4 N in, 4 N out; z: 4 N + N in, 4 N out) and their sum; the per-pass kernel times come
    from rocprofv3 --kernel-trace --stats runs of this script's trace mode (EB_TRACE = cap or
    full: the one call, 50 times, nothing else), whose CSVs EB_TRACE_DIR names; without them the
    per-pass rows say "not measured";
  - the formulation a caller has today on the device: a torch min-plus per axis with broadcasting
    on int32 squares, chunked to fit, then the square root; checked for equality with the call
    before it is timed;
  - the host backend's tgms_field_edt plus one upload of the values: the CPU alternative;
  - the neighbouring steps on the built field: the table build (tgms_field_occupancy_device,
    r_free 0.3) and one tgms_field_clearance_batch_device of 65,536 x M = 10 at tol 1e-2;
  - EB_BIG^3 = 256^3 once per case (the call only).
One JSON line per result on stdout and in EB_OUT (default profiles/edt_bench.jsonl, rewritten)."""
import csv, glob, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trajectory_generator_ros2_amd import synthetic as S
from trajectory_generator_ros2_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("EB_OUT", os.path.join(ROOT, "profiles", "edt_bench.jsonl"))
ROUNDS = int(os.environ.get("EB_ROUNDS", 5))
ITERS = int(os.environ.get("EB_ITERS", 20))
GRID = int(os.environ.get("EB_GRID", 128))
BIG = int(os.environ.get("EB_BIG", 256))
TRACE = os.environ.get("EB_TRACE", "")
TRACE_DIR = os.environ.get("EB_TRACE_DIR", "")
N_TRAJ, M, K_BOXES, R_FREE, TOL = int(os.environ.get("EB_TRAJ", 65536)), 10, 64, 0.3, 1e-2
ORIGIN = (-6.0, -6.0, -0.5)
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


def scene(grid):
    h = 12.0 / (grid - 1)
    occ = S.box_occupancy(boxes(K_BOXES, 64), ORIGIN, h, (grid,) * 3)
    return h, occ, {"cap 1 m": 1.0, "no cap": h * (np.sqrt(3.0) * grid + 2.0)}


s = Solver(0)


class Call:
    """The device call on one grid with its buffers."""

    def __init__(self, grid):
        self.grid, self.n = grid, (grid,) * 3
        self.h, self.occ, self.caps = scene(grid)
        self.d_occ = torch.from_numpy(self.occ).cuda()
        self.work = torch.empty(s.field_edt_work_size(ORIGIN, self.h, self.n) // 4, dtype=torch.int32, device="cuda")
        self.values = torch.empty(self.occ.shape, dtype=torch.float32, device="cuda")
        self.d2 = torch.empty(self.occ.shape, dtype=torch.int32, device="cuda")

    def run(self, max_dist, signed=False, d2=False):
        s.field_edt_device(ORIGIN, self.h, self.n, self.d_occ, max_dist, self.work, self.values,
                           self.d2 if d2 else None, signed)


c = Call(GRID)
if TRACE:  # under rocprofv3: one case, nothing else
    md = c.caps["cap 1 m" if TRACE == "cap" else "no cap"]
    for _ in range(50):
        c.run(md)
    torch.cuda.synchronize()
    sys.exit(0)

N = GRID ** 3
emit({"scene": "%d boxes rasterised on %d^3, h %.4g" % (K_BOXES, GRID, c.h), "occupied_nodes": int(c.occ.sum()),
      "work_bytes": int(c.work.numel() * 4)})

# ---- the call ----
per = {}
for cap_name, md in c.caps.items():
    for signed in (False, True):
        r = {"case": "edt %d^3, %s, %s, values only" % (GRID, "signed" if signed else "unsigned", cap_name),
             "grid": GRID, "signed": signed, "max_dist": md, "launches": 6 if signed else 3}
        r.update(timed(lambda: c.run(md, signed), ITERS))
        emit(r)
        per[(cap_name, signed)] = r["ms"]
    r = {"case": "edt %d^3, unsigned, %s, values and d2" % (GRID, cap_name), "grid": GRID, "max_dist": md}
    r.update(timed(lambda: c.run(md, False, True), ITERS))
    emit(r)

# ---- copies of the bytes each pass must move (a copy of X bytes moves 2 X) ----
pass_bytes = {"k_edt_rows": 5 * N, "k_edt_lines<false>": 8 * N, "k_edt_lines<true>": 9 * N}
copy_ms = {}
for name, b in list(pass_bytes.items()) + [("total", sum(pass_bytes.values()))]:
    src = torch.empty(b // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    r = {"case": "device-to-device copy moving the bytes of %s" % name, "bytes_moved": b}
    r.update(timed(lambda: dst.copy_(src), ITERS))
    r["tb_per_s"] = b / r["ms"] * 1e-9
    emit(r)
    copy_ms[name] = r["ms"]
    del src, dst
for cap_name in c.caps:
    emit({"case": "edt %d^3 unsigned, %s, over the copy of all three passes' bytes" % (GRID, cap_name),
          "call_over_copy": per[(cap_name, False)] / copy_ms["total"],
          "copy_share_reached": copy_ms["total"] / per[(cap_name, False)]})


def kernel_stats(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            rows[row["Name"]] = float(row["AverageNs"]) * 1e-6
    return rows


for cap_name, sub in (("cap 1 m", "cap"), ("no cap", "full")):
    st = kernel_stats(os.path.join(TRACE_DIR, sub)) if TRACE_DIR else {}
    for name, b in pass_bytes.items():
        keys = {"k_edt_rows": ("k_edt_rows",), "k_edt_lines<false>": ("k_edt_lines<false>", "k_edt_linesILb0E"),
                "k_edt_lines<true>": ("k_edt_lines<true>", "k_edt_linesILb1E")}[name]
        ms = next((v for k, v in st.items() if any(x in k for x in keys)), None)
        r = {"case": "pass %s, %d^3 unsigned, %s (rocprofv3 kernel trace, mean of 50)" % (name, GRID, cap_name),
             "bytes_moved": b, "ms": ms if ms is not None else "not measured"}
        if ms is not None:
            r["copy_ms"] = copy_ms[name]
            r["copy_share_reached"] = copy_ms[name] / ms
        emit(r)

# ---- the torch formulation: min-plus per axis with broadcasting on int32 squares ----
FAR = 1 << 29


def minplus(f, axis, chunk=1 << 27):
    f = f.movedim(axis, -1)
    shape, n = f.shape, f.shape[-1]
    f = f.reshape(-1, n)
    j = torch.arange(n, device="cuda", dtype=torch.int32)
    d2 = (j[:, None] - j[None, :]) ** 2
    out = torch.empty_like(f)
    step = max(1, chunk // (n * n))
    for lo in range(0, f.shape[0], step):
        out[lo:lo + step] = (f[lo:lo + step, None, :] + d2[None]).amin(dim=-1)
    return out.reshape(shape).movedim(-1, axis)


def torch_edt(d_occ, h, max_dist):
    f = torch.where(d_occ != 0, 0, FAR).to(torch.int32)
    for axis in (2, 1, 0):
        f = minplus(f, axis).contiguous()
    dist = torch.tensor(h, dtype=torch.float64, device="cuda") * torch.sqrt(f.to(torch.float64))
    return torch.clamp(dist, max=max_dist).to(torch.float32), f


for cap_name, md in c.caps.items():
    c.run(md, False, True)
    tv, tf = torch_edt(c.d_occ, c.h, md)
    torch.cuda.synchronize()
    R = int(c.d2.max().item()) if cap_name == "cap 1 m" else None
    assert torch.equal(c.values.view(torch.int32), tv.view(torch.int32)), "the torch formulation's values differ"
    assert torch.equal(c.d2, tf if R is None else torch.clamp(tf, max=R)), "the torch formulation's squares differ"
    rt = {"case": "torch min-plus per axis + sqrt, %d^3 unsigned, %s (no window: it cannot use the cap)" % (GRID, cap_name),
          "equal_to_the_call": True}
    rt.update(timed(lambda: torch_edt(c.d_occ, c.h, md), 1, rounds=3))
    rt["torch_over_call"] = rt["ms"] / per[(cap_name, False)]
    emit(rt)
    del tv, tf

# ---- the host backend and one upload of its values ----
with Solver(host=True) as hs:
    for cap_name, md in c.caps.items():
        hs.field_edt(c.occ, ORIGIN, c.h, md)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            hv, _ = hs.field_edt(c.occ, ORIGIN, c.h, md)
            t.append((time.perf_counter() - t0) * 1e3)
        c.run(md)
        torch.cuda.synchronize()
        assert np.array_equal(hv.view(np.int32), c.values.cpu().numpy().view(np.int32)), "host and device differ"
        up = timed(lambda: c.values.copy_(torch.from_numpy(hv)), 5)
        emit({"case": "host backend tgms_field_edt %d^3 unsigned, %s, one thread, plus the upload of the values" % (GRID, cap_name),
              "host_ms": float(np.median(t)), "host_ms_min": min(t), "host_ms_max": max(t), "upload_ms": up["ms"],
              "upload_bytes": 4 * N, "host_plus_upload_over_call": (float(np.median(t)) + up["ms"]) / per[(cap_name, False)],
              "equal_to_the_call": True})

# ---- the neighbouring steps on the built field ----
md = c.caps["no cap"]
c.run(md)
table = torch.empty((GRID + 1,) * 3, dtype=torch.int32, device="cuda")
rb = {"case": "table build %d^3 on the built field, r_free %.3g (three launches)" % (GRID, R_FREE)}
rb.update(timed(lambda: s.field_occupancy_device(ORIGIN, c.h, c.n, c.values, R_FREE, table), ITERS))
emit(rb)
so, W, T = S.uniform_batch(N_TRAJ, M)
dW, dT, d_so = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(so).cuda()
dC = torch.empty((N_TRAJ, M, 3, 8), dtype=torch.float64, device="cuda")
s.solve_uniform_device(N_TRAJ, M, dW, dT, dC)
near = torch.empty((N_TRAJ, 2), dtype=torch.float64, device="cuda")
evals, flags = (torch.empty((N_TRAJ,), dtype=torch.int32, device="cuda") for _ in range(2))
v = c.values.cpu().numpy().astype(np.float64)
lip = float(np.sqrt(sum((np.abs(np.diff(v, axis=a)).max() / c.h) ** 2 for a in range(3))))
rf = {"case": "field clearance %d x M=%d on the built field, r_min %.3g, tol %.0e, lip given" % (N_TRAJ, M, R_FREE, TOL),
      "lip_from_values": lip}
rf.update(timed(lambda: s.field_clearance_device(N_TRAJ, d_so, dT, dC, ORIGIN, c.h, c.n, c.values, lip, R_FREE, TOL,
                                                 1 << 20, near, evals, flags), 2))
emit(rf)
for cap_name in c.caps:
    for signed in (False, True):
        e = per[(cap_name, signed)]
        emit({"case": "share of a map update (edt + table build + one clearance call), %s, %s" %
              ("signed" if signed else "unsigned", cap_name), "edt_ms": e, "table_ms": rb["ms"], "clearance_ms": rf["ms"],
              "edt_share": e / (e + rb["ms"] + rf["ms"]), "edt_over_table_build": e / rb["ms"]})
del dW, dT, dC, near, table

# ---- the larger grid, once ----
if BIG > GRID:
    del c
    b = Call(BIG)
    for cap_name, md in b.caps.items():
        for signed in (False, True):
            r = {"case": "edt %d^3, %s, %s, values only" % (BIG, "signed" if signed else "unsigned", cap_name),
                 "grid": BIG, "signed": signed, "max_dist": md, "work_bytes": int(b.work.numel() * 4)}
            r.update(timed(lambda: b.run(md, signed), 5, rounds=3))
            emit(r)
    src = torch.empty(11 * BIG ** 3, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    r = {"case": "device-to-device copy moving the bytes of all three passes, %d^3" % BIG, "bytes_moved": 22 * BIG ** 3}
    r.update(timed(lambda: dst.copy_(src), 5, rounds=3))
    emit(r)

os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    for d in results:
        f.write(json.dumps(d) + "\n")
