"""GPU: the sampler kernel (k_sample, csrc/tgms_sample.hip), every sample of every
trajectory against the extended-precision reference and the derived per-sample bounds of
tests/sample_ref.py (p/v/a/j within 32 u S_q, the pinned sample bit-equal, psi and dpsi within
their conditioning bounds, yaw_const below the speed threshold; nothing masked).

The batches (sample_ref.py; test_sample_ref.py holds the host backend to the same bounds on
them, so a correct implementation is known to pass):
  headings    24 hand-built trajectories: axis-aligned and diagonal flight, pure vertical
              motion, end derivatives, a pinned sample faster than all others and one below
              the yaw threshold, 2 / 64 / 65 / 128 / 129 / 256 / 257 samples, knots on k*dt;
  pieces8     47 .. 97 chunks of 64 samples at pieces = 4: np = 1, 2, 3 and 4 pieces per
              trajectory, a last piece that holds the pinned sample alone;
  pieces5000, pieces7000   pieces = 3 and 2, three long trajectories among short ones;
  grid        68,536 trajectories on 65,536 workgroups: the grid-stride loop on reused LDS.
The coefficients are the host backend's solve of each batch (the sampler takes them as
input), so the inputs are the same bits here and in the CPU test."""
import numpy as np
import pytest

import sample_ref as R
from extrema_ref import check_against_samples

pytestmark = pytest.mark.gpu
MODES = [R.YAW_CONSTANT, R.YAW_VELOCITY]


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def sampled(solver):
    """name, yaw_mode -> the host-pointer call's output for that batch, computed once."""
    cache = {}

    def get(name, yaw_mode):
        if (name, yaw_mode) not in cache:
            d = R.prepared(name)
            offs, out = solver.sample(d["so"], d["W"], d["T"], d["ED"], d["C"], d["dt"], yaw_mode, R.YAW_CONST)
            assert np.array_equal(offs, d["offs"])
            out.setflags(write=False)
            cache[(name, yaw_mode)] = out
        return cache[(name, yaw_mode)]
    return get


def _check(name, yaw_mode, out):
    worst = R.check_samples(out, R.prepared(name)["ref"], yaw_mode, R.YAW_CONST)
    print(name, "yaw_mode", yaw_mode, "worst error / bound:", worst)


@pytest.mark.parametrize("yaw_mode", MODES)
def test_headings_every_sample(sampled, yaw_mode):
    _check("headings", yaw_mode, sampled("headings", yaw_mode))


def test_axis_and_diagonal_psi(sampled):
    """Flight along +-x, +-y and the four diagonals: the velocity across a line is exactly 0
    and |vx| == |vy| in every bit on a diagonal, so only the atan2's own error is left: psi
    is the reference's multiple of pi/2 (odd multiple of pi/4) to 32 u pi in every moving
    sample, and on the lines dpsi is exactly 0 (both products are)."""
    d = R.prepared("headings")
    ref, out = d["ref"], sampled("headings", R.YAW_VELOCITY)
    tol = R.K * R.U * R.PI
    for group, step in ((d["lines"], R.PI / 2), (d["diagonals"], R.PI / 4)):
        for b in group:
            r = slice(int(ref.offs[b]), int(ref.offs[b + 1]))
            fast = ~ref.slow[r]
            m = np.rint(ref.psi[r][fast] / step)
            err = np.abs(R.wrap(out[r, 12][fast].astype(R.LD) - m * step))
            assert err.max() <= tol, (b, float(err.max()))
            assert (ref.dpsi[r][fast] == 0).all()
            if step == R.PI / 2:
                assert (out[r, 13][fast] == 0.0).all()


@pytest.mark.parametrize("yaw_mode", MODES)
def test_piece_splits(sampled, yaw_mode):
    _check("pieces8", yaw_mode, sampled("pieces8", yaw_mode))


@pytest.mark.parametrize("name", ["pieces5000", "pieces7000"])
def test_piece_splits_in_large_batches(sampled, name):
    _check(name, R.YAW_VELOCITY, sampled(name, R.YAW_VELOCITY))


def test_grid_stride_reuses_lds(sampled):
    _check("grid", R.YAW_VELOCITY, sampled("grid", R.YAW_VELOCITY))


@pytest.mark.parametrize("name", ["headings", "pieces8"])
def test_no_stray_stores(solver, sampled, name):
    """The device call into a 16-B-aligned slice of a NaN-filled tensor: every row inside is
    written, every guard row (more than a 64-sample chunk's worth on either side) is still
    NaN, and the rows are the host-pointer call's bits."""
    import torch
    d = R.prepared(name)
    n, guard = int(d["offs"][-1]), 70
    buf = torch.full((guard + n + guard, 14), float("nan"), dtype=torch.float64, device="cuda")
    inner = buf[guard:guard + n]
    assert inner.data_ptr() % 16 == 0 and inner.is_contiguous()
    solver.sample_device(len(d["so"]) - 1, _dev(d["so"]), _dev(d["W"]), _dev(d["T"]), _dev(d["C"]), d["dt"],
                         _dev(d["offs"]), inner, _dev(d["ED"]), R.YAW_VELOCITY, R.YAW_CONST)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[:guard]).all() and np.isnan(got[guard + n:]).all()
    assert np.isfinite(got[guard:guard + n]).all()
    assert np.array_equal(got[guard:guard + n].view(np.int64), sampled(name, R.YAW_VELOCITY).view(np.int64))


def test_feasibility_check_on_piece_batch(solver, sampled):
    """k_extrema where a segment holds 1,500 or more samples (several rounds of four samples
    per lane, then the two- and one-sample tails), against the sampler's own output."""
    d = R.prepared("pieces8")
    ext, fl = solver.extrema(d["so"], d["W"], d["T"], d["ED"], d["C"], d["dt"])
    assert not fl.any()
    check_against_samples(ext, d["so"], d["T"], d["offs"], sampled("pieces8", R.YAW_CONSTANT))


def test_feasibility_check_on_grid_slice(solver, sampled):
    """4,096 trajectories of the grid-stride batch, across the 65,536 boundary."""
    d = R.prepared("grid")
    lo, hi = R.GRID_BLOCKS - 2048, R.GRID_BLOCKS + 2048
    so, offs = d["so"].astype(np.int64), d["offs"]
    s0, s1 = int(so[lo]), int(so[hi])
    sso = (so[lo:hi + 1] - s0).astype(np.int32)
    W, T, C, ED = d["W"][s0 + lo:s1 + hi], d["T"][s0:s1], d["C"][s0:s1], d["ED"][lo:hi]
    ext, fl = solver.extrema(sso, W, T, ED, C, d["dt"])
    assert not fl.any()
    out = sampled("grid", R.YAW_VELOCITY)[offs[lo]:offs[hi]]
    check_against_samples(ext, sso, T, offs[lo:hi + 1] - offs[lo], out)
