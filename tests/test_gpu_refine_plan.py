"""The ragged refinement loop's device plan under its cached graph (tgms_refine_loop_device on a
ragged batch: k_perm_hist and k_plan_scatter build the plan on the device, k_refine_loop_dev
runs once per occupancy class, all captured into a graph that run_loop_graph caches by sizes,
pointers and scalars).  csrc/tgms_internal.h: "a captured graph stays valid for any offsets of
the same B and S: each replay regroups".  Held here:

  1. the same graph replayed on other offsets of the same B and S (every M, then an empty
     one-wave class, then two M with partial tiles, then the first batch reordered), and
     ragged -> uniform -> ragged on the same tensors;
  2. the planner's shape corners: B around its block of 1,024, 31 / 32 / 33 trajectories of one
     M, an empty two-wave class, more than 64 planner blocks, the persistent threshold;
  3. the graph cache: 17 keys through 16 entries, nullable outputs in the key, eviction with
     replays in flight;
  4. device offsets that disagree with the host's, on the plain handle.

Two references.  The independent one is the oracle's restatement of the loop at the 1e-9 of
test_gpu_parity.py::test_refine_matches_oracle (times, costs, coefficients norm-wise per
trajectory, every status 0).  The same-kernel one is a call on a fresh handle with fresh
tensors (a new capture, nothing stale) or, for the large batches, calls on chunks small enough
for one planner block or one block per tile: bit-equal, since which wave takes which tile does
not change a tile's arithmetic.  Every call starts from outputs prefilled with NaN (statuses
-1), so a trajectory no tile visited shows."""
import numpy as np
import pytest

import refine_plan_ref as P
from conftest import batch_rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9
K_T, ETA, ITERS = 1.0, 0.1, 3


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Slots:
    """Device tensors of one (B, S) allocated once, written in place per batch: the pointers,
    and so the loop graph's key, stay the same from call to call."""

    def __init__(self, B, n_seg, with_ed, n_seg_alloc=None):
        import torch
        n = n_seg if n_seg_alloc is None else n_seg_alloc
        f64 = dict(dtype=torch.float64, device="cuda")
        self.B, self.S = B, n_seg
        self.dso = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
        self.dW = torch.zeros((n + B, 3), **f64)
        self.dT = torch.zeros(n, **f64)
        self.dED = torch.zeros((B, 18), **f64) if with_ed else None
        self.dC = torch.empty((n, 3, 8), **f64)
        self.dcost = torch.empty(B, **f64)
        self.dst = torch.empty(B, dtype=torch.int32, device="cuda")

    def write(self, so, W, T, ED, dso=None):
        assert len(so) - 1 == self.B and int(so[-1]) == self.S
        self.dso.copy_(_dev(np.asarray(so if dso is None else dso, dtype=np.int32)))
        self.dW[:len(W)].copy_(_dev(W))
        self.dT[:len(T)].copy_(_dev(T))
        if self.dED is not None:
            self.dED.copy_(_dev(ED))
        self.prefill()

    def prefill(self):
        self.dC.fill_(float("nan"))
        self.dcost.fill_(float("nan"))
        self.dst.fill_(-1)

    def call(self, solver, so, iters=ITERS, coeffs=True, cost=True, status=True, stream=0):
        solver.refine_loop_device(so, self.dso, self.dW, self.dT, K_T, ETA, iters, self.dC if coeffs else None,
                                  self.dcost if cost else None, self.dst if status else None, self.dED, stream)

    def results(self):
        import torch
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in (self.dT, self.dC, self.dcost, self.dst))


def run_fixed(solver, slots, so, W, T, ED, iters=ITERS):
    slots.write(so, W, T, ED)
    slots.call(solver, so, iters)
    return slots.results()


def run_fresh(so, W, T, ED, iters=ITERS, solver=None):
    """The same call with freshly allocated tensors: (T, C, cost, status) on the host.  Without
    a solver, on a handle of its own, closed afterwards: a new capture into plan buffers no
    earlier call wrote."""
    from trajectory_generator_ros2_amd.solver import Solver
    own = solver is None
    s = Solver(0) if own else solver
    try:
        slots = Slots(len(so) - 1, int(so[-1]), ED is not None)
        return run_fixed(s, slots, so, W, T, ED, iters)
    finally:
        if own:
            s.close()


def check_oracle(oracle, so, W, T, ED, got, iters=ITERS, ids=None):
    """got = (T, C, cost, status) of the whole batch against the oracle, on every trajectory
    or on the trajectories `ids`."""
    Tg, Cg, cg, stg = got
    if ids is not None:
        so, W, T, ED, seg = P.take(so, W, T, ED, ids)
        Tg, Cg, cg, stg = Tg[seg], Cg[seg], cg[ids], stg[ids]
    To, co, Co, sto = oracle.refine_batch(so, W, T, ED, K_T, ETA, iters, oracle.REDUCED)
    assert (sto == 0).all()
    assert (stg == 0).all(), np.unique(stg)
    eT, ec, eC = np.abs(Tg / To - 1).max(), np.abs(cg / co - 1).max(), batch_rel_err(so, Cg, Co)
    print("oracle: T %.2e cost %.2e C %.2e" % (eT, ec, eC))
    assert eT <= TOL
    assert ec <= TOL
    assert eC <= TOL
    if iters:
        assert not np.array_equal(Tg, np.asarray(T).reshape(-1))


def check_bit_equal(got, ref, what=""):
    for name, a, b in zip(("times", "coefficients", "costs"), got, ref):
        assert np.array_equal(_bits(a), _bits(b)), (what, name)
    assert np.array_equal(got[3], ref[3]), (what, "statuses")


# ------------------------------------------------------------------ 1. replay on new offsets

@pytest.mark.parametrize("with_ed", [False, True], ids=["rest", "end_derivs"])
def test_replay_on_new_offsets(solver, oracle, with_ed):
    """One key, one graph: A (every M), B (no M above the class boundary: the one-wave table
    goes back to no groups), C (two M, one per class, counts 32 k + 1 and 32 j - 1: 14 groups
    vanish, partial last tiles), A again in another order.  Each call against the oracle and
    bit-equal to a fresh handle's."""
    seq = P.replay_sequence(with_ed)
    slots = Slots(P.B_REPLAY, P.S_REPLAY, with_ed)
    for i, (name, so, W, T) in enumerate(seq):
        ED = P.end_derivs(P.B_REPLAY, 8150 + i) if with_ed else None
        got = run_fixed(solver, slots, so, W, T, ED)
        check_oracle(oracle, so, W, T, ED, got)
        check_bit_equal(got, run_fresh(so, W, T, ED), name)


@pytest.mark.parametrize("with_ed", [False, True], ids=["rest", "end_derivs"])
def test_ragged_uniform_ragged_on_the_same_tensors(solver, oracle, with_ed):
    """uniform_m is in the key: the middle call (every M = 8) runs the two-buffer uniform loop
    from a graph of its own, and the third call replays the first one's graph on other
    offsets after the uniform kernels ran on the same tensors."""
    slots = Slots(P.B_REPLAY, 8 * P.B_REPLAY, with_ed)
    for i, (name, so, W, T) in enumerate(P.switch_sequence()):
        ED = P.end_derivs(P.B_REPLAY, 8250 + i) if with_ed else None
        check_oracle(oracle, so, W, T, ED, run_fixed(solver, slots, so, W, T, ED))


# ------------------------------------------------------------------ 2. planner shape corners

@pytest.mark.parametrize("B", [1023, 1024, 1025])
def test_batch_around_the_planner_block(solver, oracle, B):
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = S.ragged_batch(B, 1, 16, seed=8500 + B)
    check_oracle(oracle, so, W, T, None, run_fresh(so, W, T, None, solver=solver))


@pytest.mark.parametrize("with_ed", [False, True], ids=["rest", "end_derivs"])
@pytest.mark.parametrize("count", [31, 32, 33])
@pytest.mark.parametrize("cls", [0, 1], ids=["two_wave", "one_wave"])
def test_tile_counts(solver, oracle, cls, count, with_ed):
    """31, 32 and 33 trajectories of one M (one tile, one full tile, a second tile of one
    lane), M at the class boundary on its side; one trajectory on the other side."""
    bd = P.BOUNDARY[with_ed]
    m, other = (bd, bd + 1) if cls == 0 else (bd + 1, bd)
    so, W, T = P.tile_count_batch(m, count, other, seed=8600 + count)
    ED = P.end_derivs(count + 1, 8650) if with_ed else None
    check_oracle(oracle, so, W, T, ED, run_fresh(so, W, T, ED, solver=solver))


@pytest.mark.parametrize("with_ed", [False, True], ids=["rest", "end_derivs"])
def test_empty_two_wave_class(solver, oracle, with_ed):
    rng = np.random.default_rng(8700)
    so, W, T = P.batch_from_ms(P.shuffled({15: 50, 16: 46}, rng), 8701)
    assert P.class_tiles(so, P.BOUNDARY[with_ed])[0] == 0
    ED = P.end_derivs(96, 8702) if with_ed else None
    check_oracle(oracle, so, W, T, ED, run_fresh(so, W, T, ED, solver=solver))


def _chunked(solver, so, W, T, chunk, iters):
    """The batch refined in calls of at most `chunk` trajectories, results put together."""
    from trajectory_generator_ros2_amd import shard as SH
    B = len(so) - 1
    parts = []
    for lo in range(0, B, chunk):
        so_l, W_l, T_l, _ = SH.shard_csr(so, W, T, None, lo, min(B, lo + chunk))
        parts.append(run_fresh(so_l, W_l, T_l, None, iters, solver=solver))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def test_more_than_64_planner_blocks(solver, oracle):
    """B = 65 x 1,024 + 7: 66 planner blocks, so the 64-lane sums over the block counts in
    k_plan_scatter take a second step, and the scatter bases of blocks 64 and 65 (which hold
    M = 16 trajectories, as block 0 does) depend on it.  Oracle on the first and the last
    1,024 trajectories and the 40 long ones; every trajectory bit-equal to calls on chunks of
    1,024, which plan with one block each."""
    so, W, T, long_ids = P.many_blocks_batch()
    B = len(so) - 1
    got = run_fresh(so, W, T, None, solver=solver)
    for ids in (np.arange(1024), np.arange(B - 1024, B), long_ids):
        check_oracle(oracle, so, W, T, None, got, ids=ids)
    check_bit_equal(got, _chunked(solver, so, W, T, 1024, ITERS))


@pytest.mark.parametrize("extra", [0, 1], ids=["tiles_eq_simds", "tiles_eq_simds_plus_1"])
def test_persistent_threshold(solver, oracle, extra):
    """plan->waves[1] turns non-zero exactly when the one-wave class has more tiles than the
    device has SIMDs.  With as many tiles as SIMDs the class runs one block per tile on a grid
    clamped to the SIMD count, so the last block is needed; one tile more is the smallest
    persistent case.  M in {15, 16}, partial last tiles, iters = 2."""
    import torch
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    so, W, T = P.persist_threshold_batch(simds + extra)
    Ms = np.diff(so)
    tiles1 = sum(-(-int((Ms == m).sum()) // 32) for m in range(P.BOUNDARY[False] + 1, 17))
    assert tiles1 == simds + extra, (tiles1, simds)
    B = len(so) - 1
    got = run_fresh(so, W, T, None, 2, solver=solver)
    for ids in (np.arange(256), np.arange(B - 256, B)):
        check_oracle(oracle, so, W, T, None, got, iters=2, ids=ids)
    check_bit_equal(got, _chunked(solver, so, W, T, 4096, 2))


# ------------------------------------------------------------------ 3. the graph cache

B_CACHE = 96
N_KEYS = 17  # one more than run_loop_graph keeps


@pytest.fixture(scope="module")
def cache_batch():
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = S.ragged_batch(B_CACHE, 1, 16, seed=8800)
    assert set(np.diff(so).tolist()) == set(range(1, 17))
    return so, W, T


@pytest.fixture(scope="module")
def cache_refs(cache_batch):
    """iters -> (T, C, cost, status) from a fresh handle, computed once."""
    so, W, T = cache_batch
    return {it: run_fresh(so, W, T, None, it) for it in range(N_KEYS)}


def test_iters_in_the_key_and_eviction(solver, oracle, cache_batch, cache_refs):
    """17 values of iters on fixed tensors are 17 keys through a cache of 16: the first is
    evicted, and iters = 0 and 1 capture again afterwards.  Every result bit-equal to the
    fresh handle's for that iters; iters = 0 returns the times to the bit."""
    so, W, T = cache_batch
    slots = Slots(B_CACHE, int(so[-1]), False)
    for it in list(range(N_KEYS)) + [0, 1]:
        got = run_fixed(solver, slots, so, W, T, None, it)
        check_bit_equal(got, cache_refs[it], it)
        if it == 0:
            assert np.array_equal(_bits(got[0]), _bits(T))
        if it in (0, 3):
            check_oracle(oracle, so, W, T, None, got, iters=it)


@pytest.mark.parametrize("drop", [("coeffs",), ("cost",), ("status",), ("coeffs", "cost", "status")],
                         ids=["no_coeffs", "no_cost", "no_status", "times_only"])
def test_nullable_outputs_in_the_key(solver, cache_batch, cache_refs, drop):
    """The output pointers are part of the key: a call without some of them is another graph,
    writes only the others (bit-equal to the full call's), leaves the absent ones' tensors
    alone, and the times always match.

    no_coeffs found that the cost depended on whether coefficients were asked for (87 of 96
    costs differed, max |c / c_full - 1| = 8.4e-15): refine_loop_block (csrc/tgms_reduced.hip)
    took it from the final solve's P4..P7 (seg_cost_q) with coefficients and from a gradient
    pass in the Legendre form (seg_grad_u) without.  Both paths now run the same last pass,
    which stores nothing when there is nowhere to store."""
    so, W, T = cache_batch
    slots = Slots(B_CACHE, int(so[-1]), False)
    ref = cache_refs[ITERS]
    check_bit_equal(run_fixed(solver, slots, so, W, T, None), ref, "full")  # the full call's graph first
    slots.write(so, W, T, None)
    slots.call(solver, so, **{k: False for k in drop})
    Tg, Cg, cg, stg = slots.results()
    assert np.array_equal(_bits(Tg), _bits(ref[0]))
    assert np.isnan(Cg).all() if "coeffs" in drop else np.array_equal(_bits(Cg), _bits(ref[1]))
    assert (stg == -1).all() if "status" in drop else np.array_equal(stg, ref[3])
    if "cost" in drop:
        assert np.isnan(cg).all()
    else:
        print("cost against the full call's: max |c / c_full - 1| = %.3e, %d of %d differ"
              % (np.abs(cg / ref[2] - 1).max(), int((_bits(cg) != _bits(ref[2])).sum()), len(cg)))
        assert np.array_equal(_bits(cg), _bits(ref[2]))


def test_eviction_with_replays_in_flight(solver, cache_batch, cache_refs):
    """The 17 calls back to back on a side stream, nothing synchronised in between: the 17th
    capture evicts the first graph, which must have finished before it is destroyed.  The
    times chain from call to call (the loop works in place); every call has outputs of its
    own.  All of it equals the same chain run with a synchronisation after every call."""
    import torch
    so, W, T = cache_batch
    n_seg = int(so[-1])
    dso, dW = _dev(so), _dev(W)

    def outputs():
        return [(torch.full((n_seg, 3, 8), float("nan"), dtype=torch.float64, device="cuda"),
                 torch.full((B_CACHE,), float("nan"), dtype=torch.float64, device="cuda"),
                 torch.full((B_CACHE,), -1, dtype=torch.int32, device="cuda"),
                 torch.full((n_seg,), float("nan"), dtype=torch.float64, device="cuda")) for _ in range(N_KEYS)]

    def chain(stream, sync):
        dT, outs = _dev(T.copy()), outputs()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for it, (dC, dcost, dst, snap) in enumerate(outs):
                solver.refine_loop_device(so, dso, dW, dT, K_T, ETA, it, dC, dcost, dst, None, stream.cuda_stream)
                snap.copy_(dT)  # on the same stream: the times after call `it`
                if sync:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [tuple(x.cpu().numpy() for x in (snap, dC, dcost, dst)) for dC, dcost, dst, snap in outs]

    side = torch.cuda.Stream()
    ref = chain(side, True)
    got = chain(side, False)
    assert all((r[3] == 0).all() for r in ref)
    assert not np.array_equal(ref[-1][0], ref[1][0])
    for it in (0, 1):  # iters = 0 keeps the times, so the first two calls start from T
        check_bit_equal(ref[it], cache_refs[it], ("chain", it))
    for it in range(N_KEYS):
        check_bit_equal(got[it], ref[it], it)


# ------------------------------------------------------------------ 4. device offsets that disagree

@pytest.mark.parametrize("kind", ["span", "swap"])
def test_device_offsets_that_disagree_with_the_hosts(solver, oracle, kind):
    """include/tgms.h asks for the same values in both copies; k_plan_scatter guards the case
    they differ.  Valid host offsets, and a device copy with (span) one M raised by 1 and so
    another span, or (swap) the same span with one M = 0 and one M = 17: the call returns OK,
    nothing runs, a trajectory whose own M is outside 1..16 reads ERR_INVALID_ARG and every
    other one ERR_SKIPPED, coefficients and costs are exact zeros and the times are kept.  The
    same call with the right device offsets afterwards, on the same tensors (the same graph),
    matches the oracle: plan->bad clears."""
    from trajectory_generator_ros2_amd import ERR_INVALID_ARG, ERR_SKIPPED
    from trajectory_generator_ros2_amd import synthetic as S
    so, W, T = S.ragged_batch(300, 1, 16, seed=8900)
    n_seg = int(so[-1])
    dso_bad, Ms_dev = P.bad_device_offsets(so, kind)
    span = max(n_seg, int(dso_bad[-1]))  # no index the device offsets name leaves a buffer
    slots = Slots(300, n_seg, False, n_seg_alloc=span)
    slots.dT.fill_(0.7)
    slots.write(so, W, T, None, dso=dso_bad)
    T_in = slots.dT.cpu().numpy().copy()
    slots.call(solver, so)  # returns OK (an error would raise)
    Tg, Cg, cg, stg = slots.results()
    outside = (Ms_dev < 1) | (Ms_dev > 16)
    assert outside.sum() == (0 if kind == "span" else 2)
    assert np.array_equal(stg, np.where(outside, ERR_INVALID_ARG, ERR_SKIPPED))
    assert not Cg[:n_seg].any() and not np.isnan(Cg[:n_seg]).any()
    assert np.isnan(Cg[n_seg:]).all()  # beyond the host's S nothing is written
    assert not cg.any() and not np.isnan(cg).any()
    assert np.array_equal(_bits(Tg), _bits(T_in))
    slots.write(so, W, T, None)
    slots.call(solver, so)
    Tg, Cg, cg, stg = slots.results()
    check_oracle(oracle, so, W, T, None, (Tg[:n_seg], Cg[:n_seg], cg, stg))
