"""Batch builders for the ragged refinement loop's device plan (tgms_refine_loop_device on a
ragged batch: k_perm_hist, k_plan_scatter, k_refine_loop_dev per occupancy class, all in one
cached graph), shared by test_refine_plan_ref.py and test_gpu_refine_plan.py.  NumPy only.

Every builder picks the segment counts M first, so that the batch lands on the planner path
it is meant for, and then draws waypoints and times exactly as synthetic.ragged_batch does
(the room's bounds, T = clip(distance / v, 0.5, 10)).  The occupancy classes: M up to the
boundary runs at two waves per SIMD (class 0), larger M at one (class 1); the boundary is
TGMS_TWO_WAVE_MAX_M = 13 without end derivatives and TGMS_TWO_WAVE_MAX_M_ED = 11 with them.
A class's tile count is the sum over its M of ceil(count(M) / 32), as k_plan_scatter has it.

The replay sequence shares one B and one S, because the loop's graph is cached by sizes,
pointers and scalars: B = 2,080 (two planner blocks of 1,024 and a third of one half-wave)
and S = 16,790.  S = 8 B is not possible: batch C has two values of M with counts 32 k + 1
and 32 j - 1, so S = 32 (k m_lo + j m_hi) + (m_lo - m_hi) and S mod 32 = m_lo - m_hi, which
is never 0 for two different M in 1..16.  With m_lo = 5, m_hi = 15 the nearest S to 8 B is
5 x 1,441 + 15 x 639 = 16,790 (mean M 8.07)."""
import numpy as np

from trajectory_generator_ros2_amd import synthetic as S

TPW = 32                           # trajectories per wavefront tile (RAGGED_TPW)
PERM_BLOCK = 1024                  # trajectories per planner block
BOUNDARY = {False: 13, True: 11}   # TGMS_TWO_WAVE_MAX_M, TGMS_TWO_WAVE_MAX_M_ED (by with_ed)
M_MAX = 16

B_REPLAY = 2080
C_LO, C_HI = 5, 15                 # batch C's two M: one in each class at either boundary
C_N_LO, C_N_HI = 1441, 639         # 32 x 45 + 1 and 32 x 20 - 1
S_REPLAY = C_LO * C_N_LO + C_HI * C_N_HI

B_BLOCKS = 65 * PERM_BLOCK + 7     # 66 planner blocks: the sums over hist wrap their 64 lanes


def offsets_of(Ms):
    so = np.zeros(len(Ms) + 1, dtype=np.int64)
    np.cumsum(np.asarray(Ms, dtype=np.int64), out=so[1:])
    return so.astype(np.int32)


def batch_from_ms(Ms, seed):
    """CSR batch (seg_offsets int32 [B+1], waypoints [S+B,3], times [S]) with the given segment
    counts: synthetic.ragged_batch after its draw of M (seed: an integer or a Generator)."""
    rng = np.random.default_rng(seed)
    Ms = np.asarray(Ms, dtype=np.int64)
    B = len(Ms)
    so = offsets_of(Ms).astype(np.int64)
    n_s = int(so[-1])
    n_w = n_s + B
    W = np.empty((n_w, 3), dtype=np.float64)
    W[:, 0] = rng.uniform(-5.0, 5.0, size=n_w)
    W[:, 1] = rng.uniform(-5.0, 5.0, size=n_w)
    W[:, 2] = rng.uniform(0.5, 5.0, size=n_w)
    rows = np.arange(n_s) + np.repeat(np.arange(B), Ms)
    T = np.clip(np.linalg.norm(W[rows + 1] - W[rows], axis=1) / S.V_NOMINAL, S.T_MIN, S.T_MAX)
    return so.astype(np.int32), W, T


def end_derivs(B, seed):
    return np.random.default_rng(seed).normal(0.0, 0.5, size=(B, 18))


def take(so, W, T, ED, ids):
    """The trajectories `ids` (any order) as a CSR batch of their own, and the segment indices
    they came from: (so_l, W_l, T_l, ED_l, seg)."""
    so = np.asarray(so, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    Ms = so[ids + 1] - so[ids]
    so_l = offsets_of(Ms).astype(np.int64)
    seg = np.arange(so_l[-1]) - np.repeat(so_l[:-1], Ms) + np.repeat(so[ids], Ms)
    wo_l = so_l + np.arange(len(ids) + 1)
    wrow = np.arange(wo_l[-1]) - np.repeat(wo_l[:-1], Ms + 1) + np.repeat(so[ids] + ids, Ms + 1)
    ED_l = None if ED is None else np.asarray(ED).reshape(-1, 18)[ids]
    return so_l.astype(np.int32), np.asarray(W).reshape(-1, 3)[wrow], np.asarray(T).reshape(-1)[seg], ED_l, seg


def counts_of(so):
    """count[m] for m = 0..16 (M outside that range is an error of the caller)."""
    return np.bincount(np.diff(np.asarray(so, dtype=np.int64)), minlength=M_MAX + 1)


def class_tiles(so, boundary):
    """(two-wave tiles, one-wave tiles): per class the sum over its M of ceil(count / 32)."""
    c = counts_of(so)
    t = -(-c // TPW)
    return int(t[1:boundary + 1].sum()), int(t[boundary + 1:].sum())


def is_uniform(so):
    return len(np.unique(np.diff(np.asarray(so, dtype=np.int64)))) == 1


def draw_ms(B, n_seg, m_lo, m_hi, rng):
    """B values of M, i.i.d. uniform in m_lo..m_hi and then moved by single steps, at random
    places, until they sum to n_seg."""
    assert B * m_lo <= n_seg <= B * m_hi
    Ms = rng.integers(m_lo, m_hi + 1, size=B).astype(np.int64)
    diff = int(n_seg - Ms.sum())
    while diff:
        room = np.flatnonzero(Ms < m_hi if diff > 0 else Ms > m_lo)
        idx = rng.permutation(room)[:abs(diff)]
        Ms[idx] += 1 if diff > 0 else -1
        diff = int(n_seg - Ms.sum())
    return Ms


def shuffled(counts, rng):
    """M values with the given {M: count}, in random order."""
    Ms = np.concatenate([np.full(n, m, dtype=np.int64) for m, n in counts.items()])
    return rng.permutation(Ms)


def check_replay_sequence(seq, with_ed):
    """The conditions the replay test rests on: one B and one S, no uniform batch (that would be
    another key and another path), and the class occupancies of A, B, C, A'."""
    bd = BOUNDARY[with_ed]
    assert [name for name, *_ in seq] == ["A", "B", "C", "A2"]
    for name, so, W, T in seq:
        assert so.dtype == np.int32 and so[0] == 0
        assert len(so) - 1 == B_REPLAY and int(so[-1]) == S_REPLAY, name
        assert W.shape == (S_REPLAY + B_REPLAY, 3) and T.shape == (S_REPLAY,), name
        assert not is_uniform(so), name
        Ms = np.diff(so)
        assert Ms.min() >= 1 and Ms.max() <= M_MAX, name
    cA, cB, cC, cA2 = (counts_of(so) for _, so, _, _ in seq)
    assert (cA[1:] > 0).all()                                   # A: every M in 1..16
    assert cB[bd + 1:].sum() == 0 and cB[1:bd + 1].sum() == B_REPLAY  # B: the one-wave class is empty
    assert class_tiles(seq[1][1], bd)[1] == 0 and class_tiles(seq[0][1], bd)[1] > 0
    assert np.flatnonzero(cC).tolist() == [C_LO, C_HI] and C_LO <= bd < C_HI  # C: one M per class
    assert cC[C_LO] % TPW == 1 and cC[C_HI] % TPW == TPW - 1    # partial last tiles on both sides
    assert (cA > 0).sum() - (cC > 0).sum() == 14                 # 14 groups vanish
    assert np.array_equal(cA, cA2)                               # A again: the same groups ...
    assert not np.array_equal(seq[0][1], seq[3][1])              # ... in another order


def replay_sequence(with_ed, seed=8100):
    """[(name, so, W, T)] for A, B, C, A2 (see the module docstring and the issue's section 1):
    A every M in 1..16; B only M up to the class boundary; C the two values C_LO and C_HI with
    counts 32 k + 1 and 32 j - 1; A2 is A with its trajectories in another order."""
    rng = np.random.default_rng(seed + int(with_ed))
    bd = BOUNDARY[with_ed]
    ms_a = draw_ms(B_REPLAY, S_REPLAY, 1, M_MAX, rng)
    ms_b = draw_ms(B_REPLAY, S_REPLAY, 1, bd, rng)
    ms_c = shuffled({C_LO: C_N_LO, C_HI: C_N_HI}, rng)
    seq = [(n, *batch_from_ms(ms, seed + 10 + i)) for i, (n, ms) in enumerate((("A", ms_a), ("B", ms_b), ("C", ms_c)))]
    _, so, W, T = seq[0]
    seq.append(("A2", *take(so, W, T, None, rng.permutation(B_REPLAY))[:3]))
    check_replay_sequence(seq, with_ed)
    return seq


def switch_sequence(seed=8200):
    """Ragged, uniform (every M = 8), ragged: one B = 2,080 and one S = 8 B."""
    rng = np.random.default_rng(seed)
    B, n_seg = B_REPLAY, 8 * B_REPLAY
    seq = [("ragged", *batch_from_ms(draw_ms(B, n_seg, 1, M_MAX, rng), seed + 1)),
           ("uniform", *batch_from_ms(np.full(B, 8), seed + 2)),
           ("ragged2", *batch_from_ms(draw_ms(B, n_seg, 1, M_MAX, rng), seed + 3))]
    for name, so, W, T in seq:
        assert len(so) - 1 == B and int(so[-1]) == n_seg, name
        assert is_uniform(so) == (name == "uniform"), name
    return seq


def tile_count_batch(m, count, m_other, seed):
    """`count` trajectories of M = m and one of M = m_other, shuffled: ceil(count / 32) tiles
    of m, and the single other trajectory keeps the batch ragged."""
    assert m != m_other
    rng = np.random.default_rng(seed)
    return batch_from_ms(shuffled({m: count, m_other: 1}, rng), seed + 1)


def many_blocks_batch(seed=8300):
    """B = 65 x 1,024 + 7 (66 planner blocks, so k_plan_scatter's 64-lane sums over the block
    counts take a second step): M in {1, 2}, and 40 trajectories of M = 16 in the first, the
    65th and the last block.  Returns (so, W, T, ids of the long ones)."""
    rng = np.random.default_rng(seed)
    Ms = rng.integers(1, 3, size=B_BLOCKS).astype(np.int64)
    last = B_BLOCKS - 64 * PERM_BLOCK - PERM_BLOCK  # trajectories in the last block
    long_ids = np.sort(np.concatenate([rng.choice(PERM_BLOCK, 17, replace=False),
                                       64 * PERM_BLOCK + rng.choice(PERM_BLOCK, 17, replace=False),
                                       65 * PERM_BLOCK + rng.choice(last, 6, replace=False)]))
    Ms[long_ids] = M_MAX
    so, W, T = batch_from_ms(Ms, seed + 1)
    blocks = long_ids // PERM_BLOCK
    assert -(-B_BLOCKS // PERM_BLOCK) == 66 and len(long_ids) == 40
    assert sorted(set(blocks.tolist())) == [0, 64, 65]
    assert set(np.unique(np.diff(so)).tolist()) == {1, 2, M_MAX}
    return so, W, T, long_ids


def persist_threshold_batch(tiles, seed=8400):
    """M in {15, 16}, shuffled, with exactly `tiles` one-wave tiles (tiles >= 2), both groups'
    last tiles partial.  At tiles = SIMDs the class runs one block per tile on a grid of
    exactly that many blocks; one more tile is the smallest persistent case."""
    t15 = tiles // 2
    t16 = tiles - t15
    rng = np.random.default_rng(seed + tiles)
    so, W, T = batch_from_ms(shuffled({15: TPW * t15 - 5, 16: TPW * t16 - 9}, rng), seed + 1)
    assert class_tiles(so, BOUNDARY[False]) == (0, tiles)
    return so, W, T


def bad_device_offsets(so, kind):
    """A device copy of valid offsets that disagrees with them.  "span": one M raised by 1,
    every later offset shifted (another span).  "swap": the same span with one M = 0 and
    one M = 17 (two trajectories whose M add up to 17).  Returns (offsets int32, M per
    trajectory as the device copy has them)."""
    Ms = np.diff(np.asarray(so, dtype=np.int64))
    if kind == "span":
        k = int(np.flatnonzero(Ms < M_MAX)[len(Ms) // 3])
        Ms[k] += 1
    else:
        i = int(np.flatnonzero(Ms <= 8)[5])
        j = int(np.flatnonzero(Ms == 17 - Ms[i])[-1])
        assert i != j
        Ms[i], Ms[j] = 0, 17
    dso = offsets_of(Ms)
    assert (kind == "span") == (int(dso[-1]) != int(so[-1]))
    return dso, Ms
