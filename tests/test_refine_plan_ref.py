"""CPU: the batch builders of tests/refine_plan_ref.py put every batch on the planner path that
test_gpu_refine_plan.py means to run: one B and one S along the replay sequence with the class
occupancies A, B, C, A again; the tile counts, block counts and the persistent threshold of the
shape corners; device offsets that disagree with the host's in the two ways asked for."""
import numpy as np
import pytest

import refine_plan_ref as P
from trajectory_generator_ros2_amd import synthetic as S


def _ms(so):
    return np.diff(np.asarray(so, dtype=np.int64))


def test_batch_from_ms_is_the_synthetic_batch():
    """Given ragged_batch's own M, the builder returns ragged_batch's batch (same stream of
    draws after M), so the waypoints and times are in its ranges."""
    so, W, T = S.ragged_batch(50, 1, 16, seed=3)
    rng = np.random.default_rng(3)
    rng.integers(1, 17, size=50)  # ragged_batch's draw of M comes first
    so2, W2, T2 = P.batch_from_ms(_ms(so), rng)
    assert np.array_equal(so, so2) and np.array_equal(W, W2) and np.array_equal(T, T2)
    assert T.min() >= S.T_MIN and T.max() <= S.T_MAX


@pytest.mark.parametrize("with_ed", [False, True])
def test_replay_sequence_invariants(with_ed):
    seq = P.replay_sequence(with_ed)
    P.check_replay_sequence(seq, with_ed)
    bd = 11 if with_ed else 13
    assert P.BOUNDARY[with_ed] == bd and P.B_REPLAY == 2 * 1024 + 32 and P.S_REPLAY == 16790
    Bs = {len(so) - 1 for _, so, _, _ in seq}
    Ss = {int(so[-1]) for _, so, _, _ in seq}
    assert Bs == {2080} and Ss == {16790}
    mA, mB, mC, mA2 = (_ms(so) for _, so, _, _ in seq)
    assert set(mA.tolist()) == set(range(1, 17))
    assert mB.max() <= bd and (mA > bd).any()          # the one-wave table goes from filled to empty
    nlo, nhi = int((mC == P.C_LO).sum()), int((mC == P.C_HI).sum())
    assert nlo + nhi == 2080 and nlo % 32 == 1 and nhi % 32 == 31 and P.C_LO <= bd < P.C_HI
    assert sorted(mA.tolist()) == sorted(mA2.tolist()) and not np.array_equal(mA, mA2)
    for _, so, W, T in seq:  # times belong to the waypoints
        rows = np.arange(int(so[-1])) + np.repeat(np.arange(len(so) - 1), _ms(so))
        d = np.linalg.norm(W[rows + 1] - W[rows], axis=1)
        assert np.array_equal(T, np.clip(d, S.T_MIN, S.T_MAX))


def test_replay_sequence_cannot_have_s_equal_8b():
    """Why S is not 8 B: two M with counts 32 k + 1 and 32 j - 1 give S = m_lo - m_hi mod 32."""
    for m_lo in range(1, 17):
        for m_hi in range(m_lo + 1, 17):
            for k in range(0, 66):
                for n_lo, n_hi in ((32 * k + 1, 2080 - 32 * k - 1), (32 * k - 1, 2080 - 32 * k + 1)):
                    if n_lo > 0 and n_hi > 0:
                        assert (m_lo * n_lo + m_hi * n_hi) % 32 != 0
    assert (8 * 2080) % 32 == 0


def test_a2_is_a_reordered():
    seq = P.replay_sequence(False)
    (_, soA, WA, TA), (_, so2, W2, T2) = seq[0], seq[3]
    keyA = sorted((tuple(TA[soA[b]:soA[b + 1]])) for b in range(2080))
    key2 = sorted((tuple(T2[so2[b]:so2[b + 1]])) for b in range(2080))
    assert keyA == key2


def test_take_slices_whole_trajectories():
    so, W, T = S.ragged_batch(40, 1, 16, seed=5)
    ED = P.end_derivs(40, 6)
    ids = np.array([39, 0, 17, 17, 3])
    so_l, W_l, T_l, ED_l, seg = P.take(so, W, T, ED, ids)
    assert np.array_equal(_ms(so_l), _ms(so)[ids]) and np.array_equal(ED_l, ED[ids])
    for q, b in enumerate(ids):
        assert np.array_equal(T_l[so_l[q]:so_l[q + 1]], T[so[b]:so[b + 1]])
        assert np.array_equal(seg[so_l[q]:so_l[q + 1]], np.arange(so[b], so[b + 1]))
        assert np.array_equal(W_l[so_l[q] + q:so_l[q + 1] + q + 1], W[so[b] + b:so[b + 1] + b + 1])


def test_switch_sequence():
    seq = P.switch_sequence()
    assert [n for n, *_ in seq] == ["ragged", "uniform", "ragged2"]
    assert all(len(so) - 1 == 2080 and int(so[-1]) == 8 * 2080 for _, so, _, _ in seq)
    assert (_ms(seq[1][1]) == 8).all()
    assert not P.is_uniform(seq[0][1]) and not P.is_uniform(seq[2][1])
    assert not np.array_equal(seq[0][1], seq[2][1])


@pytest.mark.parametrize("with_ed", [False, True])
@pytest.mark.parametrize("count", [31, 32, 33])
@pytest.mark.parametrize("cls", [0, 1])
def test_tile_count_batches(cls, count, with_ed):
    bd = P.BOUNDARY[with_ed]
    m, other = (bd, bd + 1) if cls == 0 else (bd + 1, bd)
    so, _, _ = P.tile_count_batch(m, count, other, seed=1)
    tiles = P.class_tiles(so, bd)
    assert tiles[cls] == -(-count // 32) and tiles[1 - cls] == 1
    assert len(so) - 1 == count + 1 and not P.is_uniform(so)


def test_many_blocks_batch():
    so, W, T, long_ids = P.many_blocks_batch()
    B = len(so) - 1
    assert B == 65 * 1024 + 7 and -(-B // 1024) > 64
    Ms = _ms(so)
    assert (Ms[long_ids] == 16).all() and (Ms == 16).sum() == 40
    assert set((long_ids // 1024).tolist()) == {0, 64, 65}
    assert (Ms[64 * 1024:] == 16).sum() >= 2 and (Ms[65 * 1024:] == 16).any()  # a late block's base counts
    for bd in (11, 13):
        t2, t1 = P.class_tiles(so, bd)
        assert t1 == 2 and t2 > 64


@pytest.mark.parametrize("simds", [1024, 1216, 6])
def test_persist_threshold_batches(simds):
    for tiles in (simds, simds + 1):
        so, _, _ = P.persist_threshold_batch(tiles)
        Ms = _ms(so)
        assert set(Ms.tolist()) == {15, 16}
        n15, n16 = int((Ms == 15).sum()), int((Ms == 16).sum())
        assert -(-n15 // 32) + -(-n16 // 32) == tiles and n15 % 32 and n16 % 32
        assert P.class_tiles(so, 13) == (0, tiles) and P.class_tiles(so, 11) == (0, tiles)


@pytest.mark.parametrize("kind", ["span", "swap"])
def test_bad_device_offsets(kind):
    so, _, _ = S.ragged_batch(300, 1, 16, seed=31)
    dso, Ms = P.bad_device_offsets(so, kind)
    assert dso.dtype == np.int32 and dso[0] == 0 and len(dso) == 301
    assert np.array_equal(np.diff(dso), Ms)
    changed = np.flatnonzero(Ms != _ms(so))
    if kind == "span":
        assert int(dso[-1]) == int(so[-1]) + 1 and len(changed) == 1
        assert 1 <= Ms.min() and Ms.max() <= 16  # every M valid: only the span gives it away
    else:
        assert int(dso[-1]) == int(so[-1]) and len(changed) == 2
        assert sorted(Ms[changed].tolist()) == [0, 17]
        assert ((Ms < 1) | (Ms > 16)).sum() == 2
