"""Reference reductions for the feasibility check (tgms_extrema_batch*), shared by
test_extrema_host.py and test_gpu_extrema.py.  A record is pmin[3] pmax[3] v_peak a_peak
j_peak duration over the sampler's samples of one trajectory."""
import numpy as np

PEAK_RTOL = 1e-14   # the components are the sampler's bits; the 3-term sum and the sqrt round differently
ORACLE_TOL = 1e-9   # the project's bound against the oracle


def reduce_samples(offs, out):
    """[B,9] pmin pmax and sqrt(max |v|^2, |a|^2, |j|^2) over sampler output out [n, >=12]."""
    B = len(offs) - 1
    ref = np.empty((B, 9))
    for b in range(B):
        s = out[offs[b]:offs[b + 1]]
        ref[b, 0:3] = s[:, 0:3].min(axis=0)
        ref[b, 3:6] = s[:, 0:3].max(axis=0)
        for q in range(3):
            d = s[:, 3 + 3 * q:6 + 3 * q]
            ref[b, 6 + q] = np.sqrt((d * d).sum(axis=1).max())
    return ref


def durations(so, T):
    """The sampler's prefix sum of T (left to right), per trajectory."""
    dur = np.empty(len(so) - 1)
    for b in range(len(so) - 1):
        acc = 0.0
        for t in np.asarray(T, dtype=np.float64).reshape(-1)[so[b]:so[b + 1]]:
            acc += float(t)
        dur[b] = acc
    return dur


def bit_equal(a, b):
    """a and b hold the same bits everywhere, except where both are zeros: the minimum of a
    set that holds +0.0 and -0.0 has no defined sign (numpy's and torch's own reductions
    return either), so there, and only there, the sign bit may differ."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | ((a == 0.0) & (b == 0.0))).all())


def check_against_samples(ext, so, T, offs, out):
    """(1) extents bit-equal to min / max over the samples (bit_equal above), (2) peaks within
    1e-14 relative of sqrt(max(sum of squares)), (3) duration bit-equal to the prefix sum."""
    ext = np.asarray(ext)
    assert ext.shape == (len(so) - 1, 10) and np.isfinite(ext).all()
    ref = reduce_samples(offs, out)
    assert bit_equal(ext[:, 0:6], ref[:, 0:6])
    assert (np.abs(ext[:, 6:9] - ref[:, 6:9]) <= PEAK_RTOL * ref[:, 6:9]).all(), \
        float((np.abs(ext[:, 6:9] - ref[:, 6:9]) / np.maximum(ref[:, 6:9], 1e-300)).max())
    assert np.array_equal(ext[:, 9].view(np.int64), durations(so, T).view(np.int64))


def check_against_oracle(ext, so, W, T, ED, C, dt, oracle):
    """(4) extents within 1e-9 x max|p| and peaks within 1e-9 relative of the reduction over
    oracle.sample, per trajectory."""
    W, T = np.asarray(W).reshape(-1, 3), np.asarray(T).reshape(-1)
    C = np.asarray(C).reshape(-1, 3, 8)
    for b in range(len(so) - 1):
        s0, s1 = int(so[b]), int(so[b + 1])
        ed = None if ED is None else np.ascontiguousarray(np.asarray(ED).reshape(-1, 18)[b])
        smp = oracle.sample(C[s0:s1], T[s0:s1], W[s0 + b:s1 + b + 1], ed, dt)
        ref = reduce_samples(np.array([0, smp.shape[0]]), smp)[0]
        assert np.abs(ext[b, 0:6] - ref[0:6]).max() <= ORACLE_TOL * np.abs(smp[:, 0:3]).max(), b
        assert (np.abs(ext[b, 6:9] - ref[6:9]) <= ORACLE_TOL * ref[6:9]).all(), b
