"""Python front-end over the C ABI (numpy host buffers or torch device tensors).

Mirrors the reference's generate-then-consume flow: a batch of
waypoint sets goes in, order-7 coefficients [seg][axis][8] come out, and the
sampler turns them into Goal-like records at dt.  All compute runs in libtgms
(HIP); this module only marshals pointers.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import TgmsError


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags.c_contiguous, "arrays must be C-contiguous"
        return a.ctypes.data
    # torch tensor (device or host)
    assert a.is_contiguous(), "tensors must be contiguous"
    return a.data_ptr()


def _csr(seg_offsets, waypoints=None, seg_times=None, coeffs=None, end_derivs=None):
    """The CSR inputs as the C ABI takes them, None staying None: (seg_offsets int32, waypoints
    [-1,3], seg_times [-1], coeffs (shape kept), end_derivs [-1,18]), the last four float64."""
    def f64(a, *shape):
        a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        return a if a is None or not shape else a.reshape(*shape)
    return (np.ascontiguousarray(seg_offsets, dtype=np.int32), f64(waypoints, -1, 3), f64(seg_times, -1), f64(coeffs),
            f64(end_derivs, -1, 18))


class Solver:
    """A libtgms handle bound to one HIP device (or, asked for explicitly, the host backend)."""

    def __init__(self, device: int = 0, method: int = _lib.METHOD_REDUCED, device_count: int = 0,
                 host: bool = False):
        """device_count > 0: a multi-GPU handle over devices 0..device_count-1
        (tgms_create_multi: one RCCL communicator per device); host=True: the explicit host
        backend (tgms_create_host: solve + sample on the CPU, config 1); else one device."""
        self._L = _lib.load()
        h = ctypes.c_void_p()
        if host:
            st = self._L.tgms_create_host(ctypes.byref(h))
            what = "tgms_create_host"
        elif device_count > 0:
            st = self._L.tgms_create_multi(ctypes.byref(h), int(device_count))
            what = "tgms_create_multi"
        else:
            st = self._L.tgms_create(ctypes.byref(h), int(device))
            what = "tgms_create"
        if st != _lib.OK:
            raise TgmsError(st, f"{what} failed (no CPU fallback exists)")
        self._h = h
        self.device = 0 if device_count > 0 else device
        self.device_count = int(self._L.tgms_device_count(h))
        self.set_method(method)

    def close(self):
        if getattr(self, "_h", None):
            self._L.tgms_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def last_error(self) -> str:
        return self._L.tgms_last_error(self._h).decode()

    def _check(self, st: int) -> None:
        if st != _lib.OK:
            raise TgmsError(st, self.last_error())

    def set_method(self, method: int):
        self._check(self._L.tgms_set_method(self._h, int(method)))
        self.method = method

    # ---------------------------------------------------------------- host API
    def solve(self, seg_offsets, waypoints, seg_times, end_derivs=None, check: bool = True,
              out: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> Tuple[np.ndarray, np.ndarray, int]:
        """CSR host batch -> (coeffs [S,3,8], status [B], worst status).

        `out` = (coeffs, status) reuses caller buffers (float64 [S,3,8], int32 [>=B]):
        fresh host pages fault in during the device-to-host copy, reused ones do not."""
        so, W, T, _, ED = _csr(seg_offsets, waypoints, seg_times, end_derivs=end_derivs)
        B = so.shape[0] - 1
        S = int(so[-1]) if B > 0 else 0
        if out is not None:
            C, st = out
            if C.dtype != np.float64 or C.size < S * 24 or not C.flags.c_contiguous:
                raise ValueError("out coeffs must be C-contiguous float64 with >= S*24 elements")
            if st.dtype != np.int32 or st.size < max(B, 1) or not st.flags.c_contiguous:
                raise ValueError("out status must be C-contiguous int32 with >= B elements")
        else:
            C = np.zeros((S, 3, 8), dtype=np.float64)
            st = np.zeros(max(B, 1), dtype=np.int32)
        worst = self._L.tgms_solve_batch(self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(ED), _ptr(C), _ptr(st))
        if check and worst not in (_lib.OK,) and worst in (_lib.ERR_DEVICE, _lib.ERR_NO_DEVICE):
            raise TgmsError(worst, self.last_error())
        return C, st[:B], worst

    def solve_multi(self, seg_offsets, waypoints, seg_times, end_derivs=None) -> Tuple[np.ndarray, np.ndarray, int]:
        """tgms_solve_batch_multi: host batch over every device of the handle."""
        so, W, T, _, ED = _csr(seg_offsets, waypoints, seg_times, end_derivs=end_derivs)
        B = so.shape[0] - 1
        C = np.zeros((int(so[-1]) if B > 0 else 0, 3, 8), dtype=np.float64)
        st = np.zeros(max(B, 1), dtype=np.int32)
        worst = self._L.tgms_solve_batch_multi(self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(ED), _ptr(C), _ptr(st))
        if worst in (_lib.ERR_DEVICE, _lib.ERR_NO_DEVICE):
            raise TgmsError(worst, self.last_error())
        return C, st[:B], worst

    def sample(self, seg_offsets, waypoints, seg_times, end_derivs, coeffs, dt: float,
               yaw_mode: int = _lib.YAW_CONSTANT, yaw_const: float = 0.0):
        so, W, T, C, ED = _csr(seg_offsets, waypoints, seg_times, coeffs, end_derivs)
        B = so.shape[0] - 1
        offs = sample_offsets(so, T, dt)
        out = np.zeros((int(offs[-1]), _lib.GOAL_STRIDE), dtype=np.float64)
        self._check(self._L.tgms_sample_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(ED), _ptr(C), float(dt), int(yaw_mode), float(yaw_const),
            _ptr(offs), _ptr(out)))
        return offs, out

    def extrema(self, seg_offsets, waypoints, seg_times, end_derivs, coeffs, dt: float,
                limits: Optional[_lib.Limits] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Feasibility check at dt (include/tgms.h tgms_extrema_batch): (extrema [B,10] =
        pmin pmax v_peak a_peak j_peak duration, flags [B] of FEAS_* bits against `limits`;
        None checks nothing, so only FEAS_NONFINITE can appear)."""
        so, W, T, C, ED = _csr(seg_offsets, waypoints, seg_times, coeffs, end_derivs)
        B = so.shape[0] - 1
        ext = np.zeros((B, _lib.EXTREMA_STRIDE), dtype=np.float64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_extrema_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(ED), _ptr(C), float(dt),
            None if limits is None else ctypes.byref(limits), _ptr(ext), _ptr(flags)))
        return ext, flags

    def bounds(self, seg_offsets, seg_times, coeffs,
               limits: Optional[_lib.Limits] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Continuous feasibility bounds (include/tgms.h tgms_bounds_batch): the record and
        flags of extrema(), from the polynomials' stationary points on every segment's closed
        interval instead of samples at a dt."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        B = so.shape[0] - 1
        ext = np.zeros((B, _lib.EXTREMA_STRIDE), dtype=np.float64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_bounds_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), None if limits is None else ctypes.byref(limits), _ptr(ext),
            _ptr(flags)))
        return ext, flags

    def thrust(self, seg_offsets, seg_times, coeffs, g: float = 9.80665,
               limits: Optional[_lib.ThrustLimits] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Continuous thrust and tilt bounds (include/tgms.h tgms_thrust_batch): (rec [B,6] =
        f_min t_fmin f_max t_fmax tilt_max t_tilt of the mass-normalised thrust p'' + g e_z,
        flags [B] of THRUST_* bits against `limits`; None checks nothing)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        B = so.shape[0] - 1
        rec = np.zeros((B, _lib.THRUST_STRIDE), dtype=np.float64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_thrust_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), float(g), None if limits is None else ctypes.byref(limits),
            _ptr(rec), _ptr(flags)))
        return rec, flags

    def rate(self, seg_offsets, seg_times, coeffs, g: float = 9.80665,
             omega_limit: float = float("inf")) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Continuous body-rate bound (include/tgms.h tgms_rate_batch): (rec [B,2] = omega_max
        t_omega of the roll/pitch rate ||f x p'''|| / ||f||^2 with f = p'' + g e_z, seg_rec [S,2]
        = each segment's own maximum and local time, flags [B]: RATE_HIGH against `omega_limit`;
        inf checks nothing)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        B = so.shape[0] - 1
        rec = np.zeros((B, _lib.RATE_STRIDE), dtype=np.float64)
        seg_rec = np.zeros((T.shape[0], _lib.RATE_STRIDE), dtype=np.float64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_rate_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), float(g), float(omega_limit), _ptr(rec), _ptr(seg_rec),
            _ptr(flags)))
        return rec, seg_rec, flags

    def dilate(self, seg_offsets, seg_times, coeffs, g: float = 9.80665, limits: Optional[_lib.Limits] = None,
               tlimits: Optional[_lib.ThrustLimits] = None, s_lo: float = 1.0, s_hi: float = 100.0):
        """Time dilation (include/tgms.h tgms_dilate_batch): per trajectory the least stretch s in
        [s_lo, s_hi] that meets v_max / a_max / j_max of `limits` and f_min / f_max / tilt_max of
        `tlimits` (None: unchecked).  Returns (scale [B], active [B] of DIL_* codes, flags [B] =
        DIL_CAPPED / FEAS_NONFINITE with the evaluation count above DIL_EVALS_SHIFT, seg_times_out
        [S] = s T, coeffs_out [S,3,8] = c_k / s^k)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        B = so.shape[0] - 1
        scale = np.zeros(B, dtype=np.float64)
        active = np.zeros(B, dtype=np.int32)
        flags = np.zeros(B, dtype=np.int32)
        T_out, C_out = np.zeros_like(T), np.zeros_like(C)
        self._check(self._L.tgms_dilate_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), float(g), None if limits is None else ctypes.byref(limits),
            None if tlimits is None else ctypes.byref(tlimits), float(s_lo), float(s_hi), _ptr(scale), _ptr(active),
            _ptr(flags), _ptr(T_out), _ptr(C_out)))
        return scale, active, flags, T_out, C_out

    def retime(self, seg_offsets, seg_times, coeffs, limits: _lib.Limits, s_lo: float = 1.0, s_hi: float = 100.0):
        """Segment re-timing (include/tgms.h tgms_retime_batch): per segment the factor r_i its own
        continuous peaks ask for against v_max / a_max / j_max of `limits` and the time s_i T_i
        with s_i = min(s_hi, max(s_lo, r_i)).  Returns (T_out [S], seg_rec [S,4] = v a j r, rec
        [B,3] = r_max D_in D_out, flags [B] of RT_* bits with the worst segment's index above
        RT_SEG_SHIFT).  The coefficients are not scaled: solve again with T_out."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        B = so.shape[0] - 1
        T_out = np.zeros_like(T)
        seg_rec = np.zeros((T.shape[0], _lib.RETIME_STRIDE), dtype=np.float64)
        rec = np.zeros((B, _lib.RETIME_REC), dtype=np.float64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_retime_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), None if limits is None else ctypes.byref(limits), float(s_lo),
            float(s_hi), _ptr(T_out), _ptr(seg_rec), _ptr(rec), _ptr(flags)))
        return T_out, seg_rec, rec, flags

    def retime_loop(self, seg_offsets, waypoints, seg_times, limits: _lib.Limits, rounds: int, s_lo: float = 1.0,
                    s_hi: float = 4.0, end_derivs=None, dilate: bool = True):
        """Solve, re-time, solve again: up to `rounds` rounds of solve + retime on host arrays,
        stopping early when no trajectory carries RT_OVER, then a final solve and, if `dilate`, one
        uniform dilation with the same limits that closes what the rounds left over.  Returns (T,
        coeffs, history); history holds per round {"over": the share of trajectories with RT_OVER
        in the round's solve, "mean_D_out": the mean duration the round leaves}.  The round that
        finds none over is recorded, keeps its times and ends the loop."""
        so, W, T, _, ED = _csr(seg_offsets, waypoints, seg_times, end_derivs=end_derivs)
        history = []
        for _ in range(int(rounds)):
            C, _, _ = self.solve(so, W, T, ED)
            T_new, _, rec, flags = self.retime(so, T, C, limits, s_lo, s_hi)
            over = (flags & _lib.RT_OVER) != 0
            history.append({"over": float(over.mean()), "mean_D_out": float(np.nanmean(rec[:, 2 if over.any() else 1]))})
            if not over.any():
                break
            T = T_new
        C, _, _ = self.solve(so, W, T, ED)
        if dilate:
            _, _, _, T, C = self.dilate(so, T, C, limits=limits)
        return T, C, history

    def corridor(self, seg_offsets, seg_times, coeffs, faces, face_offsets=None, r: float = 0.0):
        """Corridor containment (include/tgms.h tgms_corridor_batch): faces [F,4] = n[3] d, a point
        inside when n . p <= d; face_offsets [S+1] int64 gives each segment its faces, None
        applies all F (at most COR_MAX_FACES) to every segment.  Returns (rec [B,2] = m_max
        t_max, where [B,2] = segment, face, seg_rec [S,2] = m_s t_s, seg_face [S], flags [B] of
        COR_* bits; COR_OUTSIDE when m_max > -r)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        fc = np.ascontiguousarray(faces, dtype=np.float64).reshape(-1, 4)
        fo = None if face_offsets is None else np.ascontiguousarray(face_offsets, dtype=np.int64)
        B, S = so.shape[0] - 1, int(so[-1])
        rec = np.zeros((B, _lib.COR_STRIDE), dtype=np.float64)
        where = np.zeros((B, 2), dtype=np.int32)
        seg_rec = np.zeros((S, _lib.COR_STRIDE), dtype=np.float64)
        seg_face = np.zeros(S, dtype=np.int32)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_corridor_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), fc.shape[0], _ptr(fc) if fc.shape[0] else None, _ptr(fo), float(r),
            _ptr(rec), _ptr(where), _ptr(seg_rec), _ptr(seg_face), _ptr(flags)))
        return rec, where, seg_rec, seg_face, flags

    def corridor_split(self, seg_offsets, waypoints, seg_times, coeffs, faces, face_offsets, seg_rec, seg_face,
                       r: float = 0.0, mode: int = _lib.SPLIT_PULL, min_frac: float = 0.1):
        """Corridor split (include/tgms.h tgms_corridor_split_batch): a waypoint at the worst
        excursion of every segment whose margin of the corridor call (seg_rec, seg_face; the same
        faces, face_offsets and r) exceeds -r.  Returns the new batch trimmed to its S' segments and
        F' faces: (seg_offsets' [B+1], waypoints' [S'+B,3], seg_times' [S'], faces' [F',4],
        face_offsets' [S'+1], parent [S'], flags [B] of SPLIT_* bits); in shared mode
        (face_offsets None) faces' is `faces` and face_offsets' is None."""
        so, W, T, C, _ = _csr(seg_offsets, waypoints, seg_times, coeffs)
        fc = np.ascontiguousarray(faces, dtype=np.float64).reshape(-1, 4)
        fo = None if face_offsets is None else np.ascontiguousarray(face_offsets, dtype=np.int64)
        sr = np.ascontiguousarray(seg_rec, dtype=np.float64).reshape(-1, _lib.COR_STRIDE)
        sf = np.ascontiguousarray(seg_face, dtype=np.int32)
        B, S, F = so.shape[0] - 1, int(so[-1]), fc.shape[0]
        so2 = np.zeros(B + 1, dtype=np.int32)
        W2 = np.zeros((2 * S + B, 3), dtype=np.float64)
        T2 = np.zeros(2 * S, dtype=np.float64)
        fc2 = None if fo is None else np.zeros((2 * F, 4), dtype=np.float64)
        fo2 = None if fo is None else np.zeros(2 * S + 1, dtype=np.int64)
        parent = np.zeros(2 * S, dtype=np.int32)
        totals = np.zeros(2, dtype=np.int64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_corridor_split_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(C), F, _ptr(fc) if F else None, _ptr(fo), _ptr(sr), _ptr(sf),
            float(r), int(mode), float(min_frac), _ptr(so2), _ptr(W2), _ptr(T2),
            _ptr(fc2) if fc2 is not None and F else None, _ptr(fo2), _ptr(parent), _ptr(totals), _ptr(flags)))
        S2, F2 = int(totals[0]), int(totals[1])
        if fo is None:
            return so2, W2[:S2 + B], T2[:S2], fc, None, parent[:S2], flags
        return so2, W2[:S2 + B], T2[:S2], fc2[:F2], fo2[:S2 + 1], parent[:S2], flags

    def cut(self, seg_offsets, waypoints, seg_times, coeffs, t_cut, min_frac: float = 0.1, end_derivs=None,
            want_coeffs: bool = True):
        """Replan cut (include/tgms.h tgms_cut_batch): every trajectory restarted from its state at
        t_cut [B].  Returns the new batch trimmed to its S' segments: (seg_offsets' [B+1],
        waypoints' [S'+B,3], seg_times' [S'], end_derivs' [B,18], coeffs' [S',3,8] (the tail without
        a solve; None when want_coeffs is False), parent [S'], t0 [B], flags [B] of CUT_* bits)."""
        so, W, T, C, ED = _csr(seg_offsets, waypoints, seg_times, coeffs, end_derivs)
        tc = np.ascontiguousarray(t_cut, dtype=np.float64).reshape(-1)
        B = so.shape[0] - 1
        S = int(so[-1]) if B > 0 else 0
        if tc.shape[0] != B:
            raise ValueError("t_cut must have one entry per trajectory")
        so2 = np.zeros(B + 1, dtype=np.int32)
        W2 = np.zeros((S + B, 3), dtype=np.float64)
        T2 = np.zeros(S, dtype=np.float64)
        ED2 = np.zeros((B, 18), dtype=np.float64)
        C2 = np.zeros((S, 3, 8), dtype=np.float64) if want_coeffs else None
        parent = np.zeros(S, dtype=np.int32)
        t0 = np.zeros(B, dtype=np.float64)
        totals = np.zeros(1, dtype=np.int64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_cut_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(ED), _ptr(C), _ptr(tc), float(min_frac), _ptr(so2), _ptr(W2),
            _ptr(T2), _ptr(ED2), _ptr(C2), _ptr(parent), _ptr(t0), _ptr(totals), _ptr(flags)))
        S2 = int(totals[0])
        return so2, W2[:S2 + B], T2[:S2], ED2, None if C2 is None else C2[:S2], parent[:S2], t0, flags

    def corridor_loop(self, seg_offsets, waypoints, seg_times, faces, face_offsets, r: float, rounds: int,
                      mode: int = _lib.SPLIT_PULL, min_frac: float = 0.1, end_derivs=None):
        """The planner's loop on host arrays: solve, corridor, split, up to `rounds` times, stopping
        when no trajectory carries COR_OUTSIDE.  Returns ((seg_offsets, waypoints, seg_times, faces,
        face_offsets), coeffs, flagged): the final batch, its coefficients and the number of
        flagged trajectories found in each round."""
        so, W, T, fc, fo = seg_offsets, waypoints, seg_times, faces, face_offsets
        flagged = []
        while True:
            C, _, worst = self.solve(so, W, T, end_derivs)
            self._check(worst)
            _, _, seg_rec, seg_face, fl = self.corridor(so, T, C, fc, fo, r)
            flagged.append(int(((fl & _lib.COR_OUTSIDE) != 0).sum()))
            if flagged[-1] == 0 or len(flagged) > rounds:
                return (so, W, T, fc, fo), C, flagged
            so, W, T, fc, fo, _, _ = self.corridor_split(so, W, T, C, fc, fo, seg_rec, seg_face, r, mode, min_frac)

    def separation(self, seg_offsets, seg_times, coeffs, pairs=None, start_times=None, scale=None,
                   r_min: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
        """Continuous swarm separation (include/tgms.h tgms_separation_batch): per pair the
        closest approach (sep [P,2] = d_min t_min, flags [P] of SEP_* bits).  pairs: int32
        [P,2], or None for every unordered pair (0,1), (0,2), ..., (1,2), ...; start_times [B]
        (None: all 0); scale: the three per-axis factors (None: 1, 1, 1)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        t0 = None if start_times is None else np.ascontiguousarray(start_times, dtype=np.float64).reshape(-1)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(3)
        B = so.shape[0] - 1
        if pairs is None:
            pr, P = None, B * (B - 1) // 2
        else:
            pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            P = pr.shape[0]
        sep = np.full((P, _lib.SEP_STRIDE), np.nan, dtype=np.float64)
        flags = np.full(P, -1, dtype=np.int32)
        self._check(self._L.tgms_separation_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), _ptr(t0), P, _ptr(pr), _ptr(sc), float(r_min), _ptr(sep),
            _ptr(flags)))
        return sep, flags

    def neighbors(self, seg_offsets, seg_times, coeffs, r_min: float, start_times=None, scale=None):
        """Swarm neighbour search (include/tgms.h tgms_neighbors_batch): per vehicle the nearest
        other vehicle whose closest approach is below r_min.  Returns (near [B,2] = d_min t_min,
        nbr [B] (NEAR_NONE: nobody), count [B], tested [B], flags [B] of SEP_* bits)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        t0 = None if start_times is None else np.ascontiguousarray(start_times, dtype=np.float64).reshape(-1)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(3)
        B = so.shape[0] - 1
        near = np.full((B, _lib.SEP_STRIDE), np.nan, dtype=np.float64)
        nbr, count, tested, flags = (np.full(B, -2, dtype=np.int32) for _ in range(4))
        self._check(self._L.tgms_neighbors_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), _ptr(t0), _ptr(sc), float(r_min), _ptr(near), _ptr(nbr),
            _ptr(count), _ptr(tested), _ptr(flags)))
        return near, nbr, count, tested, flags

    def clearance(self, seg_offsets, seg_times, coeffs, obstacles, r_min: float, scale=None):
        """Obstacle clearance (include/tgms.h tgms_clearance_batch): per trajectory the nearest of
        the static boxes `obstacles` [K,6] = lo[3] hi[3] whose distance falls below r_min.  Returns
        (near [B,2] = d_min t_min, obs [B] (NEAR_NONE: none), count [B], tested [B], flags [B] of
        SEP_* bits and CLR_BAD_OBSTACLE)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        ob = np.ascontiguousarray(obstacles, dtype=np.float64).reshape(-1, 6)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(3)
        B, K = so.shape[0] - 1, ob.shape[0]
        near = np.full((B, _lib.SEP_STRIDE), np.nan, dtype=np.float64)
        obs, count, tested, flags = (np.full(B, -2, dtype=np.int32) for _ in range(4))
        self._check(self._L.tgms_clearance_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), K, _ptr(ob) if K else None, _ptr(sc), float(r_min), _ptr(near),
            _ptr(obs), _ptr(count), _ptr(tested), _ptr(flags)))
        return near, obs, count, tested, flags

    def field_clearance(self, seg_offsets, seg_times, coeffs, origin, h: float, values, r_min: float, tol: float,
                        lip: float = 0.0, max_evals: int = 1 << 20):
        """Distance-field clearance (include/tgms.h tgms_field_clearance_batch): per trajectory the
        least value of the voxel field `values` [nz,ny,nx] (float32, node (0,0,0) at `origin`,
        spacing h) along it, certified to tol below r_min.  lip: a Lipschitz bound of the field,
        0 to have it reduced from the values.  Returns (near [B,2] = d_min t_min, evals [B],
        flags [B] of SEP_* bits and FLD_UNRESOLVED)."""
        so, _, T, C, _ = _csr(seg_offsets, seg_times=seg_times, coeffs=coeffs)
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.ndim == 3, "values must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, v.shape[::-1])
        B = so.shape[0] - 1
        near = np.full((B, _lib.SEP_STRIDE), np.nan, dtype=np.float64)
        evals, flags = (np.full(B, -2, dtype=np.int32) for _ in range(2))
        self._check(self._L.tgms_field_clearance_batch(
            self._h, B, _ptr(so), _ptr(T), _ptr(C), ctypes.byref(fld), _ptr(v), float(lip), float(r_min), float(tol),
            int(max_evals), _ptr(near), _ptr(evals), _ptr(flags)))
        return near, evals, flags

    def corridor_inflate(self, seg_offsets, waypoints, origin, h: float, values, r_free: float, max_grow: int):
        """Corridor inflation (include/tgms.h tgms_corridor_inflate_batch): per segment of the
        waypoint paths the largest box of free nodes (value >= float32(r_free)) of the voxel field
        `values` [nz,ny,nx] that `max_grow` rounds of growth reach from the segment's own lattice
        bounding box.  Returns (box [S,6] = lo[3] hi[3], faces [6S,4] and face_offsets [S+1] as
        corridor() and corridor_loop() take them, seg_flags [S] and flags [B] of INF_* bits and
        FEAS_NONFINITE)."""
        so, W, _, _, _ = _csr(seg_offsets, waypoints)
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.ndim == 3, "values must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, v.shape[::-1])
        B = so.shape[0] - 1
        S = int(so[-1]) if B > 0 else 0
        box = np.full((S, 6), -2, dtype=np.int32)
        faces = np.full((6 * S, 4), np.nan, dtype=np.float64)
        fo = np.full(S + 1, -2, dtype=np.int64)
        seg_flags, flags = np.full(S, -2, dtype=np.int32), np.full(B, -2, dtype=np.int32)
        self._check(self._L.tgms_corridor_inflate_batch(
            self._h, B, _ptr(so), _ptr(W), ctypes.byref(fld), _ptr(v), float(r_free), int(max_grow), _ptr(box),
            _ptr(faces), _ptr(fo), _ptr(seg_flags), _ptr(flags)))
        return box, faces, fo, seg_flags, flags

    def corridor_subdivide(self, seg_offsets, waypoints, origin, h: float, values, r_free: float,
                           max_depth: int = _lib.SUB_MAX_DEPTH, seg_times=None):
        """Corridor subdivision (include/tgms.h tgms_corridor_subdivide_batch): every leg whose own
        lattice bounding box holds a non-free node of the voxel field `values` [nz,ny,nx] is halved,
        down to 2^-max_depth of the leg, until its pieces have free boxes or the trajectory would
        pass MAX_SEGMENTS.  Returns the new batch trimmed to its S' segments: (seg_offsets' [B+1],
        waypoints' [S'+B,3], seg_times' [S'] (None without seg_times), parent [S'], seg_flags [S']
        and flags [B] of SUB_* bits and FEAS_NONFINITE)."""
        so, W, T, _, _ = _csr(seg_offsets, waypoints, seg_times)
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.ndim == 3, "values must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, v.shape[::-1])
        B = so.shape[0] - 1
        S = int(so[-1]) if B > 0 else 0
        cap = min(S << max(0, min(int(max_depth), _lib.SUB_MAX_DEPTH)), _lib.MAX_SEGMENTS * B)
        so2 = np.zeros(B + 1, dtype=np.int32)
        W2 = np.zeros((cap + B, 3), dtype=np.float64)
        T2 = None if T is None else np.zeros(cap, dtype=np.float64)
        parent, seg_flags = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        totals = np.zeros(1, dtype=np.int64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_corridor_subdivide_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), ctypes.byref(fld), _ptr(v), float(r_free), int(max_depth),
            _ptr(so2), _ptr(W2), _ptr(T2), _ptr(parent), _ptr(seg_flags), _ptr(totals), _ptr(flags)))
        S2 = int(totals[0])
        return so2, W2[:S2 + B], None if T2 is None else T2[:S2], parent[:S2], seg_flags[:S2], flags

    def corridor_reroute(self, seg_offsets, waypoints, origin, h: float, values, r_free: float, margin: int,
                         max_pieces: int = _lib.RRT_MAX_PIECES, seg_times=None):
        """Corridor re-route (include/tgms.h tgms_corridor_reroute_batch): every leg whose own lattice
        bounding box holds a non-free node of the voxel field `values` [nz,ny,nx] is replaced by a
        shortest 6-neighbour path through the free nodes of its box widened by `margin` nodes, reduced
        to at most max_pieces pieces with free boxes.  Returns the new batch trimmed to its S' segments:
        (seg_offsets' [B+1], waypoints' [S'+B,3], seg_times' [S'] (None without seg_times), parent
        [S'], seg_flags [S'], hops [S] per input segment (NEAR_NONE: not searched or no path) and
        flags [B] of RRT_* bits and FEAS_NONFINITE)."""
        so, W, T, _, _ = _csr(seg_offsets, waypoints, seg_times)
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.ndim == 3, "values must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, v.shape[::-1])
        B = so.shape[0] - 1
        S = int(so[-1]) if B > 0 else 0
        cap = min(S * max(2, min(int(max_pieces), _lib.RRT_MAX_PIECES)), _lib.MAX_SEGMENTS * B)
        so2 = np.zeros(B + 1, dtype=np.int32)
        W2 = np.zeros((cap + B, 3), dtype=np.float64)
        T2 = None if T is None else np.zeros(cap, dtype=np.float64)
        parent, seg_flags = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        hops = np.zeros(S, dtype=np.int32)
        totals = np.zeros(1, dtype=np.int64)
        flags = np.zeros(B, dtype=np.int32)
        self._check(self._L.tgms_corridor_reroute_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), ctypes.byref(fld), _ptr(v), float(r_free), int(margin),
            int(max_pieces), _ptr(so2), _ptr(W2), _ptr(T2), _ptr(parent), _ptr(seg_flags), _ptr(hops), _ptr(totals),
            _ptr(flags)))
        S2 = int(totals[0])
        return so2, W2[:S2 + B], None if T2 is None else T2[:S2], parent[:S2], seg_flags[:S2], hops, flags

    def field_edt(self, occ, origin, h: float, max_dist: float, signed: bool = False):
        """Distance-field build (include/tgms.h tgms_field_edt): the exact Euclidean distance
        transform of the occupancy grid `occ` [nz,ny,nx] (uint8, occupied where not 0; node (0,0,0) at
        `origin`, spacing h), capped at max_dist.  signed: negative inside, the zero level half a
        spacing outside the occupied nodes.  Returns (values [nz,ny,nx] float32, as the other map
        calls take them, d2 [nz,ny,nx] int32, the squared lattice distances capped at R^2)."""
        o = np.ascontiguousarray(occ, dtype=np.uint8)
        assert o.ndim == 3, "occ must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, o.shape[::-1])
        values = np.full(o.shape, np.nan, dtype=np.float32)
        d2 = np.zeros(o.shape, dtype=np.int32)
        self._check(self._L.tgms_field_edt(
            self._h, ctypes.byref(fld), _ptr(o), float(max_dist), _lib.EDT_SIGNED if signed else 0, _ptr(values),
            _ptr(d2)))
        return values, d2

    def field_edt_work_size(self, origin, h: float, n, signed: bool = False) -> int:
        """tgms_field_edt_work_size: the bytes of field_edt_device's workspace for a grid of n = (nx,
        ny, nz) nodes; 0 for a grid the call refuses."""
        fld = _lib.Field(origin, h, n)
        return int(self._L.tgms_field_edt_work_size(ctypes.byref(fld), _lib.EDT_SIGNED if signed else 0))

    def field_nearest_free(self, values, origin, h: float, r_free: float, max_shift: int):
        """Nearest-free map (include/tgms.h tgms_field_nearest_free): per node of the voxel field
        `values` [nz,ny,nx] the linear index (k ny + j) nx + i of the nearest free node (value >=
        float32(r_free)) within max_shift spacings, ties to the lowest index, and its squared lattice
        distance; NEAR_NONE where there is none.  Returns (nearest, dsq), both [nz,ny,nx] int32."""
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.ndim == 3, "values must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, v.shape[::-1])
        nearest = np.full(v.shape, -2, dtype=np.int32)
        dsq = np.full(v.shape, -2, dtype=np.int32)
        self._check(self._L.tgms_field_nearest_free(
            self._h, ctypes.byref(fld), _ptr(v), float(r_free), int(max_shift), _ptr(nearest), _ptr(dsq)))
        return nearest, dsq

    def field_nearest_free_work_size(self, origin, h: float, n) -> int:
        """tgms_field_nearest_free_work_size: the bytes of field_nearest_free_device's workspace for a
        grid of n = (nx, ny, nz) nodes; 0 for a grid the call refuses."""
        fld = _lib.Field(origin, h, n)
        return int(self._L.tgms_field_nearest_free_work_size(ctypes.byref(fld)))

    def waypoints_repair(self, seg_offsets, waypoints, origin, h: float, values, r_free: float, max_shift: int,
                         mode: int = 0, seg_times=None):
        """Waypoint repair (include/tgms.h tgms_waypoints_repair_batch): every waypoint whose own cell
        holds a non-free node of the voxel field `values` [nz,ny,nx] moves onto the free node nearest
        to its nearest node, at most max_shift spacings away; mode: RPR_KEEP_FIRST | RPR_KEEP_LAST.
        seg_offsets do not change.  Returns (waypoints' [S+B,3], seg_times' [S] (None without
        seg_times), wp_flags [S+B] and flags [B] of RPR_* bits and FEAS_NONFINITE, shift [S+B]: the
        squared lattice distance of a moved waypoint, NEAR_NONE otherwise)."""
        so, W, T, _, _ = _csr(seg_offsets, waypoints, seg_times)
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.ndim == 3, "values must be [nz, ny, nx]"
        fld = _lib.Field(origin, h, v.shape[::-1])
        B = so.shape[0] - 1
        S = int(so[-1]) if B > 0 else 0
        W2 = np.zeros((S + B, 3), dtype=np.float64)
        T2 = None if T is None else np.zeros(S, dtype=np.float64)
        wp_flags, shift = np.full(S + B, -2, dtype=np.int32), np.full(S + B, -2, dtype=np.int32)
        flags = np.full(B, -2, dtype=np.int32)
        self._check(self._L.tgms_waypoints_repair_batch(
            self._h, B, _ptr(so), _ptr(W), _ptr(T), ctypes.byref(fld), _ptr(v), float(r_free), int(max_shift), int(mode),
            _ptr(W2), _ptr(T2), _ptr(wp_flags), _ptr(shift), _ptr(flags)))
        return W2, T2, wp_flags, flags, shift

    def corridor_from_map(self, seg_offsets, waypoints, seg_times, origin, h: float, values, r_free: float,
                          max_grow: int, max_depth: int = _lib.SUB_MAX_DEPTH, reroute=None, repair=None):
        """From a voxel map to what corridor_loop() takes, on host arrays: corridor_subdivide, then
        corridor_inflate on its output.  Returns ((seg_offsets, waypoints, seg_times, faces,
        face_offsets), (sub_flags [B], sub_seg_flags [S'], inf_seg_flags [S'], inf_flags [B])); a
        segment with SUB_BLOCKED is the one with INF_BLOCKED and needs re-routing.  reroute = (margin,
        max_pieces): corridor_reroute runs between the two; the batch and the inflation flags are those
        of its output (the subdivision's segment flags stay those of the subdivision's S' rows) and the
        second tuple gains (rrt_flags [B], rrt_seg_flags [S''], rrt_parent [S''], rrt_hops [S']).
        repair = (max_shift, mode): waypoints_repair runs first, the rest sees its waypoints and times,
        and the second tuple gains, last, (rpr_flags [B], rpr_wp_flags [S+B], rpr_shift [S+B])."""
        rpr = ()
        if repair is not None:
            max_shift, mode = repair
            waypoints, seg_times, rpr_wp, rpr_fl, rpr_shift = self.waypoints_repair(
                seg_offsets, waypoints, origin, h, values, r_free, max_shift, mode, seg_times)
            rpr = (rpr_fl, rpr_wp, rpr_shift)
        so, W, T, _, sub_seg, sub_fl = self.corridor_subdivide(seg_offsets, waypoints, origin, h, values, r_free,
                                                               max_depth, seg_times)
        rrt = ()
        if reroute is not None:
            margin, max_pieces = reroute
            so, W, T, rrt_par, rrt_seg, rrt_hops, rrt_fl = self.corridor_reroute(so, W, origin, h, values, r_free,
                                                                                 margin, max_pieces, T)
            rrt = (rrt_fl, rrt_seg, rrt_par, rrt_hops)
        _, faces, fo, inf_seg, inf_fl = self.corridor_inflate(so, W, origin, h, values, r_free, max_grow)
        return (so, W, T, faces, fo), (sub_fl, sub_seg, inf_seg, inf_fl) + rrt + rpr

    def refine(self, seg_offsets, waypoints, seg_times, end_derivs=None, k_T: float = 1.0, eta: float = 0.1,
               iters: int = 10, coeffs: bool = True):
        """Time-allocation refinement on the GPU (include/tgms.h tgms_refine_batch).
        Returns (T [S], coeffs [S,3,8] or None, cost [B], status [B], worst)."""
        so, W, _, _, ED = _csr(seg_offsets, waypoints, end_derivs=end_derivs)
        T = np.array(seg_times, dtype=np.float64).reshape(-1)
        B = so.shape[0] - 1
        C = np.zeros((int(so[-1]), 3, 8), dtype=np.float64) if coeffs else None
        cost = np.zeros(max(B, 1), dtype=np.float64)
        st = np.zeros(max(B, 1), dtype=np.int32)
        worst = self._L.tgms_refine_batch(self._h, B, _ptr(so), _ptr(W), _ptr(T), _ptr(ED), float(k_T), float(eta),
                                          int(iters), _ptr(C), _ptr(cost), _ptr(st))
        if worst in (_lib.ERR_DEVICE, _lib.ERR_NO_DEVICE):
            raise TgmsError(worst, self.last_error())
        return T, C, cost[:B], st[:B], worst

    # -------------------------------------------------------------- device API
    def refine_uniform_device(self, B: int, M: int, d_waypoints, d_seg_times, d_seg_times_out, k_T: float,
                              eta: float, d_cost=None, d_status=None, d_end_derivs=None, stream: int = 0) -> None:
        self._check(self._L.tgms_refine_uniform_device(
            self._h, int(B), int(M), _ptr(d_waypoints), _ptr(d_seg_times), _ptr(d_end_derivs), float(k_T), float(eta),
            _ptr(d_seg_times_out), _ptr(d_cost), _ptr(d_status), ctypes.c_void_p(stream)))

    def refine_loop_device(self, h_seg_offsets, d_seg_offsets, d_waypoints, d_seg_times, k_T: float, eta: float,
                           iters: int, d_coeffs=None, d_cost=None, d_status=None, d_end_derivs=None,
                           stream: int = 0) -> None:
        so = np.ascontiguousarray(h_seg_offsets, dtype=np.int32)
        self._check(self._L.tgms_refine_loop_device(
            self._h, int(so.shape[0] - 1), _ptr(so), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times),
            _ptr(d_end_derivs), float(k_T), float(eta), int(iters), _ptr(d_coeffs), _ptr(d_cost), _ptr(d_status),
            ctypes.c_void_p(stream)))

    def refine_batch_device(self, h_seg_offsets, d_seg_offsets, d_waypoints, d_seg_times, d_seg_times_out,
                            k_T: float, eta: float, d_cost=None, d_status=None, d_end_derivs=None,
                            stream: int = 0) -> None:
        so = np.ascontiguousarray(h_seg_offsets, dtype=np.int32)
        self._check(self._L.tgms_refine_batch_device(
            self._h, int(so.shape[0] - 1), _ptr(so), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times),
            _ptr(d_end_derivs), float(k_T), float(eta), _ptr(d_seg_times_out), _ptr(d_cost), _ptr(d_status),
            ctypes.c_void_p(stream)))

    def solve_uniform_device(self, B: int, M: int, d_waypoints, d_seg_times, d_coeffs, d_status=None,
                             d_end_derivs=None, stream: int = 0) -> None:
        self._check(self._L.tgms_solve_uniform_device(
            self._h, int(B), int(M), _ptr(d_waypoints), _ptr(d_seg_times), _ptr(d_end_derivs), _ptr(d_coeffs),
            _ptr(d_status), ctypes.c_void_p(stream)))

    def solve_batch_device(self, h_seg_offsets, d_seg_offsets, d_waypoints, d_seg_times, d_coeffs,
                           d_status=None, d_end_derivs=None, stream: int = 0) -> None:
        so = np.ascontiguousarray(h_seg_offsets, dtype=np.int32)
        self._check(self._L.tgms_solve_batch_device(
            self._h, int(so.shape[0] - 1), _ptr(so), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times),
            _ptr(d_end_derivs), _ptr(d_coeffs), _ptr(d_status), ctypes.c_void_p(stream)))

    def solve_batch_multi_device(self, h_seg_offsets, d_seg_offsets, d_waypoints, d_seg_times, d_coeffs,
                                 d_status=None, d_end_derivs=None, stream: int = 0) -> None:
        so = np.ascontiguousarray(h_seg_offsets, dtype=np.int32)
        self._check(self._L.tgms_solve_batch_multi_device(
            self._h, int(so.shape[0] - 1), _ptr(so), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times),
            _ptr(d_end_derivs), _ptr(d_coeffs), _ptr(d_status), ctypes.c_void_p(stream)))

    def refine_loop_multi_device(self, h_seg_offsets, d_seg_offsets, d_waypoints, d_seg_times, k_T: float,
                                 eta: float, iters: int, d_coeffs=None, d_cost=None, d_status=None,
                                 d_end_derivs=None, stream: int = 0) -> None:
        so = np.ascontiguousarray(h_seg_offsets, dtype=np.int32)
        self._check(self._L.tgms_refine_loop_multi_device(
            self._h, int(so.shape[0] - 1), _ptr(so), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times),
            _ptr(d_end_derivs), float(k_T), float(eta), int(iters), _ptr(d_coeffs), _ptr(d_cost), _ptr(d_status),
            ctypes.c_void_p(stream)))

    def sample_device(self, B: int, d_seg_offsets, d_waypoints, d_seg_times, d_coeffs, dt: float,
                      d_sample_offsets, d_out, d_end_derivs=None, yaw_mode: int = _lib.YAW_CONSTANT,
                      yaw_const: float = 0.0, stream: int = 0) -> None:
        self._check(self._L.tgms_sample_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), _ptr(d_end_derivs),
            _ptr(d_coeffs), float(dt), int(yaw_mode), float(yaw_const), _ptr(d_sample_offsets), _ptr(d_out),
            ctypes.c_void_p(stream)))

    def extrema_device(self, B: int, d_seg_offsets, d_waypoints, d_seg_times, d_coeffs, dt: float,
                       limits: Optional[_lib.Limits] = None, d_extrema=None, d_flags=None, d_end_derivs=None,
                       stream: int = 0) -> None:
        """tgms_extrema_batch_device: d_extrema [B,10] fp64 and / or d_flags [B] int32 (at
        least one); `limits` is read now, so it may change before the kernel runs."""
        self._check(self._L.tgms_extrema_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), _ptr(d_end_derivs),
            _ptr(d_coeffs), float(dt), None if limits is None else ctypes.byref(limits), _ptr(d_extrema), _ptr(d_flags),
            ctypes.c_void_p(stream)))

    def bounds_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, limits: Optional[_lib.Limits] = None,
                      d_extrema=None, d_flags=None, stream: int = 0) -> None:
        """tgms_bounds_batch_device: d_extrema [B,10] fp64 and / or d_flags [B] int32 (at
        least one); `limits` is read now, so it may change before the kernel runs."""
        self._check(self._L.tgms_bounds_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs),
            None if limits is None else ctypes.byref(limits), _ptr(d_extrema), _ptr(d_flags), ctypes.c_void_p(stream)))

    def thrust_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, g: float = 9.80665,
                      limits: Optional[_lib.ThrustLimits] = None, d_rec=None, d_flags=None, stream: int = 0) -> None:
        """tgms_thrust_batch_device: d_rec [B,6] fp64 and / or d_flags [B] int32 (at least
        one); g and `limits` are read now, so they may change before the kernel runs."""
        self._check(self._L.tgms_thrust_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), float(g),
            None if limits is None else ctypes.byref(limits), _ptr(d_rec), _ptr(d_flags), ctypes.c_void_p(stream)))

    def rate_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, g: float = 9.80665,
                    omega_limit: float = float("inf"), d_rec=None, d_seg_rec=None, d_flags=None,
                    stream: int = 0) -> None:
        """tgms_rate_batch_device: d_rec [B,2] fp64, d_seg_rec [S,2] fp64 and / or d_flags [B]
        int32 (at least one); g and `omega_limit` travel as kernel arguments."""
        self._check(self._L.tgms_rate_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), float(g), float(omega_limit),
            _ptr(d_rec), _ptr(d_seg_rec), _ptr(d_flags), ctypes.c_void_p(stream)))

    def dilate_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, g: float = 9.80665,
                      limits: Optional[_lib.Limits] = None, tlimits: Optional[_lib.ThrustLimits] = None,
                      s_lo: float = 1.0, s_hi: float = 100.0, d_scale=None, d_active=None, d_flags=None,
                      d_seg_times_out=None, d_coeffs_out=None, stream: int = 0) -> None:
        """tgms_dilate_batch_device: d_scale [B] fp64, d_active [B] int32, d_flags [B] int32,
        d_seg_times_out [S] fp64, d_coeffs_out [S,3,8] fp64 (at least one; the last two may be the
        inputs themselves); g and the limits are read now, so they may change before the kernel runs."""
        self._check(self._L.tgms_dilate_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), float(g),
            None if limits is None else ctypes.byref(limits), None if tlimits is None else ctypes.byref(tlimits),
            float(s_lo), float(s_hi), _ptr(d_scale), _ptr(d_active), _ptr(d_flags), _ptr(d_seg_times_out),
            _ptr(d_coeffs_out), ctypes.c_void_p(stream)))

    def retime_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, limits: _lib.Limits, s_lo: float = 1.0,
                      s_hi: float = 100.0, d_seg_times_out=None, d_seg_rec=None, d_rec=None, d_flags=None,
                      stream: int = 0) -> None:
        """tgms_retime_batch_dev: d_seg_times_out [S] fp64 (may be d_seg_times itself), d_seg_rec
        [S,4] fp64, d_rec [B,3] fp64, d_flags [B] int32 (at least one); the limits are read now,
        so they may change before the kernel runs."""
        self._check(self._L.tgms_retime_batch_dev(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs),
            None if limits is None else ctypes.byref(limits), float(s_lo), float(s_hi), _ptr(d_seg_times_out),
            _ptr(d_seg_rec), _ptr(d_rec), _ptr(d_flags), ctypes.c_void_p(stream)))

    def corridor_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, F: int, d_faces, d_face_offsets=None,
                        r: float = 0.0, d_rec=None, d_where=None, d_seg_rec=None, d_seg_face=None, d_flags=None,
                        stream: int = 0) -> None:
        """tgms_corridor_batch_device: d_faces [F,4] fp64, d_face_offsets [S+1] int64 or None (all
        F faces apply to every segment); d_rec [B,2] fp64, d_where [B,2] int32, d_seg_rec [S,2]
        fp64, d_seg_face [S] int32, d_flags [B] int32 (at least one)."""
        self._check(self._L.tgms_corridor_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), int(F), _ptr(d_faces),
            _ptr(d_face_offsets), float(r), _ptr(d_rec), _ptr(d_where), _ptr(d_seg_rec), _ptr(d_seg_face),
            _ptr(d_flags), ctypes.c_void_p(stream)))

    def corridor_split_device(self, B: int, d_seg_offsets, d_waypoints, d_seg_times, d_coeffs, F: int, d_faces,
                              d_face_offsets, d_seg_rec, d_seg_face, r: float, mode: int, min_frac: float,
                              d_seg_offsets_out, d_waypoints_out, d_seg_times_out, d_faces_out=None,
                              d_face_offsets_out=None, d_parent=None, d_totals=None, d_flags=None,
                              stream: int = 0) -> None:
        """tgms_corridor_split_batch_device: outputs sized for 2 S segments and 2 F faces
        (d_seg_offsets_out [B+1] int32, d_waypoints_out [2S+B,3], d_seg_times_out [2S], d_faces_out
        [2F,4], d_face_offsets_out [2S+1] int64, d_parent [2S] int32, d_totals [2] int64 = S' F',
        d_flags [B] int32); shared mode (d_face_offsets None) takes no face outputs.  Not
        capturable: it grows handle scratch with B."""
        self._check(self._L.tgms_corridor_split_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), _ptr(d_coeffs), int(F),
            _ptr(d_faces), _ptr(d_face_offsets), _ptr(d_seg_rec), _ptr(d_seg_face), float(r), int(mode),
            float(min_frac), _ptr(d_seg_offsets_out), _ptr(d_waypoints_out), _ptr(d_seg_times_out), _ptr(d_faces_out),
            _ptr(d_face_offsets_out), _ptr(d_parent), _ptr(d_totals), _ptr(d_flags), ctypes.c_void_p(stream)))

    def cut_device(self, B: int, d_seg_offsets, d_waypoints, d_seg_times, d_coeffs, d_t_cut, min_frac: float,
                   d_seg_offsets_out, d_waypoints_out, d_seg_times_out, d_end_derivs_out, d_totals,
                   d_end_derivs=None, d_coeffs_out=None, d_parent=None, d_t0_out=None, d_flags=None,
                   stream: int = 0) -> None:
        """tgms_cut_batch_device: outputs sized as the inputs (d_seg_offsets_out [B+1] int32,
        d_waypoints_out [S+B,3], d_seg_times_out [S], d_end_derivs_out [B,18], d_coeffs_out [S,3,8],
        d_parent [S] int32, d_t0_out [B], d_totals [1] int64 = S', d_flags [B] int32).  Not
        capturable: it grows handle scratch with B."""
        self._check(self._L.tgms_cut_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), _ptr(d_end_derivs),
            _ptr(d_coeffs), _ptr(d_t_cut), float(min_frac), _ptr(d_seg_offsets_out), _ptr(d_waypoints_out),
            _ptr(d_seg_times_out), _ptr(d_end_derivs_out), _ptr(d_coeffs_out), _ptr(d_parent), _ptr(d_t0_out),
            _ptr(d_totals), _ptr(d_flags), ctypes.c_void_p(stream)))

    def separation_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, P: int, d_pairs=None,
                          d_start_times=None, scale=None, r_min: float = 0.0, d_sep=None, d_flags=None,
                          stream: int = 0) -> None:
        """tgms_separation_batch_device: d_sep [P,2] fp64 and / or d_flags [P] int32 (at least
        one); d_pairs int32 [P,2] or None for all pairs (P = B (B - 1) / 2); `scale` (host,
        three values or None) and r_min are read now."""
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(3)
        self._check(self._L.tgms_separation_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), _ptr(d_start_times), int(P),
            _ptr(d_pairs), _ptr(sc), float(r_min), _ptr(d_sep), _ptr(d_flags), ctypes.c_void_p(stream)))

    def neighbors_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, r_min: float, d_start_times=None,
                         scale=None, d_near=None, d_nbr=None, d_count=None, d_tested=None, d_flags=None,
                         stream: int = 0) -> None:
        """tgms_neighbors_batch_device: d_near [B,2] fp64, d_nbr / d_count / d_tested / d_flags
        [B] int32 (at least one of near, nbr, count, flags); `scale` (host, three values or
        None) and r_min are read now.  Not capturable: it grows handle scratch with B."""
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(3)
        self._check(self._L.tgms_neighbors_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), _ptr(d_start_times), _ptr(sc),
            float(r_min), _ptr(d_near), _ptr(d_nbr), _ptr(d_count), _ptr(d_tested), _ptr(d_flags),
            ctypes.c_void_p(stream)))

    def clearance_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, K: int, d_obstacles, r_min: float,
                         scale=None, d_near=None, d_obs=None, d_count=None, d_tested=None, d_flags=None,
                         stream: int = 0) -> None:
        """tgms_clearance_batch_device: d_obstacles [K,6] fp64, d_near [B,2] fp64, d_obs / d_count /
        d_tested / d_flags [B] int32 (at least one of near, obs, count, flags); `scale` (host, three
        values or None) and r_min are read now.  Not capturable: it grows handle scratch with B, K."""
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(3)
        self._check(self._L.tgms_clearance_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), int(K), _ptr(d_obstacles),
            _ptr(sc), float(r_min), _ptr(d_near), _ptr(d_obs), _ptr(d_count), _ptr(d_tested), _ptr(d_flags),
            ctypes.c_void_p(stream)))

    def field_clearance_device(self, B: int, d_seg_offsets, d_seg_times, d_coeffs, origin, h: float, n, d_values,
                               lip: float, r_min: float, tol: float, max_evals: int, d_near=None, d_evals=None,
                               d_flags=None, stream: int = 0) -> None:
        """tgms_field_clearance_batch_device: n = (nx, ny, nz), d_values fp32 with x fastest, d_near
        [B,2] fp64, d_evals / d_flags [B] int32 (at least one of the three); the grid, lip, r_min,
        tol and max_evals are read now.  Capturable with lip > 0; lip == 0 uses handle scratch."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_field_clearance_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_seg_times), _ptr(d_coeffs), ctypes.byref(fld), _ptr(d_values),
            float(lip), float(r_min), float(tol), int(max_evals), _ptr(d_near), _ptr(d_evals), _ptr(d_flags),
            ctypes.c_void_p(stream)))

    def field_occupancy_device(self, origin, h: float, n, d_values, r_free: float, d_table, stream: int = 0) -> None:
        """tgms_field_occupancy_device: n = (nx, ny, nz), d_values fp32 with x fastest; d_table int32
        [(nz+1),(ny+1),(nx+1)] receives the summed-volume table of the nodes below float32(r_free).
        Three launches, no handle scratch: capturable."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_field_occupancy_device(
            self._h, ctypes.byref(fld), _ptr(d_values), float(r_free), _ptr(d_table), ctypes.c_void_p(stream)))

    def field_edt_device(self, origin, h: float, n, d_occ, max_dist: float, d_work, d_values=None, d_d2=None,
                         signed: bool = False, stream: int = 0) -> None:
        """tgms_field_edt_device: n = (nx, ny, nz), d_occ uint8 with x fastest; d_values fp32 and d_d2
        int32 of the same shape (at least one); d_work of field_edt_work_size bytes.  Three launches
        (six signed), no handle scratch: capturable."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_field_edt_device(
            self._h, ctypes.byref(fld), _ptr(d_occ), float(max_dist), _lib.EDT_SIGNED if signed else 0, _ptr(d_values),
            _ptr(d_d2), _ptr(d_work), ctypes.c_void_p(stream)))

    def corridor_inflate_device(self, B: int, d_seg_offsets, d_waypoints, origin, h: float, n, d_table, max_grow: int,
                                d_box=None, d_faces=None, d_face_offsets=None, d_seg_flags=None, d_flags=None,
                                stream: int = 0) -> None:
        """tgms_corridor_inflate_batch_device: d_table of field_occupancy_device for the same grid;
        d_box [S,6] int32, d_faces [6S,4] fp64, d_face_offsets [S+1] int64, d_seg_flags [S] and d_flags
        [B] int32 (at least one).  One launch, no handle scratch: capturable."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_corridor_inflate_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), ctypes.byref(fld), _ptr(d_table), int(max_grow),
            _ptr(d_box), _ptr(d_faces), _ptr(d_face_offsets), _ptr(d_seg_flags), _ptr(d_flags),
            ctypes.c_void_p(stream)))

    def corridor_subdivide_device(self, B: int, d_seg_offsets, d_waypoints, origin, h: float, n, d_table,
                                  max_depth: int, d_seg_offsets_out, d_waypoints_out, d_totals, d_seg_times=None,
                                  d_seg_times_out=None, d_parent=None, d_seg_flags_out=None, d_flags=None,
                                  stream: int = 0) -> None:
        """tgms_corridor_subdivide_batch_device: d_table of field_occupancy_device for the same grid;
        outputs at the capacity cap = min(2^max_depth S, MAX_SEGMENTS B): d_seg_offsets_out [B+1] int32,
        d_waypoints_out [cap+B,3], d_seg_times_out [cap] (with d_seg_times, or neither), d_parent and
        d_seg_flags_out [cap] int32, d_totals [1] int64 = S', d_flags [B] int32.  Not capturable: it
        grows handle scratch with B."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_corridor_subdivide_batch_device(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), ctypes.byref(fld),
            _ptr(d_table), int(max_depth), _ptr(d_seg_offsets_out), _ptr(d_waypoints_out), _ptr(d_seg_times_out),
            _ptr(d_parent), _ptr(d_seg_flags_out), _ptr(d_totals), _ptr(d_flags), ctypes.c_void_p(stream)))


    def corridor_reroute_device(self, B: int, d_seg_offsets, d_waypoints, origin, h: float, n, d_table, margin: int,
                                max_pieces: int, d_seg_offsets_out, d_waypoints_out, d_totals, d_seg_times=None,
                                d_seg_times_out=None, d_parent=None, d_seg_flags_out=None, d_hops=None, d_flags=None,
                                stream: int = 0) -> None:
        """tgms_corridor_reroute_batch_dev: d_table of field_occupancy_device for the same grid; outputs
        at the capacity cap = min(max_pieces S, MAX_SEGMENTS B): d_seg_offsets_out [B+1] int32,
        d_waypoints_out [cap+B,3], d_seg_times_out [cap] (with d_seg_times, or neither), d_parent and
        d_seg_flags_out [cap] int32, d_hops [S] int32 per input segment, d_totals [1] int64 = S', d_flags
        [B] int32.  Not capturable: it grows handle scratch with B."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_corridor_reroute_batch_dev(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), ctypes.byref(fld),
            _ptr(d_table), int(margin), int(max_pieces), _ptr(d_seg_offsets_out), _ptr(d_waypoints_out),
            _ptr(d_seg_times_out), _ptr(d_parent), _ptr(d_seg_flags_out), _ptr(d_hops), _ptr(d_totals), _ptr(d_flags),
            ctypes.c_void_p(stream)))

    def field_nearest_free_device(self, origin, h: float, n, d_values, r_free: float, max_shift: int, d_nearest, d_work,
                                  d_dsq=None, stream: int = 0) -> None:
        """tgms_field_nearest_free_dev: n = (nx, ny, nz), d_values fp32 with x fastest; d_nearest and
        d_dsq (optional) int32 of the same shape; d_work of field_nearest_free_work_size bytes.  Three
        launches, no handle scratch: capturable."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_field_nearest_free_dev(
            self._h, ctypes.byref(fld), _ptr(d_values), float(r_free), int(max_shift), _ptr(d_nearest), _ptr(d_dsq),
            _ptr(d_work), ctypes.c_void_p(stream)))

    def waypoints_repair_device(self, B: int, d_seg_offsets, d_waypoints, origin, h: float, n, d_nearest, mode: int,
                                d_waypoints_out, d_seg_times=None, d_seg_times_out=None, d_wp_flags=None, d_shift=None,
                                d_flags=None, stream: int = 0) -> None:
        """tgms_waypoints_repair_batch_dev: d_nearest of field_nearest_free_device for the same grid;
        d_waypoints_out [S+B,3], d_seg_times_out [S] (with d_seg_times, or neither), d_wp_flags and
        d_shift [S+B] int32, d_flags [B] int32.  One launch, no handle scratch: capturable."""
        fld = _lib.Field(origin, h, n)
        self._check(self._L.tgms_waypoints_repair_batch_dev(
            self._h, int(B), _ptr(d_seg_offsets), _ptr(d_waypoints), _ptr(d_seg_times), ctypes.byref(fld),
            _ptr(d_nearest), int(mode), _ptr(d_waypoints_out), _ptr(d_seg_times_out), _ptr(d_wp_flags), _ptr(d_shift),
            _ptr(d_flags), ctypes.c_void_p(stream)))


def sample_count(total_T: float, dt: float) -> int:
    return int(_lib.load().tgms_sample_count(float(total_T), float(dt)))


def sample_offsets(seg_offsets, seg_times, dt: float) -> np.ndarray:
    so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
    T = np.ascontiguousarray(seg_times, dtype=np.float64).reshape(-1)
    B = so.shape[0] - 1
    offs = np.zeros(B + 1, dtype=np.int64)
    st = _lib.load().tgms_sample_offsets(B, _ptr(so), _ptr(T), float(dt), _ptr(offs))
    if st != _lib.OK:
        raise TgmsError(st, "tgms_sample_offsets")
    return offs


def plan_shards(seg_offsets, parts: int, method: int = _lib.METHOD_REDUCED) -> np.ndarray:
    """tgms_plan_shards (host only): [parts+1] contiguous cost-balanced trajectory bounds."""
    so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
    bounds = np.zeros(int(parts) + 1, dtype=np.int32)
    st = _lib.load().tgms_plan_shards(int(so.shape[0] - 1), _ptr(so), int(parts), int(method), _ptr(bounds))
    if st != _lib.OK:
        raise TgmsError(st, "tgms_plan_shards")
    return bounds


def multi_schedule(seg_offsets, device_count: int, method: int = _lib.METHOD_REDUCED, flags: int = 0):
    """tgms_multi_schedule (host only): the multi-GPU call's whole schedule -- shard bounds,
    per-device workspace sizes, pieces and transfers (lists of dicts, issue order)."""
    import ctypes
    L = _lib.load()
    so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
    B = int(so.shape[0] - 1)
    n = int(device_count)
    bounds = np.zeros(n + 1, dtype=np.int32)
    ws = np.zeros(n, dtype=np.int64)
    npc, nx = ctypes.c_int32(0), ctypes.c_int32(0)
    st = L.tgms_multi_schedule(n, B, _ptr(so), int(method), int(flags), _ptr(bounds), _ptr(ws), None, 0,
                               ctypes.byref(npc), None, 0, ctypes.byref(nx))
    if st not in (_lib.OK, _lib.ERR_INVALID_ARG) or (st != _lib.OK and npc.value == 0 and nx.value == 0):
        raise TgmsError(st, "tgms_multi_schedule")
    pieces = (_lib.Piece * max(1, npc.value))()
    xfers = (_lib.Xfer * max(1, nx.value))()
    st = L.tgms_multi_schedule(n, B, _ptr(so), int(method), int(flags), _ptr(bounds), _ptr(ws), pieces, npc.value,
                               ctypes.byref(npc), xfers, nx.value, ctypes.byref(nx))
    if st != _lib.OK:
        raise TgmsError(st, "tgms_multi_schedule")
    P = [{"dev": p.dev, "piece": p.piece, "lo": p.lo, "hi": p.hi, "s0": p.s0, "s1": p.s1,
          "ws_off": list(p.ws_off)} for p in pieces[: npc.value]]
    X = [{f: getattr(x, f) for f, _ in _lib.Xfer._fields_} for x in xfers[: nx.value]]
    return bounds, ws, P, X
