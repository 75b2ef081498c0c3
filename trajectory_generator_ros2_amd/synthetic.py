"""Synthetic waypoint batches exactly as SURVEY.md §8(d) specifies them.

* seed 20251015, numpy PCG64 (``np.random.default_rng``);
* waypoints i.i.d. uniform in the reference room bounds: x, y in [-5, 5]
  (config/default.yaml:68-71), z in [0.5, 5.0] (kept above ground, within
  z_min/z_max :72-73);
* segment times T_i = clip(|w_{i+1} - w_i| / v, 0.5, 10) s with v = 1.0 m/s
  (v_line, config/default.yaml:51);
* rest-to-rest ends (every reference primitive starts and ends at rest).
"""
from __future__ import annotations

import numpy as np

SEED = 20251015
V_NOMINAL = 1.0
T_MIN, T_MAX = 0.5, 10.0


def _times(W: np.ndarray) -> np.ndarray:
    d = np.linalg.norm(np.diff(W, axis=-2), axis=-1)
    return np.clip(d / V_NOMINAL, T_MIN, T_MAX)


def uniform_batch(B: int, M: int, seed: int = SEED):
    """B trajectories of M segments: (seg_offsets [B+1], waypoints [B,M+1,3], times [B,M])."""
    rng = np.random.default_rng(seed)
    W = np.empty((B, M + 1, 3), dtype=np.float64)
    W[..., 0] = rng.uniform(-5.0, 5.0, size=(B, M + 1))
    W[..., 1] = rng.uniform(-5.0, 5.0, size=(B, M + 1))
    W[..., 2] = rng.uniform(0.5, 5.0, size=(B, M + 1))
    T = _times(W)
    so = (np.arange(B + 1, dtype=np.int64) * M).astype(np.int32)
    return so, W, T


def ragged_batch(B: int, m_lo: int = 2, m_hi: int = 16, seed: int = SEED):
    """Config 5: M_b ~ U{m_lo..m_hi}.  Returns CSR (seg_offsets, waypoints [S+B,3], times [S])."""
    rng = np.random.default_rng(seed)
    Ms = rng.integers(m_lo, m_hi + 1, size=B).astype(np.int32)
    so = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(Ms, out=so[1:])
    S = int(so[-1])
    n_w = S + B
    W = np.empty((n_w, 3), dtype=np.float64)
    W[:, 0] = rng.uniform(-5.0, 5.0, size=n_w)
    W[:, 1] = rng.uniform(-5.0, 5.0, size=n_w)
    W[:, 2] = rng.uniform(0.5, 5.0, size=n_w)
    # segment i of trajectory b joins waypoint rows so[b]+b+i and +1
    rows = np.arange(S) + np.repeat(np.arange(B), Ms)
    T = np.clip(np.linalg.norm(W[rows + 1] - W[rows], axis=1) / V_NOMINAL, T_MIN, T_MAX)
    return so.astype(np.int32), W, T


def box_field(obstacles, origin, h: float, n):
    """The exact unsigned distance to a set of axis-aligned boxes `obstacles` [K,6] = lo[3] hi[3]
    (0 inside), sampled at the nodes origin + h (i, j, k) of a grid of n = (nx, ny, nz) nodes.
    Returns float32 [nz, ny, nx], x fastest, as tgms_field_clearance_batch takes it."""
    ob = np.asarray(obstacles, dtype=np.float64).reshape(-1, 6)
    nx, ny, nz = (int(x) for x in n)
    ax = [float(origin[a]) + float(h) * np.arange(m) for a, m in enumerate((nx, ny, nz))]
    d2 = np.full((nz, ny, nx), np.inf)
    for lo_hi in ob:
        g = [np.maximum(np.maximum(lo_hi[a] - ax[a], ax[a] - lo_hi[3 + a]), 0.0) ** 2 for a in range(3)]
        np.minimum(d2, g[2][:, None, None] + g[1][None, :, None] + g[0][None, None, :], out=d2)
    return np.sqrt(d2).astype(np.float32)


def box_occupancy(obstacles, origin, h: float, n):
    """The occupancy grid of the same boxes on the same nodes: a node is occupied when it lies in a
    closed box.  Returns uint8 [nz, ny, nx], x fastest, as tgms_field_edt takes it."""
    ob = np.asarray(obstacles, dtype=np.float64).reshape(-1, 6)
    nx, ny, nz = (int(x) for x in n)
    ax = [float(origin[a]) + float(h) * np.arange(m) for a, m in enumerate((nx, ny, nz))]
    occ = np.zeros((nz, ny, nx), dtype=bool)
    for lo_hi in ob:
        g = [(ax[a] >= lo_hi[a]) & (ax[a] <= lo_hi[3 + a]) for a in range(3)]
        occ |= g[2][:, None, None] & g[1][None, :, None] & g[0][None, None, :]
    return occ.astype(np.uint8)


def box_corridor(seg_offsets, waypoints, width: float):
    """The simplest corridor of a batch: per segment the bounding box of its two waypoints grown
    by `width` on every side, as six axis-aligned faces +x -x +y -y +z -z (n[3] d, inside when
    n . p <= d).  waypoints [S+B,3] in CSR order (segment i of trajectory b joins rows
    seg_offsets[b] + b + i and + 1; a [B,M+1,3] array reshapes to it).  Returns (faces [6S,4]
    float64, face_offsets [S+1] int64) for tgms_corridor_batch."""
    so = np.asarray(seg_offsets, dtype=np.int64)
    W = np.asarray(waypoints, dtype=np.float64).reshape(-1, 3)
    S = int(so[-1])
    rows = np.arange(S) + np.repeat(np.arange(len(so) - 1), np.diff(so))
    lo = np.minimum(W[rows], W[rows + 1]) - width
    hi = np.maximum(W[rows], W[rows + 1]) + width
    faces = np.zeros((S, 6, 4), dtype=np.float64)
    for ax in range(3):
        faces[:, 2 * ax, ax], faces[:, 2 * ax, 3] = 1.0, hi[:, ax]
        faces[:, 2 * ax + 1, ax], faces[:, 2 * ax + 1, 3] = -1.0, -lo[:, ax]
    return faces.reshape(-1, 4), 6 * np.arange(S + 1, dtype=np.int64)
