"""ctypes binding of libtgms.so (the C ABI declared in include/tgms.h).

This is the Python-side twin of the binding a ROS maintainer would add (see
INTEGRATION.md).  It loads ONLY the in-tree HIP library; if that library is
missing or cannot be loaded the import fails loudly — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

from .build import LIB_TGMS

OK, ERR_INVALID_ARG, ERR_SINGULAR, ERR_NONFINITE, ERR_NO_DEVICE, ERR_DEVICE, ERR_UNSUPPORTED, ERR_SKIPPED = range(8)
METHOD_REDUCED, METHOD_DENSE_KKT, METHOD_BAND_KKT = 0, 1, 2
YAW_CONSTANT, YAW_VELOCITY = 0, 1
ABI_VERSION = 2
MAX_SEGMENTS = 16
DENSE_MAX_SEGMENTS = 10
GOAL_STRIDE = 14
EXTREMA_STRIDE = 10  # pmin[3] pmax[3] v_peak a_peak j_peak duration
FEAS_BOX, FEAS_SPEED, FEAS_ACCEL, FEAS_JERK, FEAS_NONFINITE = 1, 2, 4, 8, 16
SEP_STRIDE = 2  # d_min t_min
SEP_CLOSE, SEP_NONFINITE = 1, 16
NEAR_NONE = -1  # tgms_neighbors_batch: nobody within r_min
CLR_BAD_OBSTACLE = 32  # tgms_clearance_batch: an unusable obstacle was left out
FLD_UNRESOLVED = 64  # tgms_field_clearance_batch: the row spent max_evals; only the upper bound holds
INF_BLOCKED, INF_OUTSIDE, INF_CAPPED = 1, 2, 4  # tgms_corridor_inflate_batch, with FEAS_NONFINITE
SUB_DONE, SUB_FULL, SUB_BLOCKED, SUB_OUTSIDE = 1, 2, 4, 8  # tgms_corridor_subdivide_batch, with FEAS_NONFINITE
SUB_MAX_DEPTH = 4  # sixteenths of a leg
# tgms_corridor_reroute_batch, with FEAS_NONFINITE
RRT_DONE, RRT_FULL, RRT_BLOCKED, RRT_OUTSIDE, RRT_WINDOW, RRT_ENDS, RRT_NOPATH, RRT_LONG = 1, 2, 4, 8, 32, 64, 128, 256
RRT_WINDOW_NODES = 32768  # the largest window the re-route searches
RRT_MAX_PIECES = 8
EDT_SIGNED = 1  # tgms_field_edt mode: negative inside, zero level half a spacing outside the occupied nodes
EDT_NONE = 2**31 - 1  # the squared distance to an empty set
# tgms_waypoints_repair_batch: waypoint flags, with FEAS_NONFINITE; the mode bits; shifts use NEAR_NONE
RPR_MOVED, RPR_STUCK, RPR_KEPT, RPR_OUTSIDE = 1, 2, 4, 8
RPR_KEEP_FIRST, RPR_KEEP_LAST = 1, 2
RPR_MAX_SHIFT = 32768
THRUST_STRIDE = 6  # f_min t_fmin f_max t_fmax tilt_max t_tilt
THRUST_LOW, THRUST_HIGH, THRUST_TILT = 1, 2, 4  # with FEAS_NONFINITE
RATE_STRIDE = 2  # omega_max t_omega
RATE_HIGH = 1  # with FEAS_NONFINITE
DIL_CAPPED = 1  # tgms_dilate_batch: still infeasible at s_hi; with FEAS_NONFINITE
DIL_FLAG_MASK, DIL_EVALS_SHIFT = 0xFF, 8  # flags >> 8: evaluations of the thrust record
DIL_NONE, DIL_SPEED, DIL_ACCEL, DIL_JERK, DIL_THRUST_HIGH, DIL_THRUST_LOW, DIL_TILT = range(7)  # the active limit
RETIME_STRIDE, RETIME_REC = 4, 3  # tgms_retime_batch: seg_rec row v a j r; rec row r_max D_in D_out
RT_OVER, RT_CAPPED, RT_CHANGED = 1, 2, 4  # with FEAS_NONFINITE
RT_SEG_SHIFT = 8  # flags >> 8: the local index of the segment holding r_max
COR_STRIDE = 2  # m_max t_max
COR_MAX_FACES = 256  # faces of one segment at most
COR_OUTSIDE, COR_BAD_FACE = 1, 32  # with FEAS_NONFINITE; indices use NEAR_NONE
SPLIT_PULL, SPLIT_CHORD = 0, 1  # the inserted waypoint of tgms_corridor_split_batch
SPLIT_DONE, SPLIT_FULL, SPLIT_AT_END = 1, 2, 4  # with FEAS_NONFINITE
CUT_DONE, CUT_SNAPPED, CUT_FINISHED = 1, 2, 4  # tgms_cut_batch; with FEAS_NONFINITE

# Every symbol include/tgms.h declares (checked by tests/test_capi_symbols.py).
EXPORTS = [
    "tgms_abi_version", "tgms_status_string", "tgms_create", "tgms_create_host", "tgms_destroy", "tgms_last_error",
    "tgms_set_method", "tgms_solve_batch", "tgms_solve_uniform_device", "tgms_solve_batch_device",
    "tgms_sample_count", "tgms_sample_offsets", "tgms_sample_batch", "tgms_sample_batch_device",
    "tgms_refine_uniform_device", "tgms_refine_batch_device", "tgms_refine_loop_device", "tgms_refine_batch",
    "tgms_create_multi", "tgms_device_count", "tgms_plan_shards", "tgms_solve_batch_multi",
    "tgms_solve_batch_multi_device", "tgms_refine_loop_multi_device", "tgms_multi_schedule",
    "tgms_extrema_batch", "tgms_extrema_batch_device", "tgms_bounds_batch", "tgms_bounds_batch_device",
    "tgms_separation_batch", "tgms_separation_batch_device",
    "tgms_neighbors_batch", "tgms_neighbors_batch_device",
    "tgms_clearance_batch", "tgms_clearance_batch_device",
    "tgms_field_clearance_batch", "tgms_field_clearance_batch_device",
    "tgms_field_occupancy_device", "tgms_corridor_inflate_batch", "tgms_corridor_inflate_batch_device",
    "tgms_corridor_subdivide_batch", "tgms_corridor_subdivide_batch_device",
    "tgms_corridor_reroute_batch", "tgms_corridor_reroute_batch_dev",
    "tgms_field_edt_work_size", "tgms_field_edt_device", "tgms_field_edt",
    "tgms_field_nearest_free_work_size", "tgms_field_nearest_free_dev", "tgms_field_nearest_free",
    "tgms_waypoints_repair_batch_dev", "tgms_waypoints_repair_batch",
    "tgms_thrust_batch", "tgms_thrust_batch_device",
    "tgms_rate_batch", "tgms_rate_batch_device",
    "tgms_dilate_batch", "tgms_dilate_batch_device",
    "tgms_retime_batch", "tgms_retime_batch_dev",
    "tgms_corridor_batch", "tgms_corridor_batch_device",
    "tgms_corridor_split_batch", "tgms_corridor_split_batch_device",
    "tgms_cut_batch", "tgms_cut_batch_device",
]

SCHED_REFINE, SCHED_END_DERIVS, SCHED_COEFFS, SCHED_STATUS, SCHED_COST, SCHED_SELF_GATHER = 1, 2, 4, 8, 16, 32


class Piece(ctypes.Structure):
    """tgms_piece (include/tgms.h): one piece of one device's shard."""
    _fields_ = [("dev", ctypes.c_int32), ("piece", ctypes.c_int32), ("lo", ctypes.c_int32), ("hi", ctypes.c_int32),
                ("s0", ctypes.c_int64), ("s1", ctypes.c_int64), ("ws_off", ctypes.c_int64 * 11)]


class Xfer(ctypes.Structure):
    """tgms_xfer (include/tgms.h): one ncclSend/ncclRecv pair of the multi-GPU schedule."""
    _fields_ = [("dev", ctypes.c_int32), ("piece", ctypes.c_int32), ("gather", ctypes.c_int32),
                ("array", ctypes.c_int32), ("batch_elem", ctypes.c_int64), ("ws_byte", ctypes.c_int64),
                ("count", ctypes.c_int64), ("elem_bytes", ctypes.c_int32), ("group", ctypes.c_int32)]


class Limits(ctypes.Structure):
    """tgms_limits (include/tgms.h): the box and the speed / acceleration / jerk limits of a
    feasibility check.  The default checks nothing (+-inf everywhere)."""
    _fields_ = [("pmin", ctypes.c_double * 3), ("pmax", ctypes.c_double * 3), ("v_max", ctypes.c_double),
                ("a_max", ctypes.c_double), ("j_max", ctypes.c_double)]

    def __init__(self, pmin=None, pmax=None, v_max=float("inf"), a_max=float("inf"), j_max=float("inf")):
        super().__init__()
        self.pmin[:] = [float(x) for x in (pmin if pmin is not None else [float("-inf")] * 3)]
        self.pmax[:] = [float(x) for x in (pmax if pmax is not None else [float("inf")] * 3)]
        self.v_max, self.a_max, self.j_max = float(v_max), float(a_max), float(j_max)


class ThrustLimits(ctypes.Structure):
    """tgms_thrust_limits (include/tgms.h): the least and the largest mass-normalised thrust
    (m/s^2) and the largest tilt (rad) of a thrust check.  The default checks nothing."""
    _fields_ = [("f_min", ctypes.c_double), ("f_max", ctypes.c_double), ("tilt_max", ctypes.c_double)]

    def __init__(self, f_min=float("-inf"), f_max=float("inf"), tilt_max=float("inf")):
        super().__init__()
        self.f_min, self.f_max, self.tilt_max = float(f_min), float(f_max), float(tilt_max)


class Field(ctypes.Structure):
    """tgms_field (include/tgms.h): the grid of a distance field: the position of node (0,0,0), the
    node spacing and the nodes per axis (x fastest in the values)."""
    _fields_ = [("origin", ctypes.c_double * 3), ("h", ctypes.c_double), ("n", ctypes.c_int32 * 3)]

    def __init__(self, origin=(0.0, 0.0, 0.0), h=1.0, n=(2, 2, 2)):
        super().__init__()
        self.origin[:] = [float(x) for x in origin]
        self.h = float(h)
        self.n[:] = [int(x) for x in n]


_lib = None


class TgmsError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        self.status = status
        super().__init__(f"{status_string(status)}: {msg}" if msg else status_string(status))


def load(path: str = ""):
    """Load libtgms.so.  Raises if it is absent: build it with __graft_entry__.build().
    TGMS_LIB may name an alternative build of the same ABI (kernel experiments)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("TGMS_LIB", "") or LIB_TGMS
    if not os.path.exists(path):
        raise ImportError(f"libtgms.so not built at {path}; run `python -c 'import __graft_entry__ as g; g.build()'`")
    # PyTorch-ROCm ships its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Load
    # torch first so libtgms binds to the HIP runtime instance torch uses: one runtime
    # per process, so device pointers and streams are shared between the two.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    L.tgms_abi_version.restype = ctypes.c_int
    L.tgms_status_string.argtypes = [ctypes.c_int]
    L.tgms_status_string.restype = ctypes.c_char_p
    L.tgms_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    L.tgms_create.restype = ctypes.c_int
    L.tgms_create_host.argtypes = [ctypes.POINTER(vp)]
    L.tgms_create_host.restype = ctypes.c_int
    L.tgms_destroy.argtypes = [vp]
    L.tgms_destroy.restype = None
    L.tgms_last_error.argtypes = [vp]
    L.tgms_last_error.restype = ctypes.c_char_p
    L.tgms_set_method.argtypes = [vp, ctypes.c_int]
    L.tgms_set_method.restype = ctypes.c_int
    L.tgms_solve_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.tgms_solve_batch.restype = ctypes.c_int
    L.tgms_solve_uniform_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.tgms_solve_uniform_device.restype = ctypes.c_int
    L.tgms_solve_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tgms_solve_batch_device.restype = ctypes.c_int
    L.tgms_sample_count.argtypes = [dbl, dbl]
    L.tgms_sample_count.restype = i64
    L.tgms_sample_offsets.argtypes = [i32, vp, vp, dbl, vp]
    L.tgms_sample_offsets.restype = ctypes.c_int
    L.tgms_sample_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, ctypes.c_int, dbl, vp, vp]
    L.tgms_sample_batch.restype = ctypes.c_int
    L.tgms_sample_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, ctypes.c_int, dbl, vp, vp, vp]
    L.tgms_sample_batch_device.restype = ctypes.c_int
    L.tgms_refine_uniform_device.argtypes = [vp, i32, i32, vp, vp, vp, dbl, dbl, vp, vp, vp, vp]
    L.tgms_refine_uniform_device.restype = ctypes.c_int
    L.tgms_refine_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, dbl, vp, vp, vp, vp]
    L.tgms_refine_batch_device.restype = ctypes.c_int
    L.tgms_refine_loop_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, dbl, i32, vp, vp, vp, vp]
    L.tgms_refine_loop_device.restype = ctypes.c_int
    L.tgms_refine_batch.argtypes = [vp, i32, vp, vp, vp, vp, dbl, dbl, i32, vp, vp, vp]
    L.tgms_refine_batch.restype = ctypes.c_int
    L.tgms_create_multi.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    L.tgms_create_multi.restype = ctypes.c_int
    L.tgms_device_count.argtypes = [vp]
    L.tgms_device_count.restype = ctypes.c_int
    L.tgms_plan_shards.argtypes = [i32, vp, i32, ctypes.c_int, vp]
    L.tgms_plan_shards.restype = ctypes.c_int
    L.tgms_solve_batch_multi.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.tgms_solve_batch_multi.restype = ctypes.c_int
    L.tgms_solve_batch_multi_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tgms_solve_batch_multi_device.restype = ctypes.c_int
    L.tgms_refine_loop_multi_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, dbl, i32, vp, vp, vp, vp]
    L.tgms_refine_loop_multi_device.restype = ctypes.c_int
    L.tgms_multi_schedule.argtypes = [i32, i32, vp, ctypes.c_int, i32, vp, vp, vp, i32, vp, vp, i32, vp]
    L.tgms_multi_schedule.restype = ctypes.c_int
    L.tgms_extrema_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, ctypes.POINTER(Limits), vp, vp, vp]
    L.tgms_extrema_batch_device.restype = ctypes.c_int
    L.tgms_extrema_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, ctypes.POINTER(Limits), vp, vp]
    L.tgms_extrema_batch.restype = ctypes.c_int
    L.tgms_bounds_batch_device.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Limits), vp, vp, vp]
    L.tgms_bounds_batch_device.restype = ctypes.c_int
    L.tgms_bounds_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Limits), vp, vp]
    L.tgms_bounds_batch.restype = ctypes.c_int
    L.tgms_separation_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp, dbl, vp, vp, vp]
    L.tgms_separation_batch_device.restype = ctypes.c_int
    L.tgms_separation_batch.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp, dbl, vp, vp]
    L.tgms_separation_batch.restype = ctypes.c_int
    L.tgms_neighbors_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, vp, vp, vp, vp, vp, vp]
    L.tgms_neighbors_batch_device.restype = ctypes.c_int
    L.tgms_neighbors_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl, vp, vp, vp, vp, vp]
    L.tgms_neighbors_batch.restype = ctypes.c_int
    L.tgms_clearance_batch_device.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, dbl, vp, vp, vp, vp, vp, vp]
    L.tgms_clearance_batch_device.restype = ctypes.c_int
    L.tgms_clearance_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, dbl, vp, vp, vp, vp, vp]
    L.tgms_clearance_batch.restype = ctypes.c_int
    L.tgms_field_clearance_batch_device.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, dbl, dbl, dbl, i32,
                                                    vp, vp, vp, vp]
    L.tgms_field_clearance_batch_device.restype = ctypes.c_int
    L.tgms_field_clearance_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, dbl, dbl, dbl, i32,
                                             vp, vp, vp]
    L.tgms_field_clearance_batch.restype = ctypes.c_int
    L.tgms_field_occupancy_device.argtypes = [vp, ctypes.POINTER(Field), vp, dbl, vp, vp]
    L.tgms_field_occupancy_device.restype = ctypes.c_int
    L.tgms_corridor_inflate_batch_device.argtypes = [vp, i32, vp, vp, ctypes.POINTER(Field), vp, i32, vp, vp, vp, vp, vp,
                                                     vp]
    L.tgms_corridor_inflate_batch_device.restype = ctypes.c_int
    L.tgms_corridor_inflate_batch.argtypes = [vp, i32, vp, vp, ctypes.POINTER(Field), vp, dbl, i32, vp, vp, vp, vp, vp]
    L.tgms_corridor_inflate_batch.restype = ctypes.c_int
    L.tgms_corridor_subdivide_batch_device.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, i32, vp, vp, vp,
                                                       vp, vp, vp, vp, vp]
    L.tgms_corridor_subdivide_batch_device.restype = ctypes.c_int
    L.tgms_corridor_subdivide_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, dbl, i32, vp, vp, vp, vp,
                                                vp, vp, vp]
    L.tgms_corridor_subdivide_batch.restype = ctypes.c_int
    L.tgms_corridor_reroute_batch_dev.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, i32, i32, vp, vp, vp,
                                                  vp, vp, vp, vp, vp, vp]
    L.tgms_corridor_reroute_batch_dev.restype = ctypes.c_int
    L.tgms_corridor_reroute_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, dbl, i32, i32, vp, vp, vp,
                                              vp, vp, vp, vp, vp]
    L.tgms_corridor_reroute_batch.restype = ctypes.c_int
    L.tgms_field_edt_work_size.argtypes = [ctypes.POINTER(Field), i32]
    L.tgms_field_edt_work_size.restype = ctypes.c_size_t
    L.tgms_field_edt_device.argtypes = [vp, ctypes.POINTER(Field), vp, dbl, i32, vp, vp, vp, vp]
    L.tgms_field_edt_device.restype = ctypes.c_int
    L.tgms_field_edt.argtypes = [vp, ctypes.POINTER(Field), vp, dbl, i32, vp, vp]
    L.tgms_field_edt.restype = ctypes.c_int
    L.tgms_field_nearest_free_work_size.argtypes = [ctypes.POINTER(Field)]
    L.tgms_field_nearest_free_work_size.restype = ctypes.c_size_t
    L.tgms_field_nearest_free_dev.argtypes = [vp, ctypes.POINTER(Field), vp, dbl, i32, vp, vp, vp, vp]
    L.tgms_field_nearest_free_dev.restype = ctypes.c_int
    L.tgms_field_nearest_free.argtypes = [vp, ctypes.POINTER(Field), vp, dbl, i32, vp, vp]
    L.tgms_field_nearest_free.restype = ctypes.c_int
    L.tgms_waypoints_repair_batch_dev.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, i32, vp, vp, vp, vp,
                                                  vp, vp]
    L.tgms_waypoints_repair_batch_dev.restype = ctypes.c_int
    L.tgms_waypoints_repair_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Field), vp, dbl, i32, i32, vp, vp, vp,
                                              vp, vp]
    L.tgms_waypoints_repair_batch.restype = ctypes.c_int
    L.tgms_thrust_batch_device.argtypes = [vp, i32, vp, vp, vp, dbl, ctypes.POINTER(ThrustLimits), vp, vp, vp]
    L.tgms_thrust_batch_device.restype = ctypes.c_int
    L.tgms_thrust_batch.argtypes = [vp, i32, vp, vp, vp, dbl, ctypes.POINTER(ThrustLimits), vp, vp]
    L.tgms_thrust_batch.restype = ctypes.c_int
    L.tgms_rate_batch_device.argtypes = [vp, i32, vp, vp, vp, dbl, dbl, vp, vp, vp, vp]
    L.tgms_rate_batch_device.restype = ctypes.c_int
    L.tgms_rate_batch.argtypes = [vp, i32, vp, vp, vp, dbl, dbl, vp, vp, vp]
    L.tgms_rate_batch.restype = ctypes.c_int
    L.tgms_dilate_batch_device.argtypes = [vp, i32, vp, vp, vp, dbl, ctypes.POINTER(Limits),
                                           ctypes.POINTER(ThrustLimits), dbl, dbl, vp, vp, vp, vp, vp, vp]
    L.tgms_dilate_batch_device.restype = ctypes.c_int
    L.tgms_dilate_batch.argtypes = [vp, i32, vp, vp, vp, dbl, ctypes.POINTER(Limits), ctypes.POINTER(ThrustLimits),
                                    dbl, dbl, vp, vp, vp, vp, vp]
    L.tgms_dilate_batch.restype = ctypes.c_int
    L.tgms_retime_batch_dev.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Limits), dbl, dbl, vp, vp, vp, vp, vp]
    L.tgms_retime_batch_dev.restype = ctypes.c_int
    L.tgms_retime_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(Limits), dbl, dbl, vp, vp, vp, vp]
    L.tgms_retime_batch.restype = ctypes.c_int
    L.tgms_corridor_batch_device.argtypes = [vp, i32, vp, vp, vp, ctypes.c_int64, vp, vp, dbl, vp, vp, vp, vp, vp, vp]
    L.tgms_corridor_batch_device.restype = ctypes.c_int
    L.tgms_corridor_batch.argtypes = [vp, i32, vp, vp, vp, ctypes.c_int64, vp, vp, dbl, vp, vp, vp, vp, vp]
    L.tgms_corridor_batch.restype = ctypes.c_int
    L.tgms_corridor_split_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, dbl,
                                                   ctypes.c_int, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tgms_corridor_split_batch_device.restype = ctypes.c_int
    L.tgms_corridor_split_batch.argtypes = [vp, i32, vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, dbl,
                                            ctypes.c_int, dbl, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tgms_corridor_split_batch.restype = ctypes.c_int
    L.tgms_cut_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tgms_cut_batch_device.restype = ctypes.c_int
    L.tgms_cut_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tgms_cut_batch.restype = ctypes.c_int
    if L.tgms_abi_version() != ABI_VERSION:
        raise ImportError(f"libtgms ABI {L.tgms_abi_version()} != {ABI_VERSION}")
    _lib = L
    return L


def status_string(status: int) -> str:
    return load().tgms_status_string(int(status)).decode()
