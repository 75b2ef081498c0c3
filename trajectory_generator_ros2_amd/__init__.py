"""trajectory_generator_ros2_amd — MI355X-native batched minimum-snap solver.

The product is ``lib/libtgms.so`` (HIP kernels for gfx950 behind the C ABI in
``include/tgms.h``) plus the C++ ``MinSnap`` primitive in ``host/`` that plugs it
behind the reference's ``Trajectory`` interface.  This Python package only
marshals buffers for tests, the benchmark and multi-GPU sharding.
"""
from ._lib import (DIL_ACCEL, DIL_CAPPED, DIL_EVALS_SHIFT, DIL_FLAG_MASK, DIL_JERK, DIL_NONE, DIL_SPEED, DIL_THRUST_HIGH,
                   DIL_THRUST_LOW, DIL_TILT)
from ._lib import CUT_DONE, CUT_FINISHED, CUT_SNAPPED
from ._lib import RATE_HIGH, RATE_STRIDE
from ._lib import FLD_UNRESOLVED, Field
from ._lib import INF_BLOCKED, INF_CAPPED, INF_OUTSIDE
from ._lib import EDT_NONE, EDT_SIGNED
from ._lib import SUB_BLOCKED, SUB_DONE, SUB_FULL, SUB_MAX_DEPTH, SUB_OUTSIDE
from ._lib import (CLR_BAD_OBSTACLE, COR_BAD_FACE, COR_MAX_FACES, COR_OUTSIDE, COR_STRIDE, ERR_DEVICE, ERR_INVALID_ARG,
                   ERR_NO_DEVICE, ERR_NONFINITE, ERR_SINGULAR, ERR_SKIPPED,
                   ERR_UNSUPPORTED, EXTREMA_STRIDE, FEAS_ACCEL, FEAS_BOX, FEAS_JERK, FEAS_NONFINITE, FEAS_SPEED,
                   METHOD_BAND_KKT, METHOD_DENSE_KKT, METHOD_REDUCED, NEAR_NONE, OK, SEP_CLOSE, SEP_NONFINITE, SEP_STRIDE,
                   SPLIT_AT_END, SPLIT_CHORD, SPLIT_DONE, SPLIT_FULL, SPLIT_PULL, THRUST_HIGH, THRUST_LOW, THRUST_STRIDE,
                   THRUST_TILT, YAW_CONSTANT, YAW_VELOCITY, Limits, TgmsError,
                   ThrustLimits)

__all__ = [
    "OK", "ERR_INVALID_ARG", "ERR_SINGULAR", "ERR_NONFINITE", "ERR_NO_DEVICE", "ERR_DEVICE",
    "ERR_UNSUPPORTED", "ERR_SKIPPED", "METHOD_REDUCED", "METHOD_DENSE_KKT", "METHOD_BAND_KKT", "YAW_CONSTANT", "YAW_VELOCITY",
    "EXTREMA_STRIDE", "FEAS_BOX", "FEAS_SPEED", "FEAS_ACCEL", "FEAS_JERK", "FEAS_NONFINITE", "Limits",
    "SEP_STRIDE", "SEP_CLOSE", "SEP_NONFINITE", "NEAR_NONE", "CLR_BAD_OBSTACLE", "TgmsError",
    "THRUST_STRIDE", "THRUST_LOW", "THRUST_HIGH", "THRUST_TILT", "ThrustLimits",
    "RATE_STRIDE", "RATE_HIGH",
    "DIL_CAPPED", "DIL_FLAG_MASK", "DIL_EVALS_SHIFT", "DIL_NONE", "DIL_SPEED", "DIL_ACCEL", "DIL_JERK",
    "DIL_THRUST_HIGH", "DIL_THRUST_LOW", "DIL_TILT",
    "COR_STRIDE", "COR_MAX_FACES", "COR_OUTSIDE", "COR_BAD_FACE",
    "SPLIT_PULL", "SPLIT_CHORD", "SPLIT_DONE", "SPLIT_FULL", "SPLIT_AT_END",
    "CUT_DONE", "CUT_SNAPPED", "CUT_FINISHED",
    "FLD_UNRESOLVED", "Field",
    "INF_BLOCKED", "INF_OUTSIDE", "INF_CAPPED",
    "SUB_DONE", "SUB_FULL", "SUB_BLOCKED", "SUB_OUTSIDE", "SUB_MAX_DEPTH",
    "EDT_SIGNED", "EDT_NONE",
]
