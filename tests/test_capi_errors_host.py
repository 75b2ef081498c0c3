"""CPU: what the host-pointer analysis and map entry points answer to bad arguments -- status and
last_error, byte for byte -- against tests/golden/capi_errors.json, which was recorded from the
library before the C-ABI unit was first split (tests/golden/make_capi_errors.py).  The
table (tests/capi_errors_cases.py) exercises every rule of every check_* function, the shared grid
rules per axis for each of their three callers, the generic rules (offsets, a NULL input, every
output NULL, a NULL handle), the refusal of every GPU-only entry point on a host handle, and
tgms_field_edt_work_size on every refused grid.  The message of a refused stream capture cannot be
reached without a GPU: tests/test_gpu_capture.py holds it."""
import json
import os

import pytest

import capi_errors_cases as CE
from trajectory_generator_ros2_amd import ERR_INVALID_ARG, OK, _lib

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_errors.json")) as f:
    WANT = CE.unpack(json.load(f))


@pytest.fixture(scope="module")
def got():
    return CE.run_all(_lib.load())


def test_the_fixture_holds_the_table_and_nothing_else(got):
    assert sorted(got) == sorted(WANT)
    assert len(WANT) > 400


@pytest.mark.parametrize("entry", list(CE.SPEC) + ["tgms_field_edt_work_size", "host handle"])
def test_status_and_message_as_recorded(got, entry):
    ids = [k for k in WANT if (k.endswith(": host handle") if entry == "host handle" else k.startswith(entry + ": "))]
    assert ids
    bad = {k: (got[k], WANT[k]) for k in ids if got[k] != WANT[k]}
    assert not bad, bad


def test_the_table_reaches_what_it_names():
    """The recorded answers themselves: every "ok" case passed, every other argument case was
    refused with a message, and the three grid callers word their count rules differently."""
    for k, (st, msg) in WANT.items():
        entry, label = k.split(": ", 1)
        if entry == "tgms_field_edt_work_size":
            assert (st > 0) == label.startswith("ok"), k
        elif label == "ok" or " ok" in label or label.startswith("empty batch"):
            assert (st, msg) == (OK, ""), k
        elif label == "handle NULL":
            assert (st, msg) == (ERR_INVALID_ARG, ""), k
        else:
            assert st != OK and msg, k
    count = {e: WANT[f"{e}: count axis2"][1] for e in CE.GRID}
    assert count["tgms_field_clearance_batch"] == count["tgms_field_edt"] != count["tgms_corridor_inflate_batch"]
    assert WANT["tgms_field_edt: n[0]=16385"][1] != WANT["tgms_field_clearance_batch: n[0]=1"][1]
