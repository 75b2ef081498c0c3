"""CPU: the register and scratch budget of the time-dilation kernel (csrc/tgms_dilate.hip), read
from the gfx950 code object of build/tgms_dilate.hip.o as tests/test_thrust_resources.py reads
k_thrust's.  It runs the three norm ladders and the two thrust ladders one after the other, with
the search's state in LDS: every kernel in the object must run without scratch memory, without a
spilled VGPR, and within 256 VGPRs."""
from test_kernel_resources import _kernels


def test_dilate_kernels_have_no_scratch_and_fit_the_register_file(tmp_path):
    ks = _kernels(tmp_path, "tgms_dilate")
    assert any("k_dilate" in k["name"] for k in ks)
    for k in ks:
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k["agpr"] <= 256, k
