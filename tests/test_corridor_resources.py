"""CPU: the register and scratch budget of the corridor kernel (csrc/tgms_corridor.hip), read
from the gfx950 code object of build/tgms_corridor.hip.o as tests/test_kernel_resources.py reads
the other kernels'.  The root list of its ladder (6 doubles per lane) and the projected and axis
coefficients are meant to be registers with compile-time indices: every kernel in the object
must run without scratch memory, without a spilled VGPR, and within 256 VGPRs."""
from test_kernel_resources import _kernels


def test_corridor_kernels_have_no_scratch_and_fit_the_register_file(tmp_path):
    ks = _kernels(tmp_path, "tgms_corridor")
    assert any("k_corridor" in k["name"] for k in ks)
    for k in ks:
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k["agpr"] <= 256, k
