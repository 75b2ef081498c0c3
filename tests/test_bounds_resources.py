"""CPU: the register and scratch budget of the continuous-bounds kernel (csrc/tgms_bounds.hip),
read from the gfx950 code object of build/tgms_bounds.hip.o as tests/test_kernel_resources.py
reads the other kernels'.  The kernel's root lists (up to 11 doubles per lane) and polynomial
coefficients are meant to be registers with compile-time indices: every kernel in the object
must run without scratch memory, without a spilled VGPR, and within the 256 VGPRs that leave
two wavefronts per SIMD resident."""
from test_kernel_resources import _kernels


def test_bounds_kernels_have_no_scratch_and_fit_two_waves(tmp_path):
    ks = _kernels(tmp_path, "tgms_bounds")
    assert any("k_bounds" in k["name"] for k in ks)
    for k in ks:
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k["agpr"] <= 256, k
