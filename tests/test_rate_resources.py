"""CPU: the register and scratch budget of the body-rate kernel (csrc/tgms_rate.hip), read from
the gfx950 code object of build/tgms_rate.hip.o as tests/test_kernel_resources.py reads the other
kernels'.  The 26 coefficients of the stationarity polynomial and the 25 slots of its ladder are
meant to be registers with compile-time indices at one wave per SIMD: every kernel in the object
must run without scratch memory, without a spilled VGPR, and within the 512 registers a lane has
there (k_rate: 308 VGPRs, 52 AGPRs)."""
from test_kernel_resources import _kernels


def test_rate_kernels_have_no_scratch_and_fit_the_register_file(tmp_path):
    ks = _kernels(tmp_path, "tgms_rate")
    assert any("k_rate" in k["name"] for k in ks)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k["agpr"] <= 512, k
