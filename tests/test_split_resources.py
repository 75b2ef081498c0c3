"""CPU: the register and scratch budget of the corridor split's kernels
(csrc/tgms_corridor_split.hip), read from the gfx950 code object of build/tgms_corridor_split.hip.o
as tests/test_kernel_resources.py reads the other kernels'.  The plan, the three kernels of the
scan and the write keep their coefficients and face rows in registers with compile-time indices:
every kernel in the object must run without scratch memory, without a spilled VGPR, and within
256 VGPRs."""
from test_kernel_resources import _kernels


def test_split_kernels_have_no_scratch_and_fit_the_register_file(tmp_path):
    ks = _kernels(tmp_path, "tgms_corridor_split")
    for name in ("k_split_plan", "k_scan_sums", "k_scan_top", "k_scan_add", "k_split_write"):
        assert any(name in k["name"] for k in ks), name
    for k in ks:
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k["agpr"] <= 256, k
