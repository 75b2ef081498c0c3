"""CPU: the register and scratch budget of the replan cut's kernels (csrc/tgms_cut.hip), read from
the gfx950 code object of build/tgms_cut.hip.o as tests/test_kernel_resources.py reads the other
kernels'.  The plan and the write keep the one shifted row per trajectory in registers with
compile-time indices: every kernel in the object must run without scratch memory, without a
spilled VGPR, and within 256 VGPRs.  (The three kernels of the scan are the split's, launched from
tgms_corridor_split.hip.o, which test_split_resources.py reads.)"""
from test_kernel_resources import _kernels


def test_cut_kernels_have_no_scratch_and_fit_the_register_file(tmp_path):
    ks = _kernels(tmp_path, "tgms_cut")
    for name in ("k_cut_plan", "k_cut_write", "k_cut_empty"):
        assert any(name in k["name"] for k in ks), name
    for k in ks:
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k["agpr"] <= 256, k
