"""CPU: the scratch and spill budget of the separation kernel (csrc/tgms_separation.hip), read
from the gfx950 code object of build/tgms_separation.hip.o as tests/test_kernel_resources.py
reads the other kernels'.  The kernel's root list (13 doubles per lane) and its polynomial
coefficients are meant to be registers with compile-time indices: every kernel in the object
must run without scratch memory and without a spilled VGPR, the project's standing condition
for all kernels.  The VGPR count itself is not fixed here; DESIGN.md records the figure."""
from test_kernel_resources import _kernels


def test_separation_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_separation")
    assert any("k_separation" in k["name"] for k in ks)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
