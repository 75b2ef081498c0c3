"""CPU: the scratch and spill budget of the corridor subdivision kernels (csrc/tgms_subdivide.hip),
read from the gfx950 code object of build/tgms_subdivide.hip.o as test_inflate_resources.py reads
k_inflate's.  k_sub_plan waits for eight-corner gathers from the occupancy table and nothing but
other wavefronts hides them, so it must keep to the registers of full occupancy.  Every kernel in
the object runs without scratch memory and without a spilled VGPR.  The VGPR counts are not fixed
here; DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_subdivide_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_subdivide")
    names = [k["name"] for k in ks]
    assert any("k_sub_plan" in n for n in names) and any("k_sub_write" in n for n in names)
    assert any("k_sub_empty" in n for n in names)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
