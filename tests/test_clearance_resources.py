"""CPU: the scratch and spill budget of the obstacle clearance kernels (csrc/tgms_clearance.hip),
read from the gfx950 code object of build/tgms_clearance.hip.o as test_neighbors_resources.py
reads k_neighbors'.  k_clearance runs clearance::combo_item, a degree-13 ladder, inside its
sweep, so the item's root list and coefficients must stay registers there: every kernel in the
object runs without scratch memory and without a spilled VGPR.  The VGPR counts are not fixed
here; DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_clearance_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_clearance")
    names = [k["name"] for k in ks]
    assert any("k_clearance_boxes" in n for n in names) and any("k_clearance" in n and "boxes" not in n for n in names)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
