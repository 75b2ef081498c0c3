"""CPU: the scratch and spill budget of the neighbour search kernels (csrc/tgms_neighbors.hip),
read from the gfx950 code object of build/tgms_neighbors.hip.o as test_separation_resources.py
reads k_separation's.  k_neighbors runs separation::interval_item inside its sweep, so the
item's root list and coefficients must stay registers there too: every kernel in the object
runs without scratch memory and without a spilled VGPR.  The VGPR counts are not fixed here;
DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_neighbors_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_neighbors")
    assert any("k_neighbors" in k["name"] for k in ks) and any("k_neighbor_boxes" in k["name"] for k in ks)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
