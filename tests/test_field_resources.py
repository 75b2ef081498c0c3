"""CPU: the scratch and spill budget of the distance-field clearance kernels (csrc/tgms_field.hip),
read from the gfx950 code object of build/tgms_field.hip.o as test_clearance_resources.py reads
k_clearance's.  k_field keeps a segment's 24 coefficients and its place in the interval tree in
registers and waits for gathers, so it lives on the wavefronts a SIMD can hold: every kernel in
the object runs without scratch memory and without a spilled VGPR.  The VGPR counts are not
fixed here; DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_field_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_field")
    names = [k["name"] for k in ks]
    assert any("k_field" in n and "lip" not in n for n in names)
    assert any("k_field_lip" in n and "fold" not in n for n in names) and any("k_field_lip_fold" in n for n in names)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
