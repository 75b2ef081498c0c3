"""CPU: the scratch and spill budget of the distance-field kernels (csrc/tgms_edt.hip), read from
the gfx950 code object of build/tgms_edt.hip.o as test_inflate_resources.py reads the inflation's.
The row pass and both line passes are in the object, and every kernel in it runs without scratch
memory and without a spilled VGPR.  The VGPR counts are not fixed here; DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_edt_kernels_have_no_scratch_and_no_spill(tmp_path):
    from trajectory_generator_ros2_amd.build import HIP_SOURCES
    assert "tgms_edt.hip" in HIP_SOURCES  # the build makes the object read below
    ks = _kernels(tmp_path, "tgms_edt")
    names = [k["name"] for k in ks]
    assert any("k_edt_rows" in n for n in names)
    assert any("k_edt_linesILb0" in n for n in names) and any("k_edt_linesILb1" in n for n in names)
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
