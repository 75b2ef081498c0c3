"""CPU: the scratch and spill budget of the waypoint repair kernels (csrc/tgms_repair.hip), read from
the gfx950 code object of build/tgms_repair.hip.o as test_reroute_resources.py reads the re-route's.
Every kernel in the object runs without scratch memory and without a spilled VGPR.  The VGPR and
LDS counts are not fixed here; DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_repair_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_repair")
    names = [k["name"] for k in ks]
    for want in ("k_near_rows", "k_near_lines", "k_repair"):
        assert any(want in n for n in names), want
    assert sum("k_near_lines" in n for n in names) == 2  # the y pass and the z pass
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
