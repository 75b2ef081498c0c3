"""CPU: the scratch and spill budget of the corridor re-route kernels (csrc/tgms_reroute.hip), read
from the gfx950 code object of build/tgms_reroute.hip.o as test_subdivide_resources.py reads the
subdivision's.  The search kernel keeps a window's distances in LDS and must not add private memory
to that; every kernel in the object runs without scratch memory and without a spilled VGPR.  The
VGPR and LDS counts are not fixed here; DESIGN.md records them."""
from test_kernel_resources import _kernels


def test_reroute_kernels_have_no_scratch_and_no_spill(tmp_path):
    ks = _kernels(tmp_path, "tgms_reroute")
    names = [k["name"] for k in ks]
    for want in ("k_rrt_classify", "k_rrt_search", "k_rrt_count", "k_rrt_write", "k_rrt_empty"):
        assert any(want in n for n in names), want
    for k in ks:
        print(k)
        assert k["private_segment_fixed_size"] == 0, k
        assert k["vgpr_spill_count"] == 0, k
