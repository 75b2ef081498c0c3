"""CPU: the register and scratch budget of the feasibility-check kernel (csrc/tgms_extrema.hip),
read from the gfx950 code object of build/tgms_extrema.hip.o as tests/test_kernel_resources.py
reads the other kernels'.  The kernel keeps one segment's 78 derivative-form coefficients and
up to four samples' chains in registers: it must do so without scratch memory, without a
spilled VGPR, and within the 256 VGPRs that leave two wavefronts per SIMD resident."""
from test_kernel_resources import _kernels


def test_extrema_kernel_has_no_scratch_and_fits_two_waves(tmp_path):
    ks = [k for k in _kernels(tmp_path, "tgms_extrema") if "k_extrema" in k["name"]]
    assert len(ks) == 1
    k = ks[0]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] + k["agpr"] <= 256, k
