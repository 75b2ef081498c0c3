"""CPU: the register, scratch and workgroup budget of the re-timing kernel (csrc/tgms_retime.hip),
read from the gfx950 code objects of the build as tests/test_bounds_resources.py reads k_bounds'.
k_retime runs k_bounds' three norm ladders without its position items: no scratch memory, no
spilled VGPR, one wavefront per workgroup, and no more VGPRs than k_bounds has in the same build."""
import re
import subprocess

from test_kernel_resources import LLVM, _kernels


def _workgroup_sizes(tmp_path, src):
    """{kernel name: .max_flat_workgroup_size} of the code object _kernels() left in tmp_path."""
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", str(tmp_path / (src + ".co"))], check=True,
                           capture_output=True, text=True).stdout
    return dict(zip(re.findall(r"^    \.name:\s+(\S+)", notes, re.M),
                    (int(x) for x in re.findall(r"^    \.max_flat_workgroup_size:\s+(\d+)", notes, re.M))))


def test_retime_kernel_has_no_scratch_one_wave_and_fits_k_bounds(tmp_path):
    ks = [k for k in _kernels(tmp_path, "tgms_retime") if "k_retime" in k["name"]]
    kb = [k for k in _kernels(tmp_path, "tgms_bounds") if "k_bounds" in k["name"]]
    assert len(ks) == 1 and len(kb) == 1
    k = ks[0]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] + k["agpr"] <= kb[0]["vgpr_count"] + kb[0]["agpr"], (k, kb[0])
    assert _workgroup_sizes(tmp_path, "tgms_retime")[k["name"]] == 64
