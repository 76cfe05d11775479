"""What the gfx950 code object says about the array mooring kernels (raft_amd/csrc/raftx_array_mooring.h), in the style of
tests/test_code_object.py (its helpers, its skip rule; no GPU needed): the instantiations a batch of single rows and shared rows
runs -- k_array_moor_line<false, false>, k_array_moor_design<false>, k_array_mean_pose<false, false> -- use 0 B of scratch.
The CHAINS / BRIDLES instantiations call the non-inlined bodies of composite lines and bridles, as k_moor_line<true> and
k_mean_pose<true> do, and have the scratch of those calls."""
import re

from tests.test_code_object import code_object, kernel_notes, pytestmark       # noqa: F401  (code_object is a fixture)

NEW_KERNELS = (r"^_Z17k_array_moor_lineILb0ELb0EE", r"^_Z19k_array_moor_designILb0EE", r"^_Z17k_array_mean_poseILb0ELb0EE")


def test_no_scratch_on_the_array_mooring_kernels(code_object):    # noqa: F811
    notes = kernel_notes(code_object)
    for pat in NEW_KERNELS:
        hit = [(n, k) for n, k in notes.items() if re.search(pat, n)]
        assert len(hit) == 1, (pat, [n for n, _ in hit])
        name, k = hit[0]
        print("%s: %s VGPRs, %s B LDS, %s B scratch" % (name, k["vgpr_count"], k["group_segment_fixed_size"], k["private_segment_fixed_size"]))
        assert int(k["private_segment_fixed_size"]) == 0, name
        assert k["uses_dynamic_stack"] == "false", name
