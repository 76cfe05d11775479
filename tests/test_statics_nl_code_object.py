"""What the gfx950 code object says about k_mean_pose_nl (raft_amd/csrc/raftx_statics.h), in the style of
tests/test_array_modal_code_object.py (the helpers and the skip rule of tests/test_code_object.py; no GPU needed): the six
instantiations -- rows in memory | rows of the program, times plain lines | chains | bridles -- exist, none has a dynamic
stack, the only LDS is the 256 B behind __syncthreads_or, and each one's scratch is what the device functions it reuses
bring with them: none for rows in memory with plain lines, the member pass's for rows of the program, k_mean_pose's for
chains and bridles."""
import re

from tests.test_code_object import code_object, kernel_notes, pytestmark       # noqa: F401  (code_object is a fixture)


def _one(notes, pat):
    hit = [(n, k) for n, k in notes.items() if re.search(pat, n)]
    assert len(hit) == 1, (pat, [n for n, _ in hit])
    return hit[0]


def test_the_six_instantiations(code_object):                    # noqa: F811
    notes = kernel_notes(code_object)
    scratch = {}
    for rows in ("13GeomRowsPlain", "12GeomRowsProg"):
        for lines in ("Lb0ELb0E", "Lb1ELb0E", "Lb1ELb1E"):
            name, k = _one(notes, r"^_Z14k_mean_pose_nlI%s%sE" % (rows, lines))
            print("%s: %s VGPRs, %s AGPRs, %s B LDS, %s B scratch" % (name, k["vgpr_count"], k.get("agpr_count"), k["group_segment_fixed_size"],
                                                                     k["private_segment_fixed_size"]))
            assert k["uses_dynamic_stack"] == "false", name
            assert int(k["group_segment_fixed_size"]) == 256, name
            scratch[(rows, lines)] = int(k["private_segment_fixed_size"])
    assert scratch[("13GeomRowsPlain", "Lb0ELb0E")] == 0
    # no more than the line code's own scratch (k_mean_pose of the same line kind) and the member pass's (k_geom_member)
    member = int(_one(notes, r"^_Z13k_geom_member8GeomArgs")[1]["private_segment_fixed_size"])
    for lines, pat in (("Lb0ELb0E", r"^_Z11k_mean_poseILb0ELb0EE"), ("Lb1ELb0E", r"^_Z11k_mean_poseILb1ELb0EE"), ("Lb1ELb1E", r"^_Z11k_mean_poseILb1ELb1EE")):
        own = int(_one(notes, pat)[1]["private_segment_fixed_size"])
        assert scratch[("13GeomRowsPlain", lines)] <= own + member, (lines, scratch, own, member)
        assert scratch[("12GeomRowsProg", lines)] <= own + member, (lines, scratch, own, member)
