"""What the gfx950 code object says about the array eigen kernels (raft_amd/csrc/raftx_array_modal.h), in the style of
tests/test_array_mooring_code_object.py (the helpers and the skip rule of tests/test_code_object.py; no GPU needed): every
instantiation of k_array_modal -- N = 6, 12, 18, 24, 30, 36 -- and the assemble kernel use 0 B of scratch and no dynamic
stack, and the LDS of k_array_modal<N> is H | Z | X at a pitch of N + 1 doubles, 3 N doubles of vectors and the claim."""
import re

from tests.test_code_object import code_object, kernel_notes, pytestmark       # noqa: F401  (code_object is a fixture)

SIZES = (6, 12, 18, 24, 30, 36)


def test_no_scratch_on_the_array_modal_kernels(code_object):    # noqa: F811
    notes = kernel_notes(code_object)
    pats = [(r"^_Z13k_array_modalILi%dEE" % n, 8 * (3 * n * (n + 1) + 3 * n + (n + 1) // 2)) for n in SIZES]
    pats.append((r"^_Z22k_array_modal_assemble", 0))
    for pat, lds in pats:
        hit = [(n, k) for n, k in notes.items() if re.search(pat, n)]
        assert len(hit) == 1, (pat, [n for n, _ in hit])
        name, k = hit[0]
        print("%s: %s VGPRs, %s B LDS, %s B scratch" % (name, k["vgpr_count"], k["group_segment_fixed_size"], k["private_segment_fixed_size"]))
        assert int(k["private_segment_fixed_size"]) == 0, name
        assert k["uses_dynamic_stack"] == "false", name
        assert int(k["group_segment_fixed_size"]) == lds, name
    assert len([n for n in notes if re.search(r"^_Z13k_array_modalILi", n)]) == len(SIZES)
