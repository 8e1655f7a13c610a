"""k_compare_fast_own is a COPY of k_compare_fast's body (the shared __device__ template changed the code
generation of the existing kernels).  A fix to one has to be made in the other by hand; this test keeps the two from
drifting: outside the signature and the hunks marked OWN the two bodies are the same text, line for line."""
import difflib
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bioem_amd", "csrc")


def kernel_body(path, name):
    """the lines of `template <...> __global__ ... void name(...) { ... }`, up to the closing brace in column 0"""
    lines = open(os.path.join(CSRC, path)).read().split("\n")
    sig = [i for i, l in enumerate(lines) if re.search(r"\bvoid %s\(" % name, l) and "__global__" in l]
    assert len(sig) == 1, (path, name, sig)
    end = next(i for i in range(sig[0], len(lines)) if lines[i] == "}")
    return lines[sig[0]:end + 1]


def test_own_body_is_the_plain_body_outside_the_marked_lines():
    plain = kernel_body("compare_fast.hpp", "k_compare_fast")
    own = kernel_body("compare_fast_own.hpp", "k_compare_fast_own")
    assert len(plain) > 200 and len(own) > 200
    hunks = [op for op in difflib.SequenceMatcher(None, plain, own, autojunk=False).get_opcodes() if op[0] != "equal"]
    for tag, i0, i1, j0, j1 in hunks:
        theirs, ours = plain[i0:i1], own[j0:j1]
        marked = any("OWN" in l for l in ours) or any("void k_compare_fast_own(" in l for l in ours)
        assert marked, "compare_fast.hpp and compare_fast_own.hpp differ outside a hunk marked OWN:\n- %s\n+ %s" % (
            "\n- ".join(theirs), "\n+ ".join(ours))
    # the signature, the block-to-work mapping, the Nyquist rows' index, the partials' index
    assert len(hunks) == 4, hunks
    # and the marked hunks are small: the mapping is the only one of more than a line
    assert sum(j1 - j0 for _, _, _, j0, j1 in hunks) <= 12
