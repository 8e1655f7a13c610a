"""The own-list variants of k_compare_fast and k_nyquist_rows are instantiations of those kernels on another argument
struct, so the two bodies cannot drift: there is ONE body.  This test keeps it so -- no second __global__
definition of either kernel, under either name, anywhere in the engine's sources."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bioem_amd", "csrc")


def global_definitions(name):
    """(file, line) of every `__global__ ... void name(` in bioem_amd/csrc"""
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path) or not path.endswith((".hpp", ".hip", ".inc", ".h", ".cpp")):
            continue
        # a definition may break its line between the attributes and the name
        text = re.sub(r"\s+", " ", open(path).read())
        for m in re.finditer(r"__global__[^;{}()]*(?:\([^()]*\))?[^;{}()]*\bvoid %s\(" % name, text):
            found.append((os.path.basename(path), m.start()))
    return found


def test_one_body_for_the_fast_kernel_and_its_own_list_variant():
    assert len(global_definitions("k_compare_fast")) == 1, global_definitions("k_compare_fast")
    assert len(global_definitions("k_nyquist_rows")) == 1, global_definitions("k_nyquist_rows")
    assert global_definitions("k_compare_fast_own") == []
    assert global_definitions("k_nyquist_rows_own") == []
    assert global_definitions("k_compare_fast")[0][0] == "compare_fast.hpp"
    assert global_definitions("k_nyquist_rows")[0][0] == "compare_fast.hpp"
    assert not os.path.exists(os.path.join(CSRC, "compare_fast_own.hpp"))
