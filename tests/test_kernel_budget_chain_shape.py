"""Register budget of the shape-specialised instances of k_polar_mx (k_polar_mxs.hip), from the
compiler's resource report next to the object (build/hip_k_polar_mxs.usage): the three conditions
tests/test_kernel_budget.py holds the generic chain instance k_polar_mx<3, true, 3, 8> to -- at most
120 registers (so that a wave of the next frame's measuring pass fits beside four of its waves on a
SIMD), 4 waves per SIMD, no scratch."""
import os
import re
import subprocess

BUILD = os.path.join(os.path.dirname(__file__), "..", "libplacebo_amd", "csrc", "build")


def test_shape_instances_keep_the_chain_budget(built):
    text = open(os.path.join(BUILD, "hip_k_polar_mxs.usage")).read()
    found = re.findall(r"Function Name: (\S+)\nVGPRs: (\d+)\nScratchSize \[bytes/lane\]: (\d+)\n"
                       r"Occupancy \[waves/SIMD\]: (\d+)", text)
    names = subprocess.run(["c++filt"] + [n for n, *_ in found], capture_output=True,
                           text=True).stdout.split("\n")
    recs = {name.replace("void ", "").replace("(plh_pass)", ""): (int(v), int(s), int(o))
            for (_, v, s, o), name in zip(found, names)}
    # MX_POST_SHAPE + curve (k_polar_mx.hiph): BT.1886, the power laws, sRGB
    want = ["k_polar_mx<3, true, %d, 8>" % post for post in (8, 9, 10)]
    assert sorted(recs) == sorted(want), sorted(recs)
    for name, (vgprs, scratch, occupancy) in recs.items():
        assert vgprs <= 120 and scratch == 0 and occupancy >= 4, (name, vgprs, scratch, occupancy)
