"""The PQ EOTF's piece position (pqseg.hiph: pq_eotf_pos), one product against the two it replaces,
over all 2^32 bit patterns of a float: tests/c/eotf_pos_exhaustive.hip, a stand-alone program with
the old formulation kept in it as the reference. This test builds it with the library's flags
(tests/c/eotf_pos_exhaustive.mk), runs it once and reads its one line."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_product_is_the_two_products_for_every_float(gpu):
    env = dict(os.environ)
    if os.path.exists("/opt/rocm/bin/hipcc"):
        env["PATH"] = "/opt/rocm/bin:" + env.get("PATH", "")
    mk = subprocess.run(["make", "-f", os.path.join(ROOT, "tests", "c", "eotf_pos_exhaustive.mk")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert mk.returncode == 0, mk.stdout[-2000:]
    run = subprocess.run([os.path.join(ROOT, "tests", "c", "build", "eotf_pos_exhaustive")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(run.stdout.strip())
    m = re.search(r"over (\d+) bit patterns.*pq_eotf_pos<true> (\d+), pq_eotf_pos<false> (\d+)", run.stdout)
    assert m, run.stdout[-2000:]
    assert int(m.group(1)) == 1 << 32
    assert (int(m.group(2)), int(m.group(3))) == (0, 0), run.stdout
    assert run.returncode == 0, run.stdout[-2000:]
