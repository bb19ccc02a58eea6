"""The PL_HIP_* environment switches are one table (libplacebo_amd/csrc/hip/plh_switch.h) read by
one function (csrc/host/plh_switch.c). These tests read the sources as text and keep it so: no
second reader of the environment, INTEGRATION.md's table follows the code's, and every switch a
test, the benchmark, the entry points or the public header names exists."""
import glob
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "libplacebo_amd", "csrc")
# named like switches, but not the library's: the binding's library path, the public header's
# parameter defaults macro, the parity tests' report mode
NOT_SWITCHES = {"PL_HIP_LIB", "PL_HIP_DEFAULTS", "PL_PARITY_REPORT_ONLY"}


def read(*path):
    with open(os.path.join(ROOT, *path), encoding="utf-8") as f:
        return f.read()


def table_names():
    rows = re.findall(r'^\s*X\((\w+),\s*"(\w+)",\s*(-?\d+),\s*"[^"]+"\)', read(CSRC, "hip", "plh_switch.h"), re.M)
    assert rows, "no X(...) rows found in plh_switch.h"
    for ident, name, _ in rows:
        assert name == "PL_HIP_" + ident, (ident, name)
    names = [name for _, name, _ in rows]
    assert len(set(names)) == len(names), names
    return names


def test_one_reader_of_the_environment():
    sources = [f for f in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True)
               if os.path.isfile(f) and os.sep + "build" + os.sep not in f]
    assert len(sources) > 50, len(sources)
    users = sorted(os.path.relpath(f, CSRC) for f in sources
                   if "getenv(" in open(f, encoding="utf-8", errors="replace").read())
    assert users == [os.path.join("host", "plh_switch.c")], users


def test_document_follows_the_table():
    doc = read("INTEGRATION.md")
    start = doc.index("| variable | values and effect |")
    table = doc[start:doc.index("\n\n", start)]
    documented = re.findall(r"^\| `(PL_HIP_\w+)` \|", table, re.M)
    assert documented == table_names()     # the same switches, in the same order
    # no other switch is mentioned inside a row either
    assert set(re.findall(r"PL_HIP_\w+", table)) == set(table_names())


def test_every_switch_in_use_is_in_the_table():
    known = set(table_names())
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) + [
        os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py"),
        os.path.join(ROOT, "include", "libplacebo", "hip.h")]
    assert len(files) > 20
    unknown = {}
    for f in files:
        used = set(re.findall(r"\bPL_HIP_[A-Z0-9_]+\b|\bPL_PARITY_REPORT_ONLY\b", open(f, encoding="utf-8").read()))
        bad = used - known - NOT_SWITCHES
        if bad:
            unknown[os.path.relpath(f, ROOT)] = sorted(bad)
    assert not unknown, unknown
