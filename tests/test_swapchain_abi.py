"""include/libplacebo/swapchain.h is layout- and source-compatible with the reference's header, and
the library exports the presentation interface.

Same mechanism as tests/test_abi_layout.py (tools/abi_probe.py: one C probe printing sizeof /
offsetof of every aggregate), with swapchain.h and the backend's own hip_swapchain.h as a group of
their own and a golden table of their own, tests/golden/abi_layout_swapchain.json
(`tools/abi_probe.py golden-swapchain`, from the reference's header). The ctypes mirrors
(_capi.MIRRORS_SWAPCHAIN) are held to the same probe. tests/c/swapchain_loop.c -- the reference's
render loop -- must compile against include/ and, where the reference's headers are present,
against those with only the backend include swapped. No GPU needed."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import pytest

from libplacebo_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_probe  # noqa: E402

GROUP = "swapchain"
GOLDEN = abi_probe.GROUPS[GROUP][1]
REF_GEN = os.path.join(ROOT, "oracle", "_ref", "gen")
HAVE_REF = os.path.isdir(os.path.join(abi_probe.REF, "src", "include")) and \
    os.path.exists(os.path.join(REF_GEN, "libplacebo", "config.h"))

REFERENCE_AGGREGATES = {"struct pl_swapchain_t", "struct pl_swapchain_frame"}
OWN_AGGREGATES = {"struct pl_hip_swapchain_params", "struct pl_hip_presented"}
LOOP = os.path.join(ROOT, "tests", "c", "swapchain_loop.c")


def norm(table):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in table.items()}


@pytest.fixture(scope="module")
def ours():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    return norm(abi_probe.run_probe("ours", abi_probe.aggregates("ours", GROUP), group=GROUP))


@pytest.fixture(scope="module")
def golden():
    return norm(json.load(open(GOLDEN)))


def test_layout_equals_the_reference_golden(ours, golden):
    assert {k for k in golden if "." not in k} == REFERENCE_AGGREGATES
    bad = {k: (ours.get(k), v) for k, v in golden.items() if ours.get(k) != v}
    assert not bad, bad


def test_no_member_missing_or_extra_and_own_aggregates(ours, golden):
    """every member the reference declares exists here and none is extra; the group's own
    aggregates are the two of hip_swapchain.h"""
    for agg in REFERENCE_AGGREGATES:
        theirs = {k for k in golden if k.startswith(agg + ".")}
        mine = {k for k in ours if k.startswith(agg + ".")}
        assert theirs and theirs == mine, (agg, sorted(theirs ^ mine))
    own = {k for k in ours if "." not in k} - REFERENCE_AGGREGATES
    assert own == OWN_AGGREGATES, own


@pytest.mark.skipif(not HAVE_REF, reason="reference headers not present")
def test_golden_is_what_the_reference_header_gives(golden):
    live = norm(abi_probe.run_probe("ref", group=GROUP))
    assert live == golden, "abi_layout_swapchain.json is stale: run tools/abi_probe.py golden-swapchain"


@pytest.mark.skipif(not HAVE_REF, reason="reference headers not present")
def test_members_textually_equal_the_reference():
    a, b = abi_probe.aggregates("ours", GROUP), abi_probe.aggregates("ref", GROUP)
    assert {f"{k[0]} {k[1]}" for k in b} == REFERENCE_AGGREGATES
    for k in b:
        assert a[k] == b[k], (k, a[k], b[k])    # same members, same order


def test_ctypes_mirrors_match_the_probe(ours):
    assert set(capi.MIRRORS_SWAPCHAIN) == REFERENCE_AGGREGATES | OWN_AGGREGATES
    assert not set(capi.MIRRORS_SWAPCHAIN) & set(capi.MIRRORS)
    bad = []
    for cname, mirror in capi.MIRRORS_SWAPCHAIN.items():
        if C.sizeof(mirror) != ours[cname]:
            bad.append((cname, "sizeof", C.sizeof(mirror), ours[cname]))
        for fname, *_ in mirror._fields_:
            key = f"{cname}.{fname.rstrip('_')}"
            assert key in ours, key
            f = getattr(mirror, fname)
            if (f.offset, f.size) != ours[key]:
                bad.append((key, (f.offset, f.size), ours[key]))
        n_c = sum(1 for k in ours if k.startswith(cname + "."))
        if n_c != len(mirror._fields_):
            bad.append((cname, "member count", len(mirror._fields_), n_c))
    assert not bad, bad


def test_library_exports_the_presentation_interface(built):
    """the seven functions of swapchain.h, the constructor and the two consumer calls of
    hip_swapchain.h, and renderer.h's pl_frame_from_swapchain"""
    lib = C.CDLL(capi.LIB_PATH)
    assert len(capi.SWAPCHAIN_FUNCTIONS) == 11
    missing = [n for n in capi.SWAPCHAIN_FUNCTIONS if not hasattr(lib, n)]
    assert not missing, missing


def _compile_only(args):
    r = subprocess.run(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror",
                        "-Wno-deprecated-declarations", "-c", LOOP, "-o", os.devnull, *args],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_loop_compiles_against_our_headers():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    _compile_only(["-I", os.path.join(ROOT, "include")])


@pytest.mark.skipif(not HAVE_REF, reason="reference headers not present")
def test_loop_compiles_against_the_reference_headers():
    """only the reference's headers on the search path: nothing of include/ can leak in"""
    _compile_only(["-DSWAPCHAIN_LOOP_REFERENCE", "-I", REF_GEN,
                   "-I", os.path.join(abi_probe.REF, "src", "include")])


def test_loop_program_was_built(built):
    assert os.access(os.path.join(ROOT, "tests", "c", "build", "swapchain_loop"), os.X_OK)
