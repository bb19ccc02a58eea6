"""The matrix-pipe tables of the polar kernels (csrc/host/polar_mx_tables.c) -- the blob k_polar_mx,
k_polar_mxp, k_polar_mxr and k_polar_mxd read: f16 hi + lo weight fragments, their first-order
derivatives in the phase, the per-column / per-row phase deviations -- pinned byte for byte.
Host logic only (no GPU): tests/golden/polar_mx_tables.npz holds what the device evaluated for
each geometry (fcoord and base texel of every column and row, the phase classes, the tap list, the
weights of every class pair) and tests/golden/polar_mx_tables.json what the commit named in it
built from them, recorded on an MI355X: the kind, every scalar of struct plh_polar_mx, the blob's
layout and SHA-256 -- of the whole blob and of each section, so that a failure names the section --
and the figures its log line prints (largest phase deviation, weight split error, row asymmetry).
The hook classifies the axes itself and fails where that differs from the recorded classes, then
tries the kinds in the library's order. tests/test_gpu_polar_mfma.py renders these geometries and
holds the kernels to k_polar_pp."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import libplacebo_amd as pl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "polar_mx_tables.json")) as f:
    FIXTURE = json.load(f)
CASES = FIXTURE["cases"]
SCALARS = ("ratio", "group", "sx", "sy", "org_x", "org_y", "npairs", "row_first0", "row_first1")
PROPS = ("bound", "tile_fp32", "address_mode", "transpose", "src_w")
ARRAYS = (("colfc", np.float32), ("rowfc", np.float32), ("colbase", np.int32), ("rowbase", np.int32),
          ("clsx", np.float32), ("clsy", np.float32), ("idx", np.uint16), ("idy", np.uint16),
          ("taps", np.uint32), ("wall", np.float32))


class Case(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("w", "h", "ncx", "ncy", "ntaps") + PROPS] +
                [("antiring", C.c_float), ("max_shmem_size", C.c_uint64)] +
                [(n, C.c_void_p) for n, _ in ARRAYS])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sections(blob, dfx, dfy, sink):
    """the blob by section: the four fragment kinds (frag f = 4 * group + kind, 64 lanes x 8 f16
    each), then the two deviation tables"""
    frag = np.frombuffer(blob[:dfx], np.uint16).reshape(-1, 4, 64 * 8)
    out = {k: sha(frag[:, i]) for i, k in enumerate(("hi", "lo", "ddx", "ddy"))}
    out["dfx"] = sha(np.frombuffer(blob[dfx:dfy], np.uint8))
    out["dfy"] = sha(np.frombuffer(blob[dfy:sink or len(blob)], np.uint8))
    return out


def build(name, **override):
    """the hook on the recorded inputs of one case -> (kind, scalars, layout, blob, figures)"""
    with np.load(os.path.join(GOLDEN, "polar_mx_tables.npz")) as z:
        arr = {n: np.ascontiguousarray(z[name + "_" + n], dtype=t) for n, t in ARRAYS}
    for n, v in override.items():
        if n in arr:
            arr[n] = np.ascontiguousarray(v, dtype=arr[n].dtype)
    props = dict(CASES[name]["props"], **{n: v for n, v in override.items() if n not in arr})
    c = Case(w=len(arr["colfc"]), h=len(arr["rowfc"]), ncx=len(arr["clsx"]), ncy=len(arr["clsy"]),
             ntaps=len(arr["taps"]), antiring=float.fromhex(props["antiring"]),
             max_shmem_size=props["max_shmem_size"], **{n: props[n] for n in PROPS},
             **{n: a.ctypes.data for n, a in arr.items()})
    assert len(arr["wall"]) == c.ncx * c.ncy * (c.ntaps + 1)
    fn = pl.lib().plh_test_polar_mx_tables
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(Case), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    scalars, layout, figures = np.zeros(9, np.int32), np.zeros(4, np.uint64), np.zeros(3, np.float64)
    blob = np.zeros(256 * 1024, np.uint8)
    kind = fn(C.byref(c), scalars.ctypes.data, layout.ctypes.data, figures.ctypes.data, blob.ctypes.data,
              blob.nbytes)
    return (kind, dict(zip(SCALARS, map(int, scalars))), [int(v) for v in layout], blob,
            dict(zip(("dev", "worst", "asym"), map(float, figures))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_are_those_of_the_recorded_commit(name):
    want = CASES[name]["expect"]
    kind, scalars, (dfx, dfy, sink, size), blob, figures = build(name)
    assert kind == want["kind"]
    assert scalars == {k: want[k] for k in SCALARS}
    assert (dfx, dfy, sink, size) == (want["dfx"], want["dfy"], want["sink"], want["size"])
    if not kind:
        return
    blob = blob[:size].tobytes()
    got = sections(blob, dfx, dfy, sink)
    assert got == want["sections"], [k for k in got if got[k] != want["sections"][k]]
    assert hashlib.sha256(blob).hexdigest() == want["sha256"]
    # the figures of the log line, to the bit, and as the recorded line words them
    assert figures == {k: float.fromhex(want[k]) for k in figures}
    line = [l for l in CASES[name]["log"] if "matrix-pipe tables" in l]
    assert len(line) == 1 and "phases within %.2e:" % figures["dev"] in line[0]
    assert line[0].endswith("weight split error <= %.2e" % figures["worst"])
    assert kind != 2 or "row symmetry %.1e," % figures["asym"] in line[0]


def test_fixture_covers_what_it_claims():
    """both row-pair counts of the 2x kind, both groups of the R : G kind, the wrapped phase of the
    odd ratio on either axis (cases i and k: rows and columns above 0.98; at the size of case d the
    device leaves no output there), first-order
    tables that are not all zeros (but for case g, whose only phase class is 1/2 exactly: case j
    is the 2 : 1 geometry with deviations), and a geometry every kind refuses"""
    e = {n: c["expect"] for n, c in CASES.items()}
    assert {3, 4} <= {x["npairs"] for x in e.values() if x["kind"] == 1}
    assert {1, 2} <= {x["group"] for x in e.values() if x["kind"] == 3}
    assert {0, 1, 2, 3} == {x["kind"] for x in e.values()}
    with np.load(os.path.join(GOLDEN, "polar_mx_tables.npz")) as z:
        assert e["i"]["kind"] == 3 and (z["i_rowfc"] > 0.98).any()
        assert e["k"]["kind"] == 3 and (z["k_colfc"] > 0.98).any()
    assert all(float.fromhex(x["dev"]) > 0 for n, x in e.items() if x["kind"] and n != "g")
    assert e["j"]["kind"] == 2 and float.fromhex(e["j"]["dev"]) > 0


def test_a_change_of_the_classes_is_noticed():
    """the hook classifies the axes itself: a recorded class id that is off by one fails the case"""
    with np.load(os.path.join(GOLDEN, "polar_mx_tables.npz")) as z:
        idx = z["a_idx"].copy()
    idx[5] ^= 1
    assert build("a", idx=idx)[0] == -1


def test_eligibility_is_per_kind():
    """2x and R : G need 64 KiB of shared memory and a bound <= 4, 2 : 1 needs 124 KiB and has no
    bound test (its 14 x 14 footprint is bound 7)"""
    up = [n for n, c in CASES.items() if c["expect"]["kind"] in (1, 3)]
    down = [n for n, c in CASES.items() if c["expect"]["kind"] == 2]
    for n in up:
        assert build(n, max_shmem_size=64 * 1024)[0] == CASES[n]["expect"]["kind"]
        assert build(n, max_shmem_size=64 * 1024 - 1)[0] == 0
        assert build(n, bound=5)[0] == 0
    for n in down:
        assert CASES[n]["props"]["bound"] > 4
        assert build(n, max_shmem_size=124 * 1024)[0] == 2
        assert build(n, max_shmem_size=124 * 1024 - 1)[0] == 0
    for n in up + down:
        for prop in (dict(tile_fp32=1), dict(transpose=1), dict(address_mode=1), dict(src_w=1),
                     dict(antiring="0x1p-1")):
            assert build(n, **prop)[0] == 0, (n, prop)
