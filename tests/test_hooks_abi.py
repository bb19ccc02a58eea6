"""include/libplacebo/shaders/custom.h is layout-identical to the reference's header: a `struct
pl_hook` compiled against libplacebo's own headers can be put into pl_render_params.hooks as it is.

Same mechanism as tests/test_abi_layout.py (tools/abi_probe.py: one C probe printing sizeof /
offsetof of every aggregate), with the header as a group of its own and a golden table of its own,
tests/golden/abi_layout_custom.json (`tools/abi_probe.py golden-custom`, from the reference's
header). The ctypes mirrors (_capi.MIRRORS_CUSTOM) are held to the same table. Also here: what the
two GLSL entry points of that header do on a backend without a shader compiler. No GPU needed."""
import ctypes as C
import json
import os
import shutil
import sys

import pytest

import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_probe  # noqa: E402

GOLDEN = abi_probe.GROUPS["custom"][1]
HAVE_REF = os.path.isdir(os.path.join(abi_probe.REF, "src", "include")) and \
    os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gen", "libplacebo", "config.h"))

AGGREGATES = ["struct pl_custom_shader", "struct pl_hook_params", "struct pl_hook_res",
              "union pl_var_data", "struct pl_hook_par", "struct pl_hook"]


def norm(table):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in table.items()}


@pytest.fixture(scope="module")
def ours():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    return norm(abi_probe.run_probe("ours", abi_probe.aggregates("ours", "custom"), group="custom"))


@pytest.fixture(scope="module")
def golden():
    return norm(json.load(open(GOLDEN)))


def test_every_member_has_the_references_offset_and_size(ours, golden):
    for name in AGGREGATES:
        assert name in golden, f"{name} missing from the golden table"
    assert {k for k in golden if "." not in k} == set(AGGREGATES)
    bad = {k: (ours.get(k), v) for k, v in golden.items() if ours.get(k) != v}
    assert not bad, bad
    assert set(ours) == set(golden), sorted(set(ours) ^ set(golden))


@pytest.mark.skipif(not HAVE_REF, reason="reference headers not present")
def test_golden_is_what_the_reference_header_gives(golden):
    live = norm(abi_probe.run_probe("ref", group="custom"))
    assert live == golden, "abi_layout_custom.json is stale: run tools/abi_probe.py golden-custom"


def test_ctypes_mirrors_match_the_header(ours):
    assert set(capi.MIRRORS_CUSTOM) == set(AGGREGATES)
    bad = []
    for cname, mirror in capi.MIRRORS_CUSTOM.items():
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


def test_stage_values_and_resizable_stages():
    """enum pl_hook_stage is a bit per stage in visiting order; the header's inline
    pl_hook_stage_resizable says which stages may change the image's size"""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    import subprocess
    import tempfile
    names = capi.HOOK_STAGES
    prog = "#include <stdio.h>\n#include <libplacebo/renderer.h>\nint main(void) {\n"
    for n in names:
        prog += f'    printf("{n} %d %d\\n", (int) PL_HOOK_{n}, (int) pl_hook_stage_resizable(PL_HOOK_{n}));\n'
    prog += '    printf("sig %d %d %d\\n", PL_HOOK_SIG_NONE, PL_HOOK_SIG_COLOR, PL_HOOK_SIG_TEX);\n'
    prog += "    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "p.c"), os.path.join(td, "p")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                       check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    resizable = {"RGB_INPUT", "LUMA_INPUT", "CHROMA_INPUT", "ALPHA_INPUT", "XYZ_INPUT", "NATIVE", "RGB"}
    for i, n in enumerate(names):
        assert out[i].split() == [n, str(1 << i), str(int(n in resizable))], out[i]
        assert capi.HOOK_STAGE[n] == 1 << i
    assert out[16].split() == ["sig", str(capi.HOOK_SIG_NONE), str(capi.HOOK_SIG_COLOR),
                               str(capi.HOOK_SIG_TEX)]


class Log:
    """a pl_log that keeps its messages"""

    def __init__(self):
        self.msgs = []
        self._cb = capi.LOG_CB(lambda _p, lev, msg: self.msgs.append((lev, msg.decode())))
        lp = capi.LogParams(log_cb=self._cb, log_priv=None, log_level=3)
        self.log = C.c_void_p(pl.lib().pl_log_create_365(365, C.byref(lp)))

    def close(self):
        pl.lib().pl_log_destroy(C.byref(self.log))


def test_glsl_entry_points_link_and_refuse(built):
    """No shader compiler here: pl_mpv_user_shader_parse returns NULL,
    pl_shader_custom fails the shader, each with one error naming the reason; _destroy takes NULL
    and a pointer to NULL."""
    L = pl.lib()
    log = Log()
    gpu = capi.Gpu(log=log.log)
    text = b"//!HOOK LUMA\n//!BIND HOOKED\nvec4 hook() { return HOOKED_tex(HOOKED_pos); }\n"
    assert not L.pl_mpv_user_shader_parse(C.byref(gpu), text, len(text))
    errors = [m for lev, m in log.msgs if lev <= 2]
    assert len(errors) == 1 and "no shader compiler" in errors[0], log.msgs

    L.pl_mpv_user_shader_destroy(None)
    none = C.POINTER(capi.Hook)()
    L.pl_mpv_user_shader_destroy(C.byref(none))
    assert not none

    L.pl_shader_alloc.restype = C.c_void_p
    L.pl_shader_alloc.argtypes = [C.c_void_p, C.c_void_p]
    L.pl_shader_free.argtypes = [C.POINTER(C.c_void_p)]
    sh = C.c_void_p(L.pl_shader_alloc(log.log, None))
    assert sh and not L.pl_shader_is_failed(sh)
    del log.msgs[:]
    body = capi.CustomShader(body=b"color = vec4(1.0);", input=0, output=1)
    assert not L.pl_shader_custom(sh, C.byref(body))
    assert L.pl_shader_is_failed(sh)
    errors = [m for lev, m in log.msgs if lev <= 2]
    assert len(errors) == 1 and "no shader compiler" in errors[0], log.msgs
    L.pl_shader_free(C.byref(sh))
    log.close()
