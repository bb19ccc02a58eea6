"""tests/hooks/build/libtesthooks.so (built by build()) as the hook tests use it: the exported
`struct pl_hook` objects, the call log and the reset counter (tests/hooks/testhooks.c)."""
import ctypes as C
import os

import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

HERE = os.path.dirname(os.path.abspath(__file__))
STAGE = capi.HOOK_STAGE
STAGE_NAME = {v: k for k, v in STAGE.items()}


class Call(C.Structure):
    _fields_ = [("stage", C.c_int), ("tag", C.c_int), ("rect", C.c_float * 4),
                ("components", C.c_int), ("sys", C.c_int), ("transfer", C.c_int),
                ("has_tex", C.c_int), ("has_sh", C.c_int), ("tex_w", C.c_int), ("tex_h", C.c_int),
                ("src_rect", C.c_float * 4), ("dst_rect", C.c_int * 4)]


class Priv(C.Structure):
    _fields_ = [("tag", C.c_int), ("count", C.c_int), ("lut", C.POINTER(capi.CustomLut)),
                ("lut_state", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        pl.lib()    # (libplacebo_hip.so first: the helper links against it)
        _lib = C.CDLL(os.path.join(HERE, "hooks", "build", "libtesthooks.so"))
        assert _lib.th_sizeof_call() == C.sizeof(Call)
        assert _lib.th_sizeof_priv() == C.sizeof(Priv)
    return _lib


def hook(name):
    """the exported `struct pl_hook <name>` (changes are seen by the renderer)"""
    return capi.Hook.in_dll(lib(), name)


def priv(name):
    return Priv.in_dll(lib(), name + "_priv")


def silent():
    """sixteen PL_HOOK_SIG_NONE hooks, one per stage, in stage order"""
    return list((capi.Hook * 16).in_dll(lib(), "th_silent"))


def clear():
    lib().th_clear()


def calls():
    n = C.c_int.in_dll(lib(), "th_num_calls").value
    log = (Call * 512).in_dll(lib(), "th_calls")
    return [log[i] for i in range(n)]


def stages_called(tag=None):
    return [STAGE_NAME[c.stage] for c in calls() if tag is None or c.tag == tag]


def resets():
    return C.c_int.in_dll(lib(), "th_num_resets").value


def release():
    lib().th_release()
