"""What pl_render_params.hooks changes in the PLAN of a frame (render_plan.c, through plh_test_plan:
no GPU, no shader, and no callback -- the hooks here have none): the rules of the reference's
pass_scale_main (src/renderer.c:2004-2042) that depend on the hooks' stage masks only, and the
order in which the sixteen stages are visited (:1779, :1873, :1917, :1959, :2054-2085, :2703, :2795).
"""
import ctypes as C

import pytest

import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

STAGE = capi.HOOK_STAGE
ALL_STAGES = 0xffff


@pytest.fixture(scope="module")
def L(built):
    lib = pl.lib()
    lib.plh_test_format.restype = C.POINTER(capi.Fmt)
    lib.plh_test_format.argtypes = [C.c_char_p]
    lib.plh_test_plan.restype = C.c_size_t
    return lib


class FakeTex:
    """a pl_tex_t with nothing but params (what the planner may look at)"""

    def __init__(self, L, w, h, fmt):
        self.t = capi.Tex()
        self.t.params.w, self.t.params.h = w, h
        self.t.params.format = L.plh_test_format(fmt.encode())
        assert self.t.params.format, fmt
        self.t.params.sampleable = True
        self.t.params.storable = True
        self.ptr = C.pointer(self.t)


def plan(L, image, target, params):
    buf = C.create_string_buffer(4096)
    L.plh_test_plan(C.byref(image), C.byref(target), C.byref(params), C.c_bool(True),
                    C.c_size_t(160 * 1024), buf, C.c_size_t(len(buf)))
    return buf.value.decode()


def rgb_frames(L, src, dst, icsp=None, tcsp=None):
    s, d = FakeTex(L, *src, "rgba16"), FakeTex(L, *dst, "rgba16")
    image = pl.frame(s, components=3, color=icsp)
    target = pl.frame(d, color=tcsp)
    image._keep, target._keep = s, d
    return image, target


def nv12_frames(L, src, dst):
    y, uv = FakeTex(L, *src, "r8"), FakeTex(L, src[0] // 2, src[1] // 2, "rg8")
    d = FakeTex(L, *dst, "rgba16")
    f = capi.Frame(num_planes=2)
    f.planes[0].texture, f.planes[0].components = y.ptr, 1
    f.planes[1].texture, f.planes[1].components = uv.ptr, 2
    for c in range(4):
        f.planes[0].component_mapping[c] = 0 if c == 0 else -1
        f.planes[1].component_mapping[c] = c + 1 if c < 2 else -1
    f.repr = pl.color_repr("bt709", "limited", sample_depth=8, color_depth=8)
    f.color = pl.color_space("bt709", "bt1886")
    target = pl.frame(d, color=pl.color_space("bt709", "bt1886"))
    f._keep, target._keep = (y, uv), d
    return f, target


def with_hook(params, stages):
    """one hook on `stages` without callbacks: the planner must not call it"""
    h = capi.Hook(stages=stages, input=capi.HOOK_SIG_TEX, signature=1)
    assert not h.hook and not h.reset
    return pl.set_hooks(params, [h])


def hook_line(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("hook stages:")]
    assert len(lines) == 1, text
    return lines[0][len("hook stages:"):].split()


def test_pre_kernel_hook_keeps_the_main_scaler_of_a_1_to_1_render(L):
    """(a) :2004-2031: without hooks a 1:1 render skips the main scaler as a no-op; a hook that
    wants to see what the scaler reads forces the stage (and its intermediate) to exist"""
    image, target = rgb_frames(L, (48, 32), (48, 32))
    text = plan(L, image, target, pl.render_params("default"))
    assert "scale: none" in text and "hook stages" not in text, text
    text = plan(L, image, target, with_hook(pl.render_params("default"), STAGE["PRE_KERNEL"]))
    assert "scale: nearest none (kept for hooks) -> 48x32" in text, text   # (1:1: a plain fetch)
    assert hook_line(text) == ["PRE_KERNEL"], text
    # the same for a free (bilinear) upscale, which is otherwise left to the output pass
    image, target = rgb_frames(L, (48, 32), (96, 64))
    assert "scale: deferred" in plan(L, image, target, pl.render_params("fast"))
    text = plan(L, image, target, with_hook(pl.render_params("fast"), STAGE["POST_KERNEL"]))
    assert "scale: builtin up (kept for hooks) -> 96x64" in text, text


def test_linear_hook_switches_linear_light_on(L):
    """(b) :2009-2017, :2033-2042: a hook on LINEAR makes an SDR upscale happen in linear light
    although nothing else asks for it (no sigmoid); on an HDR10 source the sigmoid stays off"""
    sdr = pl.color_space("bt709", "bt1886")
    image, target = rgb_frames(L, (72, 40), (144, 80), icsp=sdr, tcsp=sdr)
    base = dict(upscaler=pl.filter_config("lanczos"), sigmoid_params=None)
    text = plan(L, image, target, pl.render_params("fast", **base))
    assert "scale: separable up two-pass -> 144x80" in text, text
    text = plan(L, image, target, with_hook(pl.render_params("fast", **base), STAGE["LINEAR"]))
    assert "scale: separable up linear two-pass -> 144x80" in text, text
    assert hook_line(text) == ["LINEAR"], text
    # a SIGMOID hook switches the sigmoid on as well (with the default curve)
    text = plan(L, image, target, with_hook(pl.render_params("fast", **base), STAGE["SIGMOID"]))
    assert "scale: separable up linear sigmoid two-pass -> 144x80" in text, text

    hdr = pl.color_space("bt2020", "pq", max_luma=1000.0)
    image, target = rgb_frames(L, (72, 40), (144, 80), icsp=hdr, tcsp=sdr)
    both = STAGE["LINEAR"] | STAGE["SIGMOID"]
    text = plan(L, image, target, with_hook(pl.render_params("default"), both))
    assert "scale: separable up linear two-pass -> 144x80" in text and "sigmoid" not in text, text
    assert hook_line(text) == ["LINEAR"], text
    # ... and disable_linear_scaling wins over both (:2033-2035)
    text = plan(L, image, target, with_hook(pl.render_params("default", disable_linear_scaling=True), both))
    assert "linear" not in text.split("scale:")[1].splitlines()[0], text
    assert hook_line(text) == ["none"], text


def test_stage_sequence_is_the_references(L):
    """(c) pl_render_default_params, a hook on every stage: an RGB source, and NV12 (whose luma
    plane has no aligned stage, :1439-1445)"""
    sdr = pl.color_space("bt709", "bt1886")
    image, target = rgb_frames(L, (72, 40), (144, 80), icsp=sdr, tcsp=sdr)
    text = plan(L, image, target, with_hook(pl.render_params("default"), ALL_STAGES))
    assert hook_line(text) == ["RGB_INPUT", "NATIVE", "RGB", "LINEAR", "SIGMOID", "PRE_KERNEL",
                               "POST_KERNEL", "SCALED", "PRE_OUTPUT", "OUTPUT"], text
    image, target = nv12_frames(L, (64, 36), (128, 72))
    text = plan(L, image, target, with_hook(pl.render_params("default"), ALL_STAGES))
    assert hook_line(text) == ["LUMA_INPUT", "CHROMA_INPUT", "CHROMA_SCALED", "NATIVE", "RGB",
                               "LINEAR", "SIGMOID", "PRE_KERNEL", "POST_KERNEL", "SCALED",
                               "PRE_OUTPUT", "OUTPUT"], text
    # an HDR10 source: linear light (forced by the hook on LINEAR), never sigmoidized
    hdr = pl.color_space("bt2020", "pq", max_luma=1000.0)
    image, target = rgb_frames(L, (72, 40), (144, 80), icsp=hdr, tcsp=sdr)
    text = plan(L, image, target, with_hook(pl.render_params("default"), ALL_STAGES))
    assert hook_line(text) == ["RGB_INPUT", "NATIVE", "RGB", "LINEAR", "PRE_KERNEL",
                               "POST_KERNEL", "SCALED", "PRE_OUTPUT", "OUTPUT"], text


def test_no_intermediates_no_hook_stage(L):
    """(d) :1041: without a four-component intermediate format (disable_fbos) no hook runs, and
    none changes the plan"""
    sdr = pl.color_space("bt709", "bt1886")
    image, target = rgb_frames(L, (72, 40), (144, 80), icsp=sdr, tcsp=sdr)
    bare = plan(L, image, target, pl.render_params("default", disable_fbos=True))
    text = plan(L, image, target, with_hook(pl.render_params("default", disable_fbos=True), ALL_STAGES))
    assert hook_line(text) == ["none", "(no", "intermediate", "format)"], text
    assert [ln for ln in text.splitlines() if not ln.startswith("hook stages:")] == bare.splitlines()
