"""pl_render_params.hooks: C callbacks at the renderer's sixteen stages (reference pass_hook,
src/renderer.c:1036-1181, fired at :1779, :1873, :1917, :1959, :2054-2085, :2703, :2795).

The hooks are C (tests/hooks/testhooks.c: a hook returns a struct by value), loaded through
tests/hooklib.py; every call the renderer makes is logged there. What is checked is bit identity
wherever both sides run the same kernels: a hook that does nothing changes nothing, a hook that
hands back the texture it was given changes nothing where that texture exists anyway, and a hook
that computes (a kernel of its own, the library's ops appended to the recording) gives exactly what
the same computation gives outside the renderer. The suite pins PL_HIP_POLAR_MFMA=0 (conftest.py);
the identity cases run with the library's default (1) as well: both renders take the same kernel.
"""
import ctypes as C
import os

import numpy as np
import pytest

import hooklib
import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

STAGE = capi.HOOK_STAGE
SDR = dict(primaries="bt709", transfer="bt1886")
HDR = dict(primaries="bt2020", transfer="pq", max_luma=1000.0)
ERR_HOOKS = capi.RENDER_ERR_HOOKS


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture()
def hooks(built):
    """the helper library with its exported hooks as they were built, and an empty log"""
    L = hooklib.lib()
    defaults = {n: (hooklib.hook(n).stages, hooklib.hook(n).priv) for n in
                ("th_identity_tex", "th_invert", "th_double", "th_lut", "th_fail", "th_count_rgb",
                 "th_count_output")}
    hooklib.clear()
    yield L
    for n, (stages, priv) in defaults.items():
        hooklib.hook(n).stages, hooklib.hook(n).priv = stages, priv
    hooklib.release()


def render(gpu, image, dst, target_kw, params, hook_list=(), rr=None):
    """one pl_render_image into `dst` (a fresh renderer unless one is given) -> the frame"""
    own = rr is None
    rr = rr or pl.Renderer(gpu)
    pl.set_hooks(params, list(hook_list))
    util.srand(1)       # (the blue-noise matrix is generated from rand())
    ok = rr.render(image, pl.frame(dst, **target_kw), params)
    assert ok, gpu.messages[-6:]
    out = dst.download()
    state = (rr.errors(), rr.disabled_hooks())
    if own:
        rr.destroy()
    return out, state


def identical(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), util.diff_stats(
        a.view(np.uint16), b.view(np.uint16))


def f16_levels(w, h, seed):
    """rgba16hf texels that survive any number of f16 round trips: multiples of 1/4 in [0, 1]"""
    img = np.random.default_rng(seed).integers(0, 5, (h, w, 4)).astype(np.float16) / np.float16(4)
    img[..., 3] = 1
    return img


# ---- the three configurations of case 1 -----------------------------------------------------

def sdr_config(gpu):
    src = gpu.tex_create(72, 40, "rgba16", util.chirp_rgba16(72, 40))
    dst = gpu.tex_create(144, 80, "rgba16")
    image = pl.frame(src, components=3, color=pl.color_space(**SDR))
    return image, dst, dict(color=pl.color_space(**SDR)), lambda: pl.render_params("default"), [src, dst]


def hdr_config(gpu):
    """the metric's configuration (bench.py, workload ewa_1080p_to_4k_hdr_tonemap) at 72 x 40"""
    img = util.chirp_rgba16(72, 40).astype(np.float32)
    img[..., :3] *= 0.75
    src = gpu.tex_create(72, 40, "rgba16", np.rint(img).astype(np.uint16))
    dst = gpu.tex_create(144, 80, "rgba16")
    image = pl.frame(src, components=3, color=pl.color_space(**HDR))
    ten_bit = pl.color_repr("rgb", "full", sample_depth=16, color_depth=10, bit_shift=6)

    def params():
        return pl.render_params(
            "default", upscaler=pl.filter_config("ewa_lanczos"),
            dither_params=capi.DitherParams(method=pl.DITHER_BLUE_NOISE, lut_size=6, transfer=0),
            peak_detect_params=pl.peak_detect_params(percentile=99.995))
    return image, dst, dict(color=pl.color_space(**SDR), repr_=ten_bit), params, [src, dst]


def nv12_config(gpu):
    rng = np.random.default_rng(3)
    y = rng.integers(16, 236, (36, 64, 1), dtype=np.uint8)
    uv = rng.integers(16, 241, (18, 32, 2), dtype=np.uint8)
    ty, tuv = gpu.tex_create(64, 36, "r8", y), gpu.tex_create(32, 18, "rg8", uv)
    dst = gpu.tex_create(128, 72, "rgba16")
    f = capi.Frame(num_planes=2)
    f.planes[0].texture, f.planes[0].components = ty.ptr, 1
    f.planes[1].texture, f.planes[1].components = tuv.ptr, 2
    for c in range(4):
        f.planes[0].component_mapping[c] = 0 if c == 0 else -1
        f.planes[1].component_mapping[c] = c + 1 if c < 2 else -1
    f.repr = pl.color_repr("bt709", "limited", sample_depth=8, color_depth=8)
    f.color = pl.color_space(**SDR)
    pl.lib().pl_frame_set_chroma_location(f, 1)
    return f, dst, dict(color=pl.color_space(**SDR)), lambda: pl.render_params("default"), [ty, tuv, dst]


SCALE_STAGES = ["LINEAR", "SIGMOID", "PRE_KERNEL", "POST_KERNEL", "SCALED"]
SEQUENCE = {
    "sdr": ["RGB_INPUT", "NATIVE", "RGB"] + SCALE_STAGES + ["PRE_OUTPUT", "OUTPUT"],
    "nv12": ["LUMA_INPUT", "CHROMA_INPUT", "CHROMA_SCALED", "NATIVE", "RGB"] + SCALE_STAGES +
            ["PRE_OUTPUT", "OUTPUT"],
    # HDR is never sigmoidized (:2037-2042)
    "hdr": ["RGB_INPUT", "NATIVE", "RGB", "LINEAR", "PRE_KERNEL", "POST_KERNEL", "SCALED",
            "PRE_OUTPUT", "OUTPUT"],
}


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("config", ["sdr", "nv12", "hdr"])
def test_silent_hooks_change_nothing(gpu, hooks, config, mfma):
    """Case 1. PL_HOOK_SIG_NONE hooks on all sixteen stages: the call log is the reference's stage
    sequence for the configuration, every call carries the image's description at that stage,
    `reset` ran once, and the frame is the frame without hooks, byte for byte.

    For the SDR and NV12 upscales under pl_render_default_params that holds as it stands: the
    sigmoid is on without hooks, and linear light with it. For the HDR10 -> SDR upscale it cannot:
    by the reference's rule (:2009-2017, plan test (b)) a hook on PL_HOOK_LINEAR switches the scaler
    to linear light, which an HDR upscale is otherwise not scaled in, so the PLAN differs and with
    it the frame. There the property is split in two, each half byte-exact: the fourteen silent
    hooks that leave the plan alone give the frame without hooks, and all sixteen give the frame
    of the one hook that changes the plan (the silent hook on LINEAR alone)."""
    image, dst, tkw, params, texs = {"sdr": sdr_config, "nv12": nv12_config, "hdr": hdr_config}[config](gpu)
    silent = hooklib.silent()
    with env(PL_HIP_POLAR_MFMA=mfma):
        plain, state = render(gpu, image, dst, tkw, params())
        assert state == (0, []) and not hooklib.calls()
        hooked, state = render(gpu, image, dst, tkw, params(), silent)
        assert state == (0, [])
        log = hooklib.calls()
        assert hooklib.stages_called() == SEQUENCE[config]
        assert hooklib.resets() == 1
        if config == "hdr":
            keep = [h for h in silent if h.stages not in (STAGE["LINEAR"], STAGE["SIGMOID"])]
            quiet, _ = render(gpu, image, dst, tkw, params(), keep)
            identical(quiet, plain)
            linear_only, _ = render(gpu, image, dst, tkw, params(), [silent[9]])
            identical(hooked, linear_only)
            assert not np.array_equal(hooked, plain)     # (the plan did change)
        else:
            identical(hooked, plain)

    by_stage = {hooklib.STAGE_NAME[c.stage]: c for c in log}
    for name, c in by_stage.items():
        assert c.tag == capi.HOOK_STAGES.index(name)      # each hook at its own stage only
        assert not c.has_tex and not c.has_sh              # PL_HOOK_SIG_NONE
        assert list(c.dst_rect) == [0, 0, dst.w, dst.h]
    lin, native = pl.TRC["linear"], pl.TRC["pq" if config == "hdr" else "bt1886"]
    if config == "nv12":
        y, c, cs = by_stage["LUMA_INPUT"], by_stage["CHROMA_INPUT"], by_stage["CHROMA_SCALED"]
        assert (y.components, list(y.rect)) == (1, [0, 0, 64, 36])
        assert c.components == 2 and (c.rect[2] - c.rect[0], c.rect[3] - c.rect[1]) == (32, 18)
        assert cs.components == 2 and list(cs.rect) == [0, 0, 64, 36]
        assert y.sys == c.sys == by_stage["NATIVE"].sys == pl.SYS["bt709"]
    else:
        first = by_stage["RGB_INPUT"]
        assert (first.components, first.sys, list(first.rect)) == (3, pl.SYS["rgb"], [0, 0, 72, 40])
    w, h = (64, 36) if config == "nv12" else (72, 40)
    assert by_stage["NATIVE"].transfer == by_stage["RGB"].transfer == native
    assert by_stage["RGB"].sys == pl.SYS["rgb"] and by_stage["RGB"].components == 3
    for name in ("LINEAR", "SIGMOID", "PRE_KERNEL"):
        if name in by_stage:
            assert by_stage[name].transfer == lin and list(by_stage[name].rect) == [0, 0, w, h]
    for name in ("POST_KERNEL", "SCALED", "PRE_OUTPUT", "OUTPUT"):
        assert list(by_stage[name].rect) == [0, 0, dst.w, dst.h]
    assert by_stage["SCALED"].transfer == lin
    assert by_stage["PRE_OUTPUT"].transfer == pl.TRC["bt1886"]
    assert list(by_stage["SCALED"].src_rect) == [0, 0, w, h]
    for t in texs:
        t.destroy()


@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("preset", ["default", "ewa"])
def test_identity_tex_hook_where_a_texture_exists_anyway(gpu, hooks, preset, mfma):
    """Case 2. PL_HOOK_SIG_TEX at PRE_KERNEL, handing back the texture it was given: the scaler
    reads an intermediate there in any case (under pl_render_default_params the sigmoidized image;
    with an EWA scaler and the sigmoid the same), so the frame is the frame without hooks."""
    image, dst, tkw, _, texs = sdr_config(gpu)
    kw = dict(upscaler=pl.filter_config("ewa_lanczos")) if preset == "ewa" else {}
    h = hooklib.hook("th_identity_tex")
    with env(PL_HIP_POLAR_MFMA=mfma):
        plain, _ = render(gpu, image, dst, tkw, pl.render_params("default", **kw))
        hooked, state = render(gpu, image, dst, tkw, pl.render_params("default", **kw), [h])
    assert state == (0, [])
    (call,) = hooklib.calls()
    assert call.stage == STAGE["PRE_KERNEL"] and call.has_tex and (call.tex_w, call.tex_h) == (72, 40)
    identical(hooked, plain)
    for t in texs:
        t.destroy()


def one_to_one(gpu, seed=7):
    img = util.random_rgba16(48, 32, seed=seed)
    src = gpu.tex_create(48, 32, "rgba16", img)
    dst = gpu.tex_create(48, 32, "rgba16hf")
    image = pl.frame(src, components=3, color=pl.color_space(**SDR))
    return image, dst, dict(color=pl.color_space(**SDR)), [src, dst]


def test_identity_tex_hook_at_output_fbo_precision_is_idempotent(gpu, hooks):
    """Case 3. 1:1 into an rgba16hf target without dither: the hook makes the finished image go
    through an rgba16hf intermediate first, which rounds exactly as the target does."""
    image, dst, tkw, texs = one_to_one(gpu)
    h = hooklib.hook("th_identity_tex")
    h.stages = STAGE["OUTPUT"]
    plain, _ = render(gpu, image, dst, tkw, pl.render_params("fast"))
    hooked, state = render(gpu, image, dst, tkw, pl.render_params("fast"), [h])
    assert state == (0, [])
    (call,) = hooklib.calls()
    assert call.stage == STAGE["OUTPUT"] and (call.tex_w, call.tex_h) == (48, 32)
    identical(hooked, plain)
    for t in texs:
        t.destroy()


@pytest.mark.parametrize("async_measure", [True, False])
def test_hook_runs_a_kernel_of_its_own(hooks, built, async_measure):
    """Case 4. `invert` (tests/hooks/hook_kernels.hip) at OUTPUT, launched by the hook on the
    backend's stream from the stage texture into a texture from get_tex, both announced with
    pl_hip_tex_access: the frame is float16(1 - float32(x)) of the frame without the hook, alpha
    untouched. On a backend with the second stream and on one without."""
    with pl.HipGpu(0, async_measure=async_measure) as g:
        image, dst, tkw, texs = one_to_one(g)
        plain, _ = render(g, image, dst, tkw, pl.render_params("fast"))
        hooked, state = render(g, image, dst, tkw, pl.render_params("fast"),
                               [hooklib.hook("th_invert")])
        assert state == (0, []), g.messages[-4:]
        want = plain.copy()
        want[..., :3] = (np.float32(1) - plain[..., :3].astype(np.float32)).astype(np.float16)
        identical(hooked, want)
        assert len(np.unique(plain[..., :3])) > 1000     # (a frame worth inverting)
        for t in texs:
            t.destroy()


def test_resizable_stage_takes_a_doubled_plane(gpu, hooks):
    """Case 5. `double_nearest` at RGB_INPUT returns a texture of twice the size and the doubled
    rect: the frame is the frame of the pre-doubled source with the crop doubled. The same kernel
    at PRE_KERNEL -- not resizable -- is refused: error bit, signature disabled, frame unchanged."""
    img = f16_levels(72, 40, seed=11)
    src = gpu.tex_create(72, 40, "rgba16hf", img)
    big = gpu.tex_create(144, 80, "rgba16hf", np.repeat(np.repeat(img, 2, axis=0), 2, axis=1))
    dst = gpu.tex_create(144, 80, "rgba16")
    tkw = dict(color=pl.color_space(**SDR))
    crop = (3, 2, 70, 37)
    small = pl.frame(src, components=3, color=pl.color_space(**SDR), crop=crop)
    doubled = pl.frame(big, components=3, color=pl.color_space(**SDR), crop=tuple(2 * c for c in crop))

    h = hooklib.hook("th_double")
    want, _ = render(gpu, doubled, dst, tkw, pl.render_params("default"))
    got, state = render(gpu, small, dst, tkw, pl.render_params("default"), [h])
    assert state == (0, []), gpu.messages[-4:]
    (call,) = hooklib.calls()
    assert call.stage == STAGE["RGB_INPUT"] and list(call.rect) == list(crop)
    identical(got, want)

    hooklib.clear()
    h.stages = STAGE["PRE_KERNEL"]
    plain, _ = render(gpu, small, dst, tkw, pl.render_params("default"))
    got, (errors, disabled) = render(gpu, small, dst, tkw, pl.render_params("default"), [h])
    assert errors == ERR_HOOKS and disabled == [h.signature]
    assert hooklib.stages_called() == ["PRE_KERNEL"]
    identical(got, plain)
    for t in (src, big, dst):
        t.destroy()


def test_color_hook_appends_the_librarys_own_ops(gpu, hooks):
    """Case 6, first half. A hook at PL_HOOK_RGB applies a PL_LUT_NORMALIZED custom LUT with
    pl_shader_custom_lut (its own pl_shader_obj) to an opaque RGB image: the same op list as the
    same LUT given as pl_frame.lut, hence the same frame."""
    image, dst, tkw, _, texs = sdr_config(gpu)
    table = np.random.default_rng(5).random((7 * 7 * 7, 3)).astype(np.float32)
    lut = pl.custom_lut(table, (7, 7, 7))
    with_lut = pl.frame(texs[0], components=3, color=pl.color_space(**SDR))
    with_lut.lut, with_lut.lut_type = C.pointer(lut), pl.LUT_NORMALIZED
    want, _ = render(gpu, with_lut, dst, tkw, pl.render_params("default"))

    hooklib.priv("th_lut").lut = C.pointer(lut)
    got, state = render(gpu, image, dst, tkw, pl.render_params("default"), [hooklib.hook("th_lut")])
    assert state == (0, []), gpu.messages[-4:]
    (call,) = hooklib.calls()
    assert call.stage == STAGE["RGB"] and call.has_sh and not call.has_tex
    identical(got, want)
    plain, _ = render(gpu, image, dst, tkw, pl.render_params("default"))
    assert not np.array_equal(got, plain)
    for t in texs:
        t.destroy()


def test_color_hook_past_the_op_cap_is_split_not_truncated(gpu, hooks):
    """Case 6, second half. The op list of a pass holds 20 ops (PLH_MAX_OPS). A hook that appends
    24 -- a 1D LUT 24 times -- fills it: the renderer stores what is recorded and the hook's shader
    continues from the copy. The LUT permutes the levels k/4 and the source holds nothing else, so
    every intermediate value is exact in f16 and the expectation is exact however the ops are
    split: the frame equals (a) the permutation applied 24 times in numpy, and (b) the same ops
    applied in two renders of 12, byte for byte (within the custom LUT's own tolerance, which
    tests/test_lut.py sets for interpolated values: none is interpolated here)."""
    img = f16_levels(48, 32, seed=13)
    src = gpu.tex_create(48, 32, "rgba16hf", img)
    mid = gpu.tex_create(48, 32, "rgba16hf")
    dst = gpu.tex_create(48, 32, "rgba16hf")
    tkw = dict(color=pl.color_space(**SDR))
    # node i of channel c -> level (i + shift_c) mod 5
    shifts = (1, 2, 4)
    table = np.array([[((i + s) % 5) / 4 for s in shifts] for i in range(5)], np.float32)
    lut = pl.custom_lut(table, (5,))
    p = hooklib.priv("th_lut")
    p.lut = C.pointer(lut)
    h = hooklib.hook("th_lut")

    def frame_of(tex):
        return pl.frame(tex, components=3, color=pl.color_space(**SDR))

    p.count = 24
    got, state = render(gpu, frame_of(src), dst, tkw, pl.render_params("fast"), [h])
    assert state == (0, []), gpu.messages[-4:]
    assert len(hooklib.calls()) == 1

    want = img.copy()
    for c, s in enumerate(shifts):
        want[..., c] = ((np.rint(img[..., c].astype(np.float32) * 4).astype(int) + 24 * s) % 5) / 4
    identical(got, want)

    p.count = 12
    _, state = render(gpu, frame_of(src), mid, tkw, pl.render_params("fast"), [h])
    twice, state2 = render(gpu, frame_of(mid), dst, tkw, pl.render_params("fast"), [h])
    assert state == state2 == (0, [])
    identical(got, twice)
    for t in (src, mid, dst):
        t.destroy()


def test_failed_hook_is_disabled_until_reset(gpu, hooks):
    """Case 7. A hook that returns `failed` at SCALED: the frame is the frame without hooks and
    PL_RENDER_ERR_HOOKS is set; the next frame does not call it; pl_renderer_reset_errors with its
    signature brings it back, with another signature does not (:4203-4246)."""
    image, dst, tkw, params, texs = sdr_config(gpu)
    plain, _ = render(gpu, image, dst, tkw, params())
    h, other = hooklib.hook("th_fail"), hooklib.hook("th_count_rgb")
    rr = pl.Renderer(gpu)
    got, (errors, disabled) = render(gpu, image, dst, tkw, params(), [h, other], rr=rr)
    identical(got, plain)
    assert errors == ERR_HOOKS and disabled == [h.signature]
    assert hooklib.stages_called() == ["RGB", "SCALED"]

    hooklib.clear()
    got, (errors, disabled) = render(gpu, image, dst, tkw, params(), [h, other], rr=rr)
    identical(got, plain)
    assert errors == ERR_HOOKS and disabled == [h.signature]
    assert hooklib.stages_called() == ["RGB"]           # the failed hook is skipped

    hooklib.clear()
    rr.reset_errors(ERR_HOOKS, hooks=[other.signature])  # not the one that is disabled
    assert rr.errors() == ERR_HOOKS and rr.disabled_hooks() == [h.signature]
    render(gpu, image, dst, tkw, params(), [h, other], rr=rr)
    assert hooklib.stages_called() == ["RGB"]

    hooklib.clear()
    rr.reset_errors(ERR_HOOKS, hooks=[h.signature])
    assert rr.errors() == 0 and rr.disabled_hooks() == []
    _, (errors, disabled) = render(gpu, image, dst, tkw, params(), [h, other], rr=rr)
    assert hooklib.stages_called() == ["RGB", "SCALED"]  # called again (and fails again)
    assert errors == ERR_HOOKS and disabled == [h.signature]

    rr.reset_errors(ERR_HOOKS)                           # no list: every hook
    assert rr.errors() == 0 and rr.disabled_hooks() == []
    render(gpu, image, dst, tkw, params(), [h], rr=rr)
    rr.reset_errors()                                    # NULL: everything
    assert rr.errors() == 0 and rr.disabled_hooks() == []
    rr.destroy()
    for t in texs:
        t.destroy()


def test_mixing_caches_frames_by_their_hooks(gpu, hooks):
    """Case 8. pl_render_image_mix over three frames: a hook on RGB runs once per frame rendered
    into the cache and is part of what identifies a cached frame (:3561-3569); a hook on OUTPUT
    alone runs once per output, on the mixed image, and is not."""
    W, H = 64, 48
    base = util.chirp_rgba16(W, H).astype(np.float64)
    texs, frames = [], []
    for i in range(3):
        img = np.roll(base, 5 * i, axis=1) * (1.0 - 0.12 * i)
        img[..., 3] = 65535
        texs.append(gpu.tex_create(W, H, "rgba16", img.astype(np.uint16)))
        frames.append(pl.frame(texs[-1], components=3, color=pl.color_space(**SDR)))
    dst = gpu.tex_create(W, H, "rgba16")
    target = pl.frame(dst, color=pl.color_space(**SDR))
    cfg = capi.FilterConfig()
    C.memmove(C.byref(cfg), C.byref(pl.filter_config("mitchell", pl.FILTER_FRAME_MIXING)), C.sizeof(cfg))
    rgb, out = hooklib.hook("th_count_rgb"), hooklib.hook("th_count_output")
    params = pl.set_hooks(pl.render_params("fast", frame_mixer=cfg), [rgb, out])
    rr = pl.Renderer(gpu)

    def mix(ts):
        hooklib.clear()
        assert rr.render_mix(frames, [1000, 1001, 1002], ts, 1.0, target, params), gpu.messages[-4:]
        assert rr.errors() == 0
        return hooklib.stages_called()

    assert mix([-0.6, 0.4, 1.4]) == ["RGB", "RGB", "RGB", "OUTPUT"]
    assert mix([-0.7, 0.3, 1.3]) == ["OUTPUT"]           # all three cached
    other = hooklib.Priv(tag=205)
    out.priv = C.cast(C.pointer(other), C.c_void_p)      # the OUTPUT-only hook changes: no re-render
    assert mix([-0.8, 0.2, 1.2]) == ["OUTPUT"]
    assert hooklib.calls()[0].tag == 205
    another = hooklib.Priv(tag=206)
    rgb.priv = C.cast(C.pointer(another), C.c_void_p)    # the RGB hook changes: the cache is stale
    assert mix([-0.9, 0.1, 1.1]) == ["RGB", "RGB", "RGB", "OUTPUT"]
    assert [c.tag for c in hooklib.calls()] == [206, 206, 206, 205]
    rr.destroy()
    for t in texs + [dst]:
        t.destroy()


def test_without_intermediates_no_hook_runs(gpu, hooks):
    """Case 9. disable_fbos: there is nothing a hook could be handed or hand back (:1041): hooks
    are skipped, the frame is the frame without hooks."""
    image, dst, tkw, _, texs = sdr_config(gpu)
    plain, _ = render(gpu, image, dst, tkw, pl.render_params("default", disable_fbos=True))
    got, state = render(gpu, image, dst, tkw, pl.render_params("default", disable_fbos=True),
                        hooklib.silent() + [hooklib.hook("th_fail")])
    assert state == (0, []) and not hooklib.calls()
    identical(got, plain)
    for t in texs:
        t.destroy()
