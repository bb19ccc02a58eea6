"""pl_options in front of the renderer: a frame rendered with `&opts->params`, the options having
been loaded from text, is the frame rendered with a pl_render_params filled in by hand (or with
the library's preset struct), byte for byte. Both renders take the same kernels with the same
arguments, so there is nothing to tolerate. Every render gets a renderer of its own: no peak
measurement is carried from one to the next.

Two frames (SDR rgba16 and HDR10, 64 x 36 into 128 x 72), four option strings; and a C hook
installed with pl_options_add_hook against the same hook put into params.hooks directly."""
import ctypes as C

import numpy as np
import pytest

import hooklib
import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

SDR = dict(primaries="bt709", transfer="bt1886")
HDR10 = dict(primaries="bt2020", transfer="pq", max_luma=1000.0)
HAND_WRITTEN = ("upscaler=ewa_lanczos,downscaler=mitchell,deband=yes,deband_iterations=2,"
                "peak_detect=yes,tone_mapping=bt2390,gamut_mapping=perceptual,dither=yes,"
                "dither_method=ordered,sigmoid=no")


def library_struct(mirror, symbol):
    """a copy of one of the library's exported parameter structs"""
    out = mirror()
    C.memmove(C.byref(out), C.byref(mirror.in_dll(pl.lib(), symbol)), C.sizeof(mirror))
    return out


def hand_written_params():
    """HAND_WRITTEN, member by member"""
    deband = library_struct(capi.DebandParams, "pl_deband_default_params")
    deband.iterations = 2
    color_map = library_struct(capi.ColorMapParams, "pl_color_map_default_params")
    color_map.tone_mapping_function = pl.lib().pl_find_tone_map_function(b"bt2390")
    color_map.gamut_mapping = pl.lib().pl_find_gamut_map_function(b"perceptual")
    dither = library_struct(capi.DitherParams, "pl_dither_default_params")
    dither.method = pl.DITHER_ORDERED_FIXED
    return pl.render_params(
        "fast", upscaler=pl.filter_config("ewa_lanczos", pl.FILTER_UPSCALING),
        downscaler=pl.filter_config("mitchell", pl.FILTER_DOWNSCALING), deband_params=deband,
        peak_detect_params=library_struct(capi.PeakDetectParams, "pl_peak_detect_default_params"),
        color_map_params=color_map, dither_params=dither, sigmoid_params=None)


STRINGS = {
    "fast": ("preset=fast", lambda: pl.render_params("fast")),
    "default": ("preset=default", lambda: pl.render_params("default")),
    "high_quality": ("preset=high_quality", lambda: pl.render_params("high_quality")),
    "hand_written": (HAND_WRITTEN, hand_written_params),
}


def frames(gpu, kind):
    img = util.chirp_rgba16(64, 36).astype(np.float32)
    if kind == "hdr10":
        img[..., :3] *= 0.75
    src = gpu.tex_create(64, 36, "rgba16", np.rint(img).astype(np.uint16))
    dst = gpu.tex_create(128, 72, "rgba16")
    image = pl.frame(src, components=3, color=pl.color_space(**(HDR10 if kind == "hdr10" else SDR)))
    ten_bit = pl.color_repr("rgb", "full", sample_depth=16, color_depth=10, bit_shift=6)
    return image, dst, pl.frame(dst, color=pl.color_space(**SDR), repr_=ten_bit), [src, dst]


def render(gpu, image, dst, target, params):
    rr = pl.Renderer(gpu)
    util.srand(1)       # (the blue-noise matrix is generated from rand())
    ok = rr.render(image, target, params)
    assert ok, gpu.messages[-6:]
    out, errors = dst.download(), rr.errors()
    rr.destroy()
    return out, errors


@pytest.mark.parametrize("kind", ["sdr", "hdr10"])
@pytest.mark.parametrize("name", list(STRINGS))
def test_frame_from_an_option_string_is_the_frame_from_the_struct(gpu, kind, name):
    text, by_hand = STRINGS[name]
    image, dst, target, texs = frames(gpu, kind)
    opts = pl.Options(gpu.log)
    assert opts.load(text), gpu.messages[-4:]
    got, got_errors = render(gpu, image, dst, target, opts.params)
    want, want_errors = render(gpu, image, dst, target, by_hand())
    assert got_errors == want_errors, gpu.messages[-6:]
    assert np.array_equal(got, want), util.diff_stats(got, want)
    assert len(np.unique(got[..., :3])) > 100           # (a picture, not a cleared target)
    if name != "fast":
        # ... and the string did something: the empty configuration gives another frame
        opts.reset(None)
        plain, _ = render(gpu, image, dst, target, opts.params)
        assert not np.array_equal(got, plain)
    opts.free()
    for t in texs:
        t.destroy()


def test_hook_added_through_the_options_runs_like_one_in_params(gpu, built):
    """`invert` (tests/hooks) at OUTPUT of a 1:1 render into rgba16hf, installed both ways"""
    hooklib.lib()
    hooklib.clear()
    hook = hooklib.hook("th_invert")
    src = gpu.tex_create(48, 32, "rgba16", util.random_rgba16(48, 32, seed=7))
    dst = gpu.tex_create(48, 32, "rgba16hf")
    image = pl.frame(src, components=3, color=pl.color_space(**SDR))
    target = pl.frame(dst, color=pl.color_space(**SDR))

    opts = pl.Options(gpu.log)
    plain, _ = render(gpu, image, dst, target, opts.params)
    opts.add_hook(hook)
    assert opts.params.num_hooks == 1 and opts.save() == ""
    got, got_errors = render(gpu, image, dst, target, opts.params)
    want, want_errors = render(gpu, image, dst, target, pl.set_hooks(pl.render_params("fast"), [hook]))
    assert got_errors == want_errors == 0, gpu.messages[-6:]
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert not np.array_equal(got.view(np.uint16), plain.view(np.uint16))
    assert [c.tag for c in hooklib.calls()] == [101, 101]
    opts.remove_hook_at(-1)
    again, _ = render(gpu, image, dst, target, opts.params)
    assert np.array_equal(again.view(np.uint16), plain.view(np.uint16))

    opts.free()
    hooklib.release()
    for t in (src, dst):
        t.destroy()
