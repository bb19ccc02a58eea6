"""pl_color_map_params.show_clipping / .visualize_lut on the host: what the plan carries
(csrc/host/colormap_plan.c), which ops pl_shader_color_map_ex records for them and in which
order, and that no specialised kernel is handed a pass with them (the chain matcher, the fusion
into the polar scaler). No GPU."""
import ctypes as C

import pytest

import colormap_ref as cr
import libplacebo_amd as pl
import ref_structs as R
from libplacebo_amd import _capi as capi

# enum plh_op_kind (csrc/hip/plh_device.h)
SCALE, LIN, DELIN, DITHER, RGB2IPT, TONE, GAMUT, IPT2RGB = 1, 3, 4, 12, 20, 21, 22, 23
CLIP_TEST, CLIP_MARK, VIZ_GAMUT, VIZ_GAMUT_SRC, VIZ_GAMUT_DST, VIZ_TONE = 36, 37, 38, 39, 40, 41
RGBA16 = 6


@pytest.fixture(scope="module")
def lib(built):
    return R.declare(pl.lib())


def hdr10_to(target):
    return (cr.make_csp(pl.PRIM["bt2020"], pl.TRC["pq"], max_luma=1000.0),
            cr.make_csp(pl.PRIM[target], pl.TRC["bt1886"]))


def viz_plan(lib, src, dst, stateful=True, **kw):
    par = pl.color_map_params(**kw)
    flags, fields, kinds = (C.c_int * 3)(), (C.c_float * 6)(), (C.c_int * 20)()
    lib.plh_test_colormap_viz.restype = C.c_int
    n = lib.plh_test_colormap_viz(C.byref(par), C.byref(src), C.byref(dst), C.c_bool(stateful),
                                  flags, fields, kinds)
    return dict(show_clipping=bool(flags[0]), plot_tone=bool(flags[1]), plot_gamut=bool(flags[2]),
                rect=tuple(fields[:4]), hue=fields[4], theta=fields[5], kinds=list(kinds[:n]))


def test_binding_accepts_the_five_fields(built):
    p = pl.color_map_params(show_clipping=True, visualize_lut=True,
                            visualize_rect=(0.25, 0.125, 0.75, 0.875), visualize_hue=0.3,
                            visualize_theta=0.8)
    assert p.show_clipping and p.visualize_lut
    assert (p.visualize_rect.x0, p.visualize_rect.y0, p.visualize_rect.x1, p.visualize_rect.y1) == \
        (0.25, 0.125, 0.75, 0.875)
    assert p.visualize_hue == pytest.approx(0.3) and p.visualize_theta == pytest.approx(0.8)
    d = pl.color_map_params()
    assert not d.show_clipping and not d.visualize_lut and d.visualize_rect.x1 == 1.0


def test_plan_carries_the_fields(lib):
    p = viz_plan(lib, *hdr10_to("bt709"), show_clipping=True, visualize_lut=True,
                 visualize_rect=(0.25, 0.125, 0.75, 0.875), visualize_hue=0.3, visualize_theta=0.8)
    assert p["show_clipping"] and p["plot_tone"] and p["plot_gamut"]
    assert p["rect"] == (0.25, 0.125, 0.75, 0.875)
    assert p["hue"] == pytest.approx(0.3) and p["theta"] == pytest.approx(0.8)
    # an all-zero axis of the rect means 0 .. 1
    p = viz_plan(lib, *hdr10_to("bt709"), visualize_lut=True, visualize_rect=(0, 0.5, 0, 1))
    assert p["rect"] == (0.0, 0.5, 1.0, 1.0)
    p = viz_plan(lib, *hdr10_to("bt709"))
    assert not (p["show_clipping"] or p["plot_tone"] or p["plot_gamut"])
    # each plot exists where its stage does: no gamut map towards a BT.2020 target
    p = viz_plan(lib, *hdr10_to("bt2020"), visualize_lut=True)
    assert p["plot_tone"] and not p["plot_gamut"]


def test_op_order(lib):
    plain = [RGB2IPT, TONE, GAMUT, IPT2RGB]
    assert viz_plan(lib, *hdr10_to("bt709"))["kinds"] == plain
    # the RGB test in front of RGB2IPT (which overwrites the colour), the I test behind it, the
    # index test in front of the lookup; the flags act once, behind IPT2RGB
    assert viz_plan(lib, *hdr10_to("bt709"), show_clipping=True)["kinds"] == \
        [CLIP_TEST, RGB2IPT, CLIP_TEST, TONE, CLIP_TEST, GAMUT, IPT2RGB, CLIP_MARK]
    # the gamut plot inside the gamut stage, behind the lookup; the tone plot last
    assert viz_plan(lib, *hdr10_to("bt709"), visualize_lut=True)["kinds"] == \
        [RGB2IPT, TONE, GAMUT, VIZ_GAMUT, VIZ_GAMUT_SRC, VIZ_GAMUT_DST, IPT2RGB, VIZ_TONE]
    assert viz_plan(lib, *hdr10_to("bt709"), show_clipping=True, visualize_lut=True)["kinds"] == \
        [CLIP_TEST, RGB2IPT, CLIP_TEST, TONE, CLIP_TEST, GAMUT, VIZ_GAMUT, VIZ_GAMUT_SRC,
         VIZ_GAMUT_DST, IPT2RGB, CLIP_MARK, VIZ_TONE]
    assert viz_plan(lib, *hdr10_to("bt2020"), show_clipping=True, visualize_lut=True)["kinds"] == \
        [CLIP_TEST, RGB2IPT, CLIP_TEST, TONE, IPT2RGB, CLIP_MARK, VIZ_TONE]


def test_matrix_only_path_records_none(lib):
    src = cr.make_csp(pl.PRIM["bt709"], pl.TRC["bt1886"])
    dst = cr.make_csp(pl.PRIM["bt2020"], pl.TRC["pq"], max_luma=1000.0)
    p = viz_plan(lib, src, dst, tone="clip", gamut="clip", show_clipping=True, visualize_lut=True)
    assert p["kinds"] == [] and not (p["show_clipping"] or p["plot_tone"] or p["plot_gamut"])
    same = cr.make_csp(pl.PRIM["bt709"], pl.TRC["bt1886"])
    p = viz_plan(lib, same, cr.make_csp(pl.PRIM["bt709"], pl.TRC["bt1886"]), show_clipping=True)
    assert p["kinds"] == [] and not p["show_clipping"]


def record(lib, src, dst, **kw):
    """pl_shader_color_map_ex on a shader without a GPU and without a state object (the tone
    curve then is the linear stand-in, the gamut map a matrix) -> pl_shader_res.glsl"""
    L = pl.lib()
    lp = capi.LogParams(log_level=0)
    log = C.c_void_p(L.pl_log_create_365(365, C.byref(lp)))
    L.pl_shader_alloc.restype = C.c_void_p
    L.pl_shader_alloc.argtypes = [C.c_void_p, C.c_void_p]
    L.pl_shader_free.argtypes = [C.POINTER(C.c_void_p)]
    sh = C.c_void_p(L.pl_shader_alloc(log, None))
    par = pl.color_map_params(**kw)
    csrc, cdst = capi.ColorSpace.from_buffer_copy(src), capi.ColorSpace.from_buffer_copy(dst)
    args = capi.ColorMapArgs(src=csrc, dst=cdst, prelinearized=True)
    L.pl_shader_color_map_ex(sh, C.byref(par), C.byref(args))
    assert not L.pl_shader_is_failed(sh)
    res = L.pl_shader_finalize(sh)
    text = res.contents.glsl.decode()
    L.pl_shader_free(C.byref(sh))
    L.pl_log_destroy(C.byref(log))
    return [ln.split("(")[0] for ln in text.splitlines() if ln and not ln.startswith("#")]


def test_recorded_listing_has_a_line_per_op(lib):
    src, dst = hdr10_to("bt709")
    assert record(lib, src, dst) == ["rgb2ipt", "tone_map", "ipt2rgb", "delinearize"]
    assert record(lib, src, dst, show_clipping=True, visualize_lut=True) == \
        ["clip_test", "rgb2ipt", "clip_test", "tone_map", "ipt2rgb", "clip_mark", "viz_tone",
         "delinearize"]


def match(kinds):
    n = len(kinds)
    out = (C.c_int * 15)()
    fn = pl.lib().plh_test_match_chain
    fn.restype = C.c_int
    return bool(fn((C.c_int * n)(*kinds), (C.c_int * n)(), n, 0, RGBA16, 0, 1, 1, 1, out))


def test_chain_matcher_and_polar_fusion_refuse_such_a_pass(lib):
    fusable = lambda kinds: bool(pl.lib().plh_test_polar_fusable_ops((C.c_int * len(kinds))(*kinds),  # noqa: E731
                                                                       len(kinds)))
    tail = [DELIN, DITHER, SCALE]
    plain = [LIN, RGB2IPT, TONE, GAMUT, IPT2RGB]
    assert match(plain + tail) and fusable(plain + [DELIN])
    for kw in (dict(show_clipping=True), dict(visualize_lut=True),
               dict(show_clipping=True, visualize_lut=True)):
        for target in ("bt709", "bt2020"):
            kinds = [LIN] + viz_plan(lib, *hdr10_to(target), **kw)["kinds"]
            assert kinds != plain
            assert not match(kinds + tail), kinds
            assert not fusable(kinds + [DELIN]), kinds
    # each of the new ops alone is enough
    for op in (CLIP_TEST, CLIP_MARK, VIZ_GAMUT, VIZ_GAMUT_SRC, VIZ_GAMUT_DST, VIZ_TONE):
        assert not fusable([LIN, op]) and not match(plain + [op] + tail)
