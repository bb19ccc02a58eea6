"""The numpy restatement of the colour map's diagnostics (tests/colormap_viz_ref.py), alone on the
CPU: for every input of tests/test_gpu_colormap_viz.py the share of samples it sets aside (a
decision taken by less than 1e-4) stays within the 2 % cap, its float32 run takes the float64
run's decisions on every sample kept, the clipping frame raises each flag from each of its
sources, and its building blocks are the formulas of tests/colormap_f64.py."""
import numpy as np
import pytest

import colormap_f64 as c64
import colormap_viz_ref as V


@pytest.fixture(scope="module")
def sdr709(built):
    return V.resolve(*V.spaces("bt709"))


def share(img, r, **kw):
    t, keep, r32 = V.compare(img, r, **kw)
    assert all(np.isfinite(v) for v in r32.values()), r32
    assert np.isfinite(t["out"]).all()
    return 1.0 - keep.mean(), t


def test_helpers_are_colormap_f64s_formulas(sdr709):
    rng = np.random.default_rng(1)
    x = rng.random(200)
    f8 = np.float64
    assert np.array_equal(V.pq_oetf(x * 5, f8), c64.pq_oetf(x * 5))
    assert np.array_equal(V.pq_eotf(x, f8), c64.pq_eotf(x))
    assert np.allclose(V.bt1886_inverse(x, 0.001, 1.0, f8), c64.bt1886_inverse(x, 0.001, 1.0), 0, 1e-15)
    kw = sdr709["kw"]
    assert np.allclose(V.lut1d(kw["tone_lut"], x, f8), c64.lerp_lut1d(kw["tone_lut"], x), 0, 1e-15)
    idx = [rng.random(200) * 1.2 - 0.1 for _ in range(3)]
    size = kw["gamut_size"]
    assert np.allclose(V.lut3d(kw["gamut_lut"], size, idx, f8), c64.lerp_lut3d(kw["gamut_lut"], size, idx), 0, 1e-14)
    inner = [np.clip(v, 0.0, 1.0) for v in idx]
    assert np.allclose(V.lut3d_cubic(kw["gamut_lut"], size, inner, f8),
                       c64.cubic_lut3d(kw["gamut_lut"], size, inner), 0, 1e-14)


def test_switches_off_is_the_plain_colour_map(sdr709):
    img = V.picture(32, 24)
    truth, _ = c64.hdr10_to_sdr(img, sdr709, 0.0)
    t = V.run(img, sdr709)
    # (the same formulas; this one holds the constants the device holds as floats, 0.5 / pi
    # among them, at float precision)
    assert np.abs(t["out"] - truth[..., :3]).max() < 1e-6
    assert (t["cls"] == V.UNMARKED).all() and not t["bits"].any()


def test_clipping_frame_raises_each_flag_from_each_source(sdr709):
    img, band = V.clip_frame(sdr709)
    aside, t = share(img, sdr709, show_clipping=True, prelinearized=True)
    assert aside <= V.SET_ASIDE_CAP, aside
    counts = {k: int(v.sum()) for k, v in t["raised"].items()}
    assert set(counts) == {"hi_rgb", "hi_I", "hi_idx", "lo_rgb", "lo_I", "lo_idx"}
    assert all(n >= 32 for n in counts.values()), counts
    # ... and from the band meant to: codes for 4000 nits, negative components, I below the
    # source's black, chroma beyond the LUT's range, the two ends of atan's range
    at = lambda src, b: int((t["raised"][src] & band[b]).sum())  # noqa: E731
    assert at("hi_rgb", "4000 nits") >= 32 and at("hi_I", "4000 nits") >= 32
    assert at("lo_rgb", "negative") >= 32 and at("lo_I", "below black") >= 32
    assert at("hi_idx", "negative") >= 32
    assert at("lo_idx", "hue -pi") >= 32 and at("hi_idx", "hue +pi") >= 1
    assert at("lo_I", "black") == band["black"].sum()
    assert (t["cls"] == V.CLIP_HI).sum() >= 32 and (t["cls"] == V.CLIP_LO).sum() >= 32
    assert (t["cls"] == V.UNMARKED).sum() >= 1024


@pytest.mark.parametrize("tone", ["spline", "clip", "linear"])
def test_tone_plot_share(built, tone):
    r = V.resolve(*V.spaces("bt2020"), tone=tone)
    assert r["need_tone"] and not r["need_gamut"]
    aside, t = share(V.picture(64, 64), r, visualize_lut=True)
    assert aside <= V.SET_ASIDE_CAP, aside
    assert (t["cls"] == V.TONE_PLOT).all()


def test_tone_plot_in_a_rect_share(built):
    r = V.resolve(*V.spaces("bt2020"))
    aside, t = share(V.picture(96, 64), r, visualize_lut=True, rect=V.RECT_96x64)
    assert aside <= V.SET_ASIDE_CAP, aside
    # 48 x 48 pixels whose centres sit on the main diagonal exactly
    assert t["in_rect"].sum() == 48 * 48 and t["in_rect"][8:56, 24:72].all()
    assert (t["cls"][~t["in_rect"]] == V.UNMARKED).all()


@pytest.mark.parametrize("hue,theta", V.HUE_THETA)
def test_gamut_plot_share(sdr709, hue, theta):
    aside, t = share(V.picture(64, 64), sdr709, visualize_lut=True, hue=hue, theta=theta)
    assert aside <= V.SET_ASIDE_CAP, aside
    assert (t["cls"] == V.GAMUT_PLOT).all()


def test_gamut_plot_tricubic_share(built):
    r = V.resolve(*V.spaces("bt709"), tricubic=True)
    aside, _ = share(V.picture(64, 64), r, visualize_lut=True, hue=0.3, theta=0.8)
    assert aside <= V.SET_ASIDE_CAP, aside


def test_both_switches_share(sdr709):
    img, _ = V.clip_frame(sdr709, 96, 64)
    aside, t = share(img, sdr709, show_clipping=True, visualize_lut=True, rect=V.RECT_96x64,
                     prelinearized=True)
    assert aside <= V.SET_ASIDE_CAP, aside
    assert {V.UNMARKED, V.CLIP_HI, V.CLIP_LO, V.GAMUT_PLOT} <= set(np.unique(t["cls"]))


def test_renderer_inputs_share(sdr709):
    # tests/test_gpu_colormap_viz.py, through pl_render_image: the plot over black
    for w, h in ((128, 72), (64, 48)):
        img = np.zeros((h, w, 4), np.float32)
        aside, _ = share(img, sdr709, visualize_lut=True, rect=V.RECT_96x64, hue=0.3, theta=0.8)
        assert aside <= V.SET_ASIDE_CAP, (w, h, aside)
