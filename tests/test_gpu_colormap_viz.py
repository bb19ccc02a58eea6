"""pl_color_map_params.show_clipping / .visualize_lut on the GPU, held to the numpy restatement
of tests/colormap_viz_ref.py.

Tolerance, per test and per pixel class (unmarked, clip_hi, clip_lo, tone plot, gamut plot): with
R32 = the largest distance between the restatement's float32 and float64 runs over the class, the
GPU must lie within max(4 R32, 1 / 65535) of the float64 run. The factor of 4 covers the device's
transcendentals (polynomial atan, the PQ pieces, sin / cos / pow), which a rounded numpy run does
not model; the floor is one 16-bit code. A sample is set aside when a decision the float64 run
takes for it has a margin below 1e-4 (`a || b` evaluated left to right: a test behind a flag that
is already set is not taken); tests/test_colormap_viz_ref.py holds the share of such samples to
2 % for every input used here. Every other sample must come out as the restatement's: same flags,
same region, same line families -- a sample that took another decision is far outside the
tolerance. Measured figures: DESIGN.md 4.5c, profiles/colormap_viz.md.

Through pl_render_image the plot rect lies over a black part of the picture: whatever the
scaler and the f16 intermediate do to the picture, the colour that enters the colour map there
is exactly 0, and the restatement can be given it. (Along the rect's edge, as far as the
scaler's support reaches, the picture bleeds in: not compared.)
"""
import ctypes as C
import os

import numpy as np
import pytest

import colormap_viz_ref as V
import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

HDR10 = dict(primaries="bt2020", transfer="pq", max_luma=1000.0)


@pytest.fixture(scope="module")
def sdr709(built):
    return V.resolve(*V.spaces("bt709"))


def dispatch(gpu, img, target, tone="spline", prelinearized=False, tricubic=False, **viz):
    """pl_shader_color_map_ex on an rgba32f texture through pl_dispatch_finish -> frame, listing"""
    h, w = img.shape[:2]
    src = gpu.tex_create(w, h, "rgba32f", img)
    dst = gpu.tex_create(w, h, "rgba32f")
    state = pl.ShaderObj()
    params = pl.color_map_params(tone=tone, lut3d_tricubic=tricubic, **viz)
    sh = gpu.begin()
    assert sh.sample("nearest", src)
    sh.color_map(pl.color_space(**HDR10), pl.color_space(target, "bt1886"), state, params,
                 prelinearized=prelinearized)
    assert not sh.failed(), gpu.messages[-3:]
    listing = sh.listing()
    assert sh.finish(dst), gpu.messages[-3:]
    out = dst.download()
    state.destroy(); src.destroy(); dst.destroy()
    names = [ln.split("(")[0] for ln in listing.splitlines() if ln and not ln.startswith("#")]
    return out, [n for n in names if not n.startswith("sample")]


def hold(tag, got, img, r, where=None, **kw):
    """got (.., 3 or 4, values in 0 .. 1) against the restatement, per class, on the samples kept"""
    t, keep, r32 = V.compare(img, r, **kw)
    assert 1.0 - keep.mean() <= V.SET_ASIDE_CAP
    if where is not None:
        keep = keep & where
    tol = V.tolerance(r32)
    dist = np.abs(got[..., :3].astype(np.float64) - t["out"]).max(-1)
    worst = {}
    for c, bound in tol.items():
        sel = keep & (t["cls"] == c)
        if not sel.any():
            continue
        worst[c] = float(dist[sel].max())
        print("%s, %s: %d samples, R32 %.3g, bound %.3g, GPU %.3g (%.2f R32), median %.3g" %
              (tag, V.CLASS_NAMES[c], sel.sum(), r32[c], bound, worst[c],
               worst[c] / max(r32[c], 1e-30), float(np.median(dist[sel]))))
    late = {V.CLASS_NAMES[c]: (worst[c], tol[c]) for c in worst if worst[c] > tol[c]}
    assert not late, (tag, late)
    return t, keep


def test_show_clipping(gpu, sdr709):
    img, _ = V.clip_frame(sdr709)
    got, listing = dispatch(gpu, img, "bt709", prelinearized=True, show_clipping=True)
    assert listing == ["clip_test", "rgb2ipt", "clip_test", "tone_map", "clip_test", "gamut_lut",
                       "ipt2rgb", "clip_mark", "delinearize"]
    t, keep = hold("show_clipping", got, img, sdr709, show_clipping=True, prelinearized=True)
    assert all(v.sum() >= 32 for v in t["raised"].values()), {k: int(v.sum()) for k, v in t["raised"].items()}
    assert np.array_equal(got[..., 3], img[..., 3])
    # the marks are there: clip_hi pixels are the inverted-saturation colours, far from the plain map
    plain, _ = dispatch(gpu, img, "bt709", prelinearized=True)
    moved = np.abs(got[..., :3] - plain[..., :3]).max(-1) > 0.02
    assert moved[keep & (t["cls"] == V.CLIP_HI)].mean() > 0.9
    assert not moved[keep & (t["cls"] == V.UNMARKED)].any()


@pytest.mark.parametrize("tone", ["spline", "clip", "linear"])
def test_tone_plot_alone(gpu, tone):
    r = V.resolve(*V.spaces("bt2020"), tone=tone)
    img = V.picture(64, 64)
    got, listing = dispatch(gpu, img, "bt2020", tone=tone, visualize_lut=True)
    assert listing == ["linearize", "rgb2ipt", "tone_map", "ipt2rgb", "viz_tone", "delinearize"]
    hold("tone plot (%s)" % tone, got, img, r, visualize_lut=True)


def test_tone_plot_in_a_rect(gpu):
    r = V.resolve(*V.spaces("bt2020"))
    img = V.picture(96, 64)
    got, _ = dispatch(gpu, img, "bt2020", visualize_lut=True, visualize_rect=V.RECT_96x64)
    t, keep = hold("tone plot in a rect", got, img, r, visualize_lut=True, rect=V.RECT_96x64)
    # (outside the rect the plain colour map: the restatement's `unmarked` class above)
    assert t["in_rect"].sum() == 48 * 48 and (t["cls"][~t["in_rect"]] == V.UNMARKED).all()
    plain, _ = dispatch(gpu, img, "bt2020")
    assert np.abs(got[~t["in_rect"]] - plain[~t["in_rect"]]).max() < 1e-4
    assert np.abs(got[t["in_rect"]] - plain[t["in_rect"]]).max() > 0.05


@pytest.mark.parametrize("hue,theta,tricubic", [(*V.HUE_THETA[0], False), (*V.HUE_THETA[1], False),
                                                (*V.HUE_THETA[2], False), (*V.HUE_THETA[1], True)])
def test_gamut_and_tone_plot(gpu, hue, theta, tricubic):
    r = V.resolve(*V.spaces("bt709"), tricubic=tricubic)
    img = V.picture(64, 64)
    got, listing = dispatch(gpu, img, "bt709", tricubic=tricubic, visualize_lut=True,
                            visualize_hue=hue, visualize_theta=theta)
    assert listing == ["linearize", "rgb2ipt", "tone_map", "gamut_lut", "viz_gamut", "viz_gamut_src",
                       "viz_gamut_dst", "ipt2rgb", "viz_tone", "delinearize"]
    hold("gamut + tone plot (hue %g, theta %g%s)" % (hue, theta, ", tricubic" if tricubic else ""),
         got, img, r, visualize_lut=True, hue=hue, theta=theta)


def test_both_switches(gpu, sdr709):
    """the order: clipping colours first, the tone plot on top, the gamut plot inside the stage"""
    img, _ = V.clip_frame(sdr709, 96, 64)
    kw = dict(show_clipping=True, visualize_lut=True)
    got, listing = dispatch(gpu, img, "bt709", prelinearized=True, visualize_rect=V.RECT_96x64, **kw)
    assert listing == ["clip_test", "rgb2ipt", "clip_test", "tone_map", "clip_test", "gamut_lut",
                       "viz_gamut", "viz_gamut_src", "viz_gamut_dst", "ipt2rgb", "clip_mark",
                       "viz_tone", "delinearize"]
    t, _ = hold("both switches", got, img, sdr709, rect=V.RECT_96x64, prelinearized=True, **kw)
    assert {V.CLIP_HI, V.CLIP_LO, V.GAMUT_PLOT, V.UNMARKED} <= set(np.unique(t["cls"]))


# ---- through the renderer -------------------------------------------------------------------------
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


def frame_with_black_window(w, h, rect):
    """rgba16 PQ picture, black where `rect` (in units of the frame) lies"""
    img = (V.picture(w, h) * 65535.0).astype(np.uint16)
    img[..., 3] = 65535
    x0, y0, x1, y1 = rect
    img[int(round(y0 * h)):int(round(y1 * h)), int(round(x0 * w)):int(round(x1 * w)), :3] = 0
    return img


def render(gpu, capfd, img, dw, dh, peak, upscaler=True, mix=None, **viz):
    """one frame (a fresh renderer) -> frame, the passes' op lists (PL_HIP_PASS_TRACE), metadata"""
    kw = dict(dither_params=None, color_map_params=pl.color_map_params(**viz),
              peak_detect_params=pl.peak_detect_params(percentile=99.995) if peak else None)
    if upscaler:
        kw["upscaler"] = pl.filter_config("ewa_lanczos")
    params = pl.render_params("default", **kw)
    h, w = img.shape[:2]
    capfd.readouterr()
    with env(PL_HIP_PASS_TRACE="1"):
        rr = pl.Renderer(gpu)
        src = gpu.tex_create(w, h, "rgba16", img)
        dst = gpu.tex_create(dw, dh, "rgba16")
        image = pl.frame(src, components=3, color=pl.color_space(**HDR10))
        target = pl.frame(dst, color=pl.color_space("bt709", "bt1886"))
        assert rr.render(image, target, params), gpu.messages[-4:]
        assert rr.errors() == 0
        out = dst.download()
        meta = capi.HdrMetadata()
        pl.lib().pl_renderer_get_hdr_metadata(rr.rr, C.byref(meta))
        rr.destroy(); src.destroy(); dst.destroy()
    trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plh] pass")]
    passes = [(int(ln.split("sampler=")[1].split()[0]), [int(k) for k in ln.split("ops:")[1].split()])
              for ln in trace]
    return out, passes, meta


def codes_statement(tag, a, b):
    """what tests/test_gpu_default_kernels.py allows between the tuned and the generic kernels on an
    HDR frame behind the colour map (test_hdr_downscale_with_fused_pq_linearisation)"""
    d = np.abs(a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64))
    print("%s: |diff| codes: median %.1f p99 %.1f p99.9 %.1f max %d; > 8 codes on %.2e" %
          (tag, np.median(d), np.quantile(d, 0.99), np.quantile(d, 0.999), d.max(), (d > 8).mean()))
    assert np.quantile(d, 0.5) <= 1 and np.quantile(d, 0.99) <= 4 and np.quantile(d, 0.999) <= 16
    assert d.max() <= 256 and (d > 8).mean() < 2e-3


VIZ_OPS = set(range(36, 42))    # enum plh_op_kind: CLIP_TEST .. VIZ_TONE
POLAR = 7


@pytest.mark.parametrize("peak", [False, True])
@pytest.mark.parametrize("shape", ["ewa 2x", "1:1"])
def test_through_pl_render_image(gpu, capfd, shape, peak):
    if shape == "ewa 2x":
        (sw, sh), (dw, dh), reach = (64, 36), (128, 72), 8     # (ewa_lanczos: 3.24 texels = 7 pixels)
    else:
        (sw, sh), (dw, dh), reach = (64, 48), (64, 48), 0
    img = frame_with_black_window(sw, sh, V.RECT_96x64)
    viz = dict(visualize_lut=True, visualize_rect=V.RECT_96x64, visualize_hue=0.3, visualize_theta=0.8)
    plain, passes0, _ = render(gpu, capfd, img, dw, dh, peak, upscaler=shape == "ewa 2x")
    got, passes1, meta = render(gpu, capfd, img, dw, dh, peak, upscaler=shape == "ewa 2x", **viz)

    # with the switches off no pass carries one of the ops, and the colour map runs where it
    # always has: as the epilogue of the polar pass / in the one pass of the 1 : 1 frame
    assert not any(VIZ_OPS & set(ops) for _, ops in passes0), passes0
    cm0 = [(s, ops) for s, ops in passes0 if 20 in ops]
    assert len(cm0) == 1, passes0
    if not peak:    # (a measurement stores the scaled image first, as ever)
        assert (cm0[0][0] == POLAR) == (shape == "ewa 2x"), passes0
    # with them on, the pass that carries them is one the generic kernel's variant runs
    cm1 = [(s, ops) for s, ops in passes1 if VIZ_OPS & set(ops)]
    assert len(cm1) == 1 and cm1[0][0] < POLAR and 20 in cm1[0][1], passes1

    # the plot, where the picture is black as far as the scaler reaches
    src, dst = V.spaces("bt709")
    if peak:
        src.hdr.max_pq_y, src.hdr.avg_pq_y = meta.max_pq_y, meta.avg_pq_y
    r = V.resolve(src, dst)
    black = np.zeros((dh, dw, 4), np.float32)
    t = V.run(black, r, visualize_lut=True, rect=V.RECT_96x64, hue=0.3, theta=0.8)
    inner = np.zeros((dh, dw), bool)
    ys, xs = np.nonzero(t["in_rect"])
    inner[ys.min() + reach:ys.max() + 1 - reach, xs.min() + reach:xs.max() + 1 - reach] = True
    assert inner.sum() >= 1024
    hold("pl_render_image %s%s" % (shape, ", peak detection" if peak else ""), got / 65535.0, black, r,
         where=inner, unorm=True, visualize_lut=True, rect=V.RECT_96x64, hue=0.3, theta=0.8)
    assert np.abs(got[inner].astype(np.int64) - plain[inner]).max() > 2000

    # outside the rect: the frame rendered with both switches off
    outside = ~t["in_rect"]
    codes_statement("outside the rect, %s" % shape, got[outside], plain[outside])


def test_frame_mixing_does_not_reuse_across_a_switch(gpu, capfd):
    """the same two frames through pl_render_image_mix twice, show_clipping flipped in between: the
    parameter hash covers the switch, so the cached frames are rendered again, marked"""
    from test_gpu_mix import mixer
    w, h = 64, 48
    imgs = [(V.picture(w, h, seed=s) * 65535.0).astype(np.uint16) for s in (7, 8)]
    for img in imgs:
        img[..., :3] = np.minimum(img[..., :3].astype(np.int64) * 5 // 4, 65535)   # beyond 1000 nits
        img[..., 3] = 65535
    texs = [gpu.tex_create(w, h, "rgba16", img) for img in imgs]
    frames = [pl.frame(t, components=3, color=pl.color_space(**HDR10)) for t in texs]
    dst = gpu.tex_create(w, h, "rgba16")
    target = pl.frame(dst, color=pl.color_space("bt709", "bt1886"))
    rr = pl.Renderer(gpu)
    outs = []
    for clipping in (False, True, False):
        params = pl.render_params("fast", frame_mixer=mixer("linear"), dither_params=None,
                                  color_map_params=pl.color_map_params(show_clipping=clipping))
        assert rr.render_mix(frames, [11, 12], [-0.7, 0.3], 1.0, target, params), gpu.messages[-4:]
        assert rr.errors() == 0
        outs.append(dst.download())
    rr.destroy(); dst.destroy()
    for t in texs:
        t.destroy()
    assert np.array_equal(outs[0], outs[2])
    d = np.abs(outs[1][..., :3].astype(np.int64) - outs[0][..., :3]).max(-1)
    # the bright right-hand part of both pictures is beyond the source's declared peak: marked
    bright = (np.minimum(imgs[0][..., :3].max(-1), imgs[1][..., :3].max(-1)) > 0.80 * 65535)
    assert bright.sum() >= 32
    assert (d[bright] > 2000).mean() > 0.5, float((d[bright] > 2000).mean())
