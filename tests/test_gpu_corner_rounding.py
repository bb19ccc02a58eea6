"""pl_render_params.corner_rounding (src/renderer.c:2615-2652): the image's corners fade out over
two pixels of a rounded rect the size of the target crop, through the image's alpha, and the
output's premultiply / background logic shows the background there. Against a float64 statement
of the mask applied to the image, within one code of 16 bits."""
import ctypes as C
import os

import numpy as np
import pytest

import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

SKIP, COLOR, TILES = 2, 0, 1
CODE = 1.0 / 65535


@pytest.fixture()
def rr(gpu):
    r = pl.Renderer(gpu)
    yield r
    r.destroy()


def corner_mask(w, h, crop_w, crop_h, rounding):
    """border per pixel of a w x h pass over a crop of crop_w x crop_h"""
    w2, h2 = abs(crop_w) / 2.0, abs(crop_h) / 2.0
    radius = min(rounding, 1.0) * min(w2, h2)
    x = -w2 + (np.arange(w) + 0.5) / w * 2 * w2
    y = -h2 + (np.arange(h) + 0.5) / h * 2 * h2
    rx = np.maximum(np.abs(x)[None, :] - w2 + radius, 0)
    ry = np.maximum(np.abs(y)[:, None] - h2 + radius, 0)
    rdist = np.sqrt(rx * rx + ry * ry) - radius
    t = np.clip((rdist - 2.0) / -2.0, 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def image(w, h, seed=1):
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 4)) * 0.8 + 0.1
    return img.astype(np.float16)


@pytest.mark.parametrize("rounding", [0.25, 1.0, 2.0])
@pytest.mark.parametrize("alpha", ["none", "independent", "premultiplied"])
@pytest.mark.parametrize("background", [COLOR, SKIP, TILES])
def test_corners_follow_the_mask(gpu, rr, rounding, alpha, background):
    w, h, tw, th = 48, 32, 64, 48
    crop = (8, 8, 8 + w, 8 + h)
    img = image(w, h, seed=int(rounding * 4))
    src = gpu.tex_create(w, h, "rgba16hf", img)
    dst = gpu.tex_create(tw, th, "rgba16")
    comps = 3 if alpha == "none" else 4
    irepr = pl.color_repr("rgb", "full", alpha=alpha if comps == 4 else "unknown")
    tre = pl.color_repr("rgb", "full", alpha="independent")
    image_f = pl.frame(src, components=comps, repr_=irepr)
    target = pl.frame(dst, crop=crop, repr_=tre)
    kw = dict(dither_params=None, corner_rounding=rounding, background=background,
              border=SKIP)
    assert rr.render(image_f, target, pl.render_params("fast", **kw)), gpu.messages[-4:]
    assert rr.errors() == 0
    got = dst.download().astype(np.float64)[8:8 + h, 8:8 + w] / 65535
    if background == TILES:
        # the tiles show through where the mask fades (alpha 1 out); where it is 1 the frame is the
        # one with square corners
        kw["corner_rounding"] = 0.0
        assert rr.render(image_f, target, pl.render_params("fast", **kw))
        sq = dst.download().astype(np.float64)[8:8 + h, 8:8 + w] / 65535
        m = corner_mask(w, h, w, h, rounding)
        assert np.abs(got[m == 1] - sq[m == 1]).max() <= 1.5 * CODE
        assert np.abs(got[..., 3] - 1.0).max() <= CODE
        if (m == 0).any():
            assert np.abs(got[m == 0][:, :3] - sq[m == 0][:, :3]).max() > 0.05
    else:
        m = corner_mask(w, h, w, h, rounding)
        f = img.astype(np.float64)
        rgb, a = f[..., :3], f[..., 3] if comps == 4 else np.ones((h, w))
        if alpha == "premultiplied":
            rgb_straight = rgb / np.maximum(a, 1e-6)[..., None]
        else:
            rgb_straight = rgb
        a2 = a * m
        if background == COLOR:       # premultiplied, blended against black, alpha 1
            exp = np.concatenate([rgb_straight * a2[..., None], np.ones((h, w, 1))], -1)
        else:                         # skipped: independent alpha out
            exp = np.concatenate([rgb_straight, a2[..., None]], -1)
            exp[..., :3] = np.where(a2[..., None] > 1e-6, exp[..., :3], got[..., :3])
        exp = np.clip(exp, 0, 1)
        assert np.abs(got - exp).max() <= 1.5 * CODE, np.abs(got - exp).max() * 65535
    src.destroy(); dst.destroy()


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_corners_on_the_default_matrix_pipe_upscale(gpu, rr, mfma):
    """an exact 2x EWA upscale, whose default kernel is the matrix-pipe one: the corner op is
    carried (not dropped by a specialised epilogue)"""
    w, h = 48, 32
    img = image(w, h, seed=3)
    img[..., 3] = 1.0
    old = os.environ.get("PL_HIP_POLAR_MFMA")
    os.environ["PL_HIP_POLAR_MFMA"] = mfma
    try:
        src = gpu.tex_create(w, h, "rgba16hf", img)
        dst = gpu.tex_create(2 * w, 2 * h, "rgba16hf")
        kw = dict(dither_params=None, upscaler=pl.filter_config("ewa_lanczos"))
        image_f, target = pl.frame(src, components=3), pl.frame(dst)
        r = pl.Renderer(gpu)
        assert r.render(image_f, target, pl.render_params("fast", **kw)), gpu.messages[-4:]
        ref = dst.download().astype(np.float64)
        assert r.render(image_f, target, pl.render_params("fast", corner_rounding=1.0, **kw))
        assert r.errors() == 0
        got = dst.download().astype(np.float64)
        r.destroy()
    finally:
        if old is None:
            os.environ.pop("PL_HIP_POLAR_MFMA", None)
        else:
            os.environ["PL_HIP_POLAR_MFMA"] = old
    m = corner_mask(2 * w, 2 * h, 2 * w, 2 * h, 1.0)[..., None]
    exp = ref[..., :3] * m      # against the black background colour
    assert np.abs(got[..., :3] - exp).max() <= 2e-3
    assert got[0, 0, :3].max() <= 2e-3 and (m < 0.5).sum() > 100
    src.destroy(); dst.destroy()
