"""pl_render_params.border = PL_CLEAR_BLUR: the bars of a cropped target filled with a blurred,
stretched copy of the frame (src/renderer.c:2345-2465 pass_blur, :2491-2553 clear_target), against
the numpy restatement in blur_ref.py. The targets are rgba16hf so that quantisation hides nothing;
the image is placed 1 : 1, so what lands inside the crop IS the image the pyramid starts from."""
import ctypes as C

import numpy as np
import pytest

import blur_ref
import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

BLUR = 3        # PL_CLEAR_BLUR
ERR_BLUR = 1 << 12


@pytest.fixture()
def rr(gpu):
    r = pl.Renderer(gpu)
    yield r
    r.destroy()


def image16f(w, h, seed=1):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([0.5 + 0.5 * np.sin(xx / max(w, 1) * 7 + k + yy / max(h, 1) * 3)
                     for k in range(3)], -1)
    img = np.empty((h, w, 4), np.float32)
    img[..., :3] = 0.8 * base + 0.2 * rng.random((h, w, 3))
    img[..., 3] = rng.random((h, w))
    return img.astype(np.float16)


class Passes:
    """the pass descriptions pl_render_params.info_callback sees"""

    def __init__(self, params):
        self.names = []

        def cb(_priv, info):
            self.names.append(info.contents.pass_.contents.shader.contents.description.decode())
        self.cb = capi.RENDER_INFO_CB(cb)
        params.info_callback = C.cast(self.cb, C.c_void_p)

    def blur(self):
        return sorted({n for n in self.names if n.startswith("blur ")})


def aspect_set(rect, aspect):
    lib = pl.lib()
    lib.pl_rect2df_aspect_set.argtypes = [C.POINTER(capi.Rect2df), C.c_float, C.c_float]
    r = capi.Rect2df(*rect)
    lib.pl_rect2df_aspect_set(C.byref(r), aspect, 0.0)
    return (r.x0, r.y0, r.x1, r.y1)


def render(gpu, rr, img, tw, th, crop, comps=3, frames=1, **kw):
    """img (float16) 1 : 1 into crop of a tw x th rgba16hf target; returns (ok, output, passes)"""
    h, w = img.shape[:2]
    src = gpu.tex_create(w, h, "rgba16hf", img)
    dst = gpu.tex_create(tw, th, "rgba16hf", np.full((th, tw, 4), 0.25, np.float16))
    image = pl.frame(src, components=comps)
    trepr = pl.color_repr("rgb", "full", alpha="independent") if comps == 4 else None
    target = pl.frame(dst, crop=crop, repr_=trepr)
    params = pl.render_params("fast", dither_params=None, **kw)
    passes = Passes(params)
    ok = True
    for _ in range(frames):     # (pass timings arrive once the GPU has finished a frame)
        ok = rr.render(image, target, params) and ok
        out = dst.download().astype(np.float32)
    src.destroy(); dst.destroy()
    return ok, out, passes


def border_of(out, crop):
    x0, y0, x1, y1 = (int(round(v)) for v in crop)
    x0, x1 = sorted((x0, x1))
    y0, y1 = sorted((y0, y1))
    mask = np.ones(out.shape[:2], bool)
    mask[y0:y1, x0:x1] = False
    inside = out[y0:y1, x0:x1]
    return mask, inside


def expected_border(inside, radius, tw, th):
    h, w = inside.shape[:2]
    border = blur_ref.pyramid(inside, radius)
    rect = aspect_set((0, 0, w, h), tw / th)
    return blur_ref.to_f16(blur_ref.border_sample(border, rect, tw, th))


def f16_ulps(a, b):
    ia = a.astype(np.float16).view(np.int16).astype(np.int64)
    ib = b.astype(np.float16).view(np.int16).astype(np.int64)
    return np.abs(ia - ib)


def check_border(got, exp, mask):
    g, e = got[mask], exp[mask]
    same = (g == e).mean()
    ulps = f16_ulps(g, e).max()
    assert same >= 0.999 and ulps <= 1, (same, ulps)


@pytest.mark.parametrize("size", [(32, 24, 64, 48, (16, 12, 48, 36)),
                                  (3840, 1600, 3840, 2160, (0, 280, 3840, 1880))])
def test_letterbox_border_is_the_blurred_frame(gpu, rr, size):
    w, h, tw, th, crop = size
    img = image16f(w, h)
    ok, out, passes = render(gpu, rr, img, tw, th, crop, border=BLUR, frames=2)
    assert ok and rr.errors() == 0, gpu.messages[-4:]
    mask, inside = border_of(out, crop)
    ok, ref, _ = render(gpu, rr, img, tw, th, crop)
    assert ok
    _, ref_inside = border_of(ref, crop)
    assert np.array_equal(inside, ref_inside)
    # the flat background colour in the bars is what this feature replaces
    assert not np.array_equal(out[mask], ref[mask])
    check_border(out, expected_border(inside, 16.0, tw, th), mask)

    n, _, levels, up = blur_ref.plan(16.0, w, h)
    assert passes.blur() == sorted([f"blur downscale pass {i + 1}" for i in range(n)] +
                                   [f"blur upscale pass {i + 1}" for i in range(n)]), passes.names
    assert "draw border" in passes.names


@pytest.mark.parametrize("w,h,radius", [(32, 24, 0.0), (1, 1, 16.0), (6, 3, 16.0), (5, 1, 64.0),
                                        (20, 12, 1000.0), (17, 9, 2.0)])
def test_small_images_and_no_radius(gpu, rr, w, h, radius):
    """r = 0: the image itself, stretched; a 1 x 1 image; pyramids that reach 1 x 1 early"""
    tw, th = 2 * w + 6, 2 * h + 4
    crop = (3, 2, 3 + w, 2 + h)
    img = image16f(w, h, seed=w * h)
    ok, out, passes = render(gpu, rr, img, tw, th, crop, border=BLUR, blur_radius=radius, frames=2)
    assert ok and rr.errors() == 0, gpu.messages[-4:]
    mask, inside = border_of(out, crop)
    check_border(out, expected_border(inside, radius, tw, th), mask)
    n, _, _, up = blur_ref.plan(radius, w, h)
    assert len(passes.blur()) == n * (2 if up else 1), passes.names


def test_four_components_and_flipped_crop(gpu, rr):
    w, h, tw, th = 40, 20, 64, 48
    img = image16f(w, h, seed=7)
    crop = (52, 34, 12, 14)     # flipped on both axes
    ok, out, _ = render(gpu, rr, img, tw, th, crop, comps=4, border=BLUR, background=2, frames=1)
    assert ok and rr.errors() == 0, gpu.messages[-4:]
    mask, inside = border_of(out, crop)
    border = blur_ref.pyramid(inside[::-1, ::-1], 16.0)
    rect = aspect_set((0, 0, w, h), tw / th)
    rect = (rect[2], rect[3], rect[0], rect[1])
    exp = blur_ref.to_f16(blur_ref.border_sample(border, rect, tw, th))
    check_border(out, exp, mask)


def test_nv12_target_gets_swizzled_rgb(gpu, rr):
    """a YCbCr target receives the blurred RGB, swizzled, without encoding (the reference's
    clear_target): the luma plane's border holds R, the chroma plane's G and B"""
    w, h, tw, th = 32, 16, 64, 48
    img = image16f(w, h, seed=3)
    src = gpu.tex_create(w, h, "rgba16hf", img)
    ty, tuv = gpu.tex_create(tw, th, "r16hf"), gpu.tex_create(tw // 2, th // 2, "rg16hf")
    f = capi.Frame(num_planes=2)
    f.planes[0].texture, f.planes[0].components = ty.ptr, 1
    f.planes[1].texture, f.planes[1].components = tuv.ptr, 2
    for c in range(4):
        f.planes[0].component_mapping[c] = 0 if c == 0 else -1
        f.planes[1].component_mapping[c] = c + 1 if c < 2 else -1
    f.repr = pl.color_repr("bt709", "full")
    f.color = pl.color_space("bt709", "srgb")
    f.crop = capi.Rect2df(16, 16, 48, 32)
    params = pl.render_params("fast", dither_params=None, border=BLUR)
    assert rr.render(pl.frame(src, components=3), f, params), gpu.messages[-4:]
    assert rr.errors() == 0
    y = ty.download().astype(np.float32)[..., 0]
    # the blurred frame is what the reference blurs: the image converted to the target's RGB
    # (here the same), sampled over the plane; the top rows are border only
    border = blur_ref.pyramid(img.astype(np.float32), 16.0)
    exp = blur_ref.to_f16(blur_ref.border_sample(border, aspect_set((0, 0, w, h), tw / th), tw, th))
    assert f16_ulps(y[:16], exp[:16, :, 0]).max() <= 1
    uv = tuv.download().astype(np.float32)
    exp2 = blur_ref.to_f16(blur_ref.border_sample(border, aspect_set((0, 0, w, h), tw / th),
                                                  tw // 2, th // 2))
    assert f16_ulps(uv[:8], exp2[:8, :, 1:3]).max() <= 1
    for t in (src, ty, tuv):
        t.destroy()


def test_frame_mixing_draws_the_blurred_border(gpu, rr):
    w, h, tw, th = 48, 20, 64, 48
    crop = (8, 14, 56, 34)
    imgs = [image16f(w, h, seed=s) for s in (11, 12)]
    srcs = [gpu.tex_create(w, h, "rgba16hf", i) for i in imgs]
    dst = gpu.tex_create(tw, th, "rgba16hf")
    target = pl.frame(dst, crop=crop)
    mixer = capi.FilterConfig()
    C.memmove(C.byref(mixer), C.byref(pl.filter_config("linear", pl.FILTER_FRAME_MIXING)),
              C.sizeof(mixer))
    params = pl.render_params("fast", dither_params=None, border=BLUR, frame_mixer=mixer)
    frames = [pl.frame(s, components=3) for s in srcs]
    assert rr.render_mix(frames, [1, 2], [-0.4, 0.6], 1.0, target, params), gpu.messages[-4:]
    assert rr.errors() == 0
    out = dst.download().astype(np.float32)
    mask, inside = border_of(out, crop)
    assert np.abs(out[mask][:, :3]).max() > 0.1     # (not the black background colour)
    check_border(out, expected_border(inside, 16.0, tw, th), mask)
    for t in srcs + [dst]:
        t.destroy()


def test_without_fbos_the_render_fails(gpu, rr):
    img = image16f(16, 8)
    ok, _, _ = render(gpu, rr, img, 32, 24, (8, 8, 24, 16), border=BLUR, disable_fbos=True)
    assert not ok
    assert any("Output requires blurred borders, but FBOs are unavailable" in m
               for _, m in gpu.messages[-8:]), gpu.messages[-8:]


def test_uncropped_target_draws_no_border(gpu, rr):
    img = image16f(32, 24)
    ok, out, passes = render(gpu, rr, img, 32, 24, None, border=BLUR, frames=2)
    assert ok and rr.errors() == 0
    assert passes.blur() == [] and "draw border" not in passes.names, passes.names
    ok, ref, _ = render(gpu, rr, img, 32, 24, None)
    assert ok and np.array_equal(out, ref)


def opaque16f(w, h, seed=1):
    img = image16f(w, h, seed)
    img[..., 3] = 1.0
    return img


def test_border_with_distortion_samples_the_undistorted_image(gpu, rr):
    """the border is taken before distortion and drawn from the rect of the image it was taken
    from (the distorted canvas is another size): a quarter turn of a 4 : 3 frame"""
    w, h, tw, th = 32, 24, 128, 48
    crop = (48, 12, 80, 36)
    img = opaque16f(w, h, seed=5)
    ok, out, _ = render(gpu, rr, img, tw, th, crop, border=BLUR,
                        distort_params=pl.distort_params(mat=((0, -1), (1, 0))))
    assert ok and rr.errors() == 0, gpu.messages[-4:]
    border = blur_ref.pyramid(img.astype(np.float32), 16.0)
    exp = blur_ref.to_f16(blur_ref.border_sample(border, aspect_set((0, 0, w, h), tw / th), tw, th))
    mask = np.zeros((th, tw), bool)
    mask[:, :40] = mask[:, 88:] = True      # (the turned image covers columns 52 .. 76 at most)
    check_border(out, exp, mask)


def test_rotated_image_border_is_transposed(gpu, rr):
    """a quarter-turned image: the border pass is transposed and aspect-set to the swapped plane"""
    w, h, tw, th = 24, 32, 64, 48
    crop = (16, 12, 48, 36)
    img = opaque16f(w, h, seed=9)
    src = gpu.tex_create(w, h, "rgba16hf", img)
    dst = gpu.tex_create(tw, th, "rgba16hf")
    image = pl.frame(src, components=3)
    image.rotation = 1      # PL_ROTATION_90
    target = pl.frame(dst, crop=crop)
    assert rr.render(image, target, pl.render_params("fast", dither_params=None, border=BLUR)), \
        gpu.messages[-4:]
    assert rr.errors() == 0
    out = dst.download().astype(np.float32)
    mask, _ = border_of(out, crop)
    border = blur_ref.pyramid(img.astype(np.float32), 16.0)
    s = blur_ref.to_f16(blur_ref.border_sample(border, aspect_set((0, 0, w, h), th / tw), th, tw))
    check_border(out, s.transpose(1, 0, 2), mask)
    src.destroy(); dst.destroy()


def test_blended_border(gpu, rr):
    """blend_params: the border's colour (alpha kept, only rgb scaled) blended over the target's
    content, like the image"""
    w, h, tw, th = 32, 24, 64, 48
    crop = (16, 12, 48, 36)
    img = image16f(w, h, seed=13)
    blend = capi.BlendParams(src_rgb=pl.BLEND_SRC_ALPHA, dst_rgb=pl.BLEND_ONE_MINUS_SRC_ALPHA,
                             src_alpha=pl.BLEND_ONE, dst_alpha=pl.BLEND_ONE_MINUS_SRC_ALPHA)
    ok, out, _ = render(gpu, rr, img, tw, th, crop, comps=4, border=BLUR, background=2,
                        blend_params=blend)
    assert ok and rr.errors() == 0, gpu.messages[-4:]
    mask, _ = border_of(out, crop)
    b = blur_ref.border_sample(blur_ref.pyramid(img.astype(np.float32), 16.0),
                               aspect_set((0, 0, w, h), tw / th), tw, th)
    a = b[..., 3:]
    exp = np.concatenate([b[..., :3] * a + np.float32(0.25) * (1 - a),
                          a + np.float32(0.25) * (1 - a)], -1)
    assert np.abs(out[mask] - exp[mask]).max() <= 2e-3
    # (not what the plain border gives)
    assert np.abs(out[mask] - blur_ref.to_f16(b)[mask]).max() > 1e-2
