"""pl_render_params.error_diffusion through pl_render_image (run_error_diffusion, rp_pick_dither).

The expected frame does not pass through run_error_diffusion. It comes from the UNDITHERED TWIN of
the render: the same image and parameters with error_diffusion = dither_params = NULL, into a
target of the renderer's intermediate format (rgba16hf; r16hf / rg16hf planes for a planar target)
with the same colour space, system and levels but no bit depths declared, so that
pl_color_repr_normalize is 1 and nothing dithers. (The encode of full-range RGB does not depend on
the depth; for limited-range YCbCr an undeclared depth means 8.) That twin is, texel for texel,
what the diffusion reads. The expectation is then

    orc.error_diffusion(twin, color_depth)  ->  half float  ->  * (1.0f / scale)  ->  the target's store

with scale = pl_color_repr_normalize of the target's repr. The diffusion runs on the image as the
last pass reads it, in the target's orientation (a rotated frame is recorded transposed, reference
src/renderer.c:2787-2793) but before a flipped target rectangle is applied (the flips are in the
rect of the final store, :2919-2924): for a flipped target the twin is un-flipped, diffused and
flipped back.

No case needed a reference composed by hand through the shader API. One needed another twin: the
chroma planes of a 4:2:0 target with left-sited chroma, of which the renderer diffuses one column
more than the plane stores (test_planar_target)."""
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util
from libplacebo_amd import _capi as capi
from test_gpu_errdiff import kernel_of, tallest_that_fits

pytestmark = pytest.mark.gpu

HALF = {"rgba8": "rgba16hf", "rgba16": "rgba16hf", "rg8": "rg16hf", "r8": "r16hf"}
EIGHT_BIT = dict(sample_depth=8, color_depth=8)
TEN_BIT = dict(sample_depth=16, color_depth=10, bit_shift=6)       # test_gpu_metric.ten_bit()
ORDERED = dict(method=pl.DITHER_ORDERED_FIXED, lut_size=6, transfer=0)
CHROMA_LEFT = 1
SHIFTS = ["sierra-lite", "floyd-steinberg", "stucki"]               # one kernel of each shift


def normalize(repr_):
    """pl_color_repr_normalize (pinned against the reference in test_tier0_ref.py), on a copy"""
    fn = pl.lib().pl_color_repr_normalize
    fn.restype = C.c_float
    copy = capi.ColorRepr.from_buffer_copy(repr_)
    return fn(C.byref(copy))


def params_for(preset, kernel, dither, **kw):
    """the preset with error_diffusion = the named kernel (or NULL) and dither_params = the
    ordered-fixed method (or NULL)"""
    k = pl.lib().pl_find_error_diffusion_kernel(kernel.encode()).contents if kernel else None
    return pl.render_params(preset, error_diffusion=k,
                            dither_params=capi.DitherParams(**ORDERED) if dither else None, **kw)


def render(gpu, image, planes, repr_, color, params, crop=None, rotation=0, chroma=None,
           init=None, rr=None):
    """One pl_render_image into fresh textures. planes: [(format, w, h, component mapping)].
    On a renderer of its own unless one is passed (debanding and peak detection depend on the
    renderer's frame count and history). -> ([plane as downloaded], pl_render_errors.errors)"""
    texs = [gpu.tex_create(w, h, fmt, None if init is None else init(fmt, w, h))
            for fmt, w, h, _ in planes]
    target = capi.Frame(num_planes=len(planes), repr=repr_, color=color, rotation=rotation)
    for i, (tex, (_, _, _, mapping)) in enumerate(zip(texs, planes)):
        target.planes[i].texture = tex.ptr
        target.planes[i].components = len(mapping)
        for c in range(4):
            target.planes[i].component_mapping[c] = mapping[c] if c < len(mapping) else -1
    if crop is not None:
        target.crop = capi.Rect2df(*crop)
    if chroma is not None:
        pl.lib().pl_frame_set_chroma_location.argtypes = [C.POINTER(capi.Frame), C.c_int]
        pl.lib().pl_frame_set_chroma_location(C.byref(target), chroma)
    own = rr is None
    rr = pl.Renderer(gpu) if own else rr
    try:
        assert rr.render(image, target, params), gpu.messages[-4:]
        return [t.download() for t in texs], rr.errors()
    finally:
        if own:
            rr.destroy()
        for t in texs:
            t.destroy()


def diffused(twin, half_fmt, dst_fmt, depth, kernel, scale, flip=(False, False)):
    """what the target plane must hold, from the twin plane (see the module's docstring)"""
    t = orc.tex_decode(twin, half_fmt)
    t = np.ascontiguousarray(t[::-1 if flip[1] else 1, ::-1 if flip[0] else 1])
    d = orc.op_quant_f16(orc.error_diffusion(t, depth, *kernel_of(kernel)))
    d = d * (np.float32(1.0) / np.float32(scale))
    assert d.dtype == np.float32
    return orc.tex_encode(np.ascontiguousarray(d[::-1 if flip[1] else 1, ::-1 if flip[0] else 1]), dst_fmt)


def on_grid(plane, fmt, depth, scale):
    """every sample a level of the depth, to the rounding of the two formats it went through: the
    half-float intermediate (half an ulp of a value below 1: 2^-12, a quarter of a 10-bit level)
    and the store (half a code of the format)"""
    dt, nc = pl._FMT_DTYPES[fmt]
    quant = (1 << depth) - 1
    v = orc.tex_decode(plane, fmt)[..., :min(nc, 3)].astype(np.float64) * float(np.float32(scale)) * quant
    return np.abs(v - np.rint(v)).max() <= quant * (2.0 ** -12 + 0.5 * scale / np.iinfo(dt).max) + 1e-3


def check(gpu, capfd, image, planes, repr_kw, kernel, preset="fast", color=None, crop=None,
          rotation=0, chroma=None, flip=(False, False), window=None, init=None, dither=(True, False),
          env=None, rr=None, twin_sizes=None, **kw):
    """The statement of this file for one frame: the render with error_diffusion set equals the
    diffusion of its undithered twin, with dither_params set and NULL alike; k_errdiff ran once per
    plane; no error bit; the frame is not the ordered-dither one; every sample is on the depth's grid.
    window: (x0, y0, x1, y1) of plane 0 that the image covers (the rest keeps `init`).
    twin_sizes: {plane: (w, h)} where the renderer diffuses more than the plane stores (the twin's
    plane then has that size, and the plane is the top left of its diffusion). -> the frame"""
    color = color if color is not None else pl.color_space("bt709", "srgb")
    bits = {k: v for k, v in repr_kw.items() if k in TEN_BIT}
    bare = {k: v for k, v in repr_kw.items() if k not in TEN_BIT}
    depth = bits["color_depth"]
    geo = dict(crop=crop, rotation=rotation, chroma=chroma)
    got = None
    with util.env(**(env or {})):
        sizes = twin_sizes or {}
        twin, errors = render(gpu, image, [(HALF[f], *sizes.get(i, (w, h)), m) for i, (f, w, h, m) in enumerate(planes)],
                              pl.color_repr(**bare), color, params_for(preset, None, False, **kw), **geo)
        assert errors == 0
        scale = normalize(pl.color_repr(**repr_kw))
        want = []
        for i, (t, (fmt, w, h, _)) in enumerate(zip(twin, planes)):
            x0, y0, x1, y1 = window if window and i == 0 else (0, 0, w, h)
            full = init(fmt, w, h).copy() if init else np.zeros((h, w, pl._FMT_DTYPES[fmt][1]), pl._FMT_DTYPES[fmt][0])
            if i in sizes:
                full[:] = diffused(t, HALF[fmt], fmt, depth, kernel, scale, flip)[:h, :w]
            else:
                full[y0:y1, x0:x1] = diffused(t[y0:y1, x0:x1], HALF[fmt], fmt, depth, kernel, scale, flip)
            want.append(full)
        ordered, _ = render(gpu, image, planes, pl.color_repr(**repr_kw), color,
                            params_for(preset, None, True, **kw), init=init, **geo)
        for with_dither in dither:
            with util.kernel_trace(capfd) as kernels:
                got, errors = render(gpu, image, planes, pl.color_repr(**repr_kw), color,
                                     params_for(preset, kernel, with_dither, **kw), init=init, rr=rr, **geo)
            assert errors == 0
            assert kernels.count("k_errdiff") == len(planes), kernels
            for i, (g, w_, (fmt, _, _, _)) in enumerate(zip(got, want, planes)):
                assert np.array_equal(g, w_), (i, with_dither, util.diff_stats(g, w_))
                assert on_grid(g, fmt, depth, scale), i
            assert any(not np.array_equal(g, o) for g, o in zip(got, ordered))
    return got


def chirp_image(gpu, w, h, **kw):
    src = gpu.tex_create(w, h, "rgba16", util.chirp_rgba16(w, h))
    return src, pl.frame(src, components=3, **kw)


@pytest.mark.parametrize("kernel", SHIFTS)
@pytest.mark.parametrize("fmt,bits", [("rgba8", EIGHT_BIT), ("rgba16", TEN_BIT)])
def test_plain_targets(gpu, capfd, kernel, fmt, bits):
    """fast preset, 1:1: one pass into the intermediate, the diffusion, the store"""
    w, h = 96, 70
    src, image = chirp_image(gpu, w, h)
    check(gpu, capfd, image, [(fmt, w, h, [0, 1, 2, 3])], dict(sys="rgb", levels="full", **bits), kernel)
    src.destroy()


def test_default_preset_upscaled(gpu, capfd):
    """default preset (separable upscale in sigmoidised linear light), 2x, 10 bit"""
    sw, sh = 48, 35
    csp = pl.color_space("bt709", "bt1886")
    src, image = chirp_image(gpu, sw, sh, color=csp)
    check(gpu, capfd, image, [("rgba16", 2 * sw, 2 * sh, [0, 1, 2, 3])],
          dict(sys="rgb", levels="full", **TEN_BIT), "floyd-steinberg", preset="default", color=csp)
    src.destroy()


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_high_quality_hdr10_to_sdr_upscaled(gpu, capfd, mfma):
    """high_quality, HDR10 -> BT.709, 2x polar upscale, 10 bit: the diffusion takes the image
    whichever polar kernel produced it (the matrix-pipe one or the sequential-fma one)"""
    from test_gpu_fullsize import hdr_frame16
    sw, sh = 48, 32
    src = gpu.tex_create(sw, sh, "rgba16", hdr_frame16(sw, sh))
    image = pl.frame(src, components=3, color=pl.color_space("bt2020", "pq", max_luma=1000.0))
    check(gpu, capfd, image, [("rgba16", 2 * sw, 2 * sh, [0, 1, 2, 3])],
          dict(sys="rgb", levels="full", **TEN_BIT), "sierra-lite", preset="high_quality",
          color=pl.color_space("bt709", "bt1886"), env={"PL_HIP_POLAR_MFMA": mfma}, dither=(True,))
    src.destroy()


def pattern(fmt, w, h):
    dt, nc = pl._FMT_DTYPES[fmt]
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((3 * x + 5 * y) % 200 + 20)[..., None], nc, axis=2).astype(dt)


def test_target_rect_inside_a_larger_target(gpu, capfd):
    """odd offsets; what lies outside the rect keeps what the target held"""
    w, h = 64, 48
    src, image = chirp_image(gpu, w, h)
    got = check(gpu, capfd, image, [("rgba8", 101, 71, [0, 1, 2, 3])], dict(sys="rgb", levels="full", **EIGHT_BIT),
                "floyd-steinberg", crop=(7, 5, 7 + w, 5 + h), window=(7, 5, 7 + w, 5 + h), init=pattern,
                skip_target_clearing=True)
    assert np.array_equal(got[0][:5], pattern("rgba8", 101, 71)[:5])
    src.destroy()


@pytest.mark.parametrize("axis", ["x", "y"])
def test_flipped_target_rect(gpu, capfd, axis):
    w, h = 64, 48
    src, image = chirp_image(gpu, w, h)
    crop = (w, 0, 0, h) if axis == "x" else (0, h, w, 0)
    check(gpu, capfd, image, [("rgba8", w, h, [0, 1, 2, 3])], dict(sys="rgb", levels="full", **EIGHT_BIT),
          "stucki", crop=crop, flip=(axis == "x", axis == "y"))
    src.destroy()


@pytest.mark.parametrize("quarter_turns", [1, 3])
def test_rotated_frame(gpu, capfd, quarter_turns):
    """A frame turned by 90 / 270 degrees is recorded transposed and stored through a flipped
    rect: a quarter turn clockwise is the transposition mirrored in x, three are the transposition
    mirrored in y (numpy: rot90(a, -1) == a.T[:, ::-1], rot90(a, 1) == a.T[::-1]). The diffusion
    runs on the transposed image, in the target's orientation, before that mirror."""
    w, h = 64, 40
    src, image = chirp_image(gpu, w, h)
    image.rotation = quarter_turns
    check(gpu, capfd, image, [("rgba8", h, w, [0, 1, 2, 3])], dict(sys="rgb", levels="full", **EIGHT_BIT),
          "sierra-lite", flip=(quarter_turns == 1, quarter_turns == 3))
    src.destroy()


@pytest.mark.parametrize("chroma", [None, CHROMA_LEFT])
@pytest.mark.parametrize("layout", ["nv12", "three planes"])
def test_planar_target(gpu, capfd, layout, chroma):
    """8-bit 4:2:0 from an RGB image: every plane is diffused on its own, at its own size, through
    the one- and two-component intermediates (one k_errdiff launch per plane), and the pooled
    FBOs suffice. With the chroma samples sited left, the chroma planes' rect is 0.25 .. 32.25
    texels: the renderer renders and diffuses 33 columns (reference src/renderer.c:2809-2828) and
    the store clips the last one, whose error has gone into columns 30 and 31. A twin plane of 32
    columns does not hold that column; one of 33 does (the subsampling ratio is still 1/2)."""
    w, h = 64, 48
    csp = pl.color_space("bt709", "bt1886")
    src, image = chirp_image(gpu, w, h, color=csp)
    planes = [("r8", w, h, [0]), ("rg8", w // 2, h // 2, [1, 2])] if layout == "nv12" else \
             [("r8", w, h, [0]), ("r8", w // 2, h // 2, [1]), ("r8", w // 2, h // 2, [2])]
    wider = {i: (w // 2 + 1, h // 2) for i in range(1, len(planes))} if chroma else None
    got = check(gpu, capfd, image, planes, dict(sys="bt709", levels="limited", **EIGHT_BIT), "floyd-steinberg",
                color=csp, chroma=chroma, twin_sizes=wider)
    # a picture, not a cleared plane: luma and both chroma components vary
    assert len(np.unique(got[0])) > 50
    chroma = np.concatenate(got[1:], axis=2)
    assert chroma.shape[2] == 2 and all(len(np.unique(chroma[..., c])) > 20 for c in range(2))
    src.destroy()


def test_alpha_is_carried_not_diffused(gpu, capfd):
    """(skip_target_clearing: otherwise the image is blended against the background and the
    target's alpha is 1)"""
    w, h = 64, 48
    img = util.random_rgba16(w, h, seed=6)
    src = gpu.tex_create(w, h, "rgba16", img)
    image = pl.frame(src, repr_=pl.color_repr("rgb", "full", alpha="independent"))
    got = check(gpu, capfd, image, [("rgba8", w, h, [0, 1, 2, 3])],
                dict(sys="rgb", levels="full", alpha="independent", **EIGHT_BIT), "burkes",
                skip_target_clearing=True)
    alpha = orc.tex_encode(orc.op_quant_f16(orc.tex_decode(img, "rgba16")), "rgba8")[..., 3]
    assert np.array_equal(got[0][..., 3], alpha) and len(np.unique(alpha)) > 200
    src.destroy()


def test_force_dither_at_sixteen_bits(gpu, capfd):
    """a declared depth of 16 is dithered (here: diffused) only under force_dither"""
    w, h = 64, 48
    src, image = chirp_image(gpu, w, h)
    planes = [("rgba16", w, h, [0, 1, 2, 3])]
    repr_kw = dict(sys="rgb", levels="full", sample_depth=16, color_depth=16)
    check(gpu, capfd, image, planes, repr_kw, "sierra-2", force_dither=True)
    color = pl.color_space("bt709", "srgb")
    with util.kernel_trace(capfd) as kernels:
        got, errors = render(gpu, image, planes, pl.color_repr(**repr_kw), color,
                             params_for("fast", "sierra-2", True))
    plain, _ = render(gpu, image, planes, pl.color_repr(**repr_kw), color, params_for("fast", None, False))
    assert errors == 0 and "k_errdiff" not in kernels
    assert np.array_equal(got[0], plain[0])
    src.destroy()


def fall_back_pair(gpu, capfd, limit, w):
    """The tallest frame whose ring fits `limit` bytes of LDS diffuses; one row more renders
    without k_errdiff and without an error bit (the reference only traces, src/renderer.c:
    2290-2295): as the ordered dither where dither_params is set, undithered where it is NULL."""
    kernel = "stucki"
    h, need = tallest_that_fits(kernel, limit)
    assert gpu.gpu.contents.glsl.max_shmem_size == limit
    repr_kw = dict(sys="rgb", levels="full", **EIGHT_BIT)
    color = pl.color_space("bt709", "srgb")
    frames = []
    for rows in (h, h + 1):
        src = gpu.tex_create(w, rows, "rgba16", util.random_rgba16(w, rows, seed=rows))
        image = pl.frame(src, components=3)
        planes = [("rgba8", w, rows, [0, 1, 2, 3])]
        if rows == h:
            frames.append(check(gpu, capfd, image, planes, repr_kw, kernel))
        else:
            for with_dither in (True, False):
                with util.kernel_trace(capfd) as kernels:
                    got, errors = render(gpu, image, planes, pl.color_repr(**repr_kw), color,
                                         params_for("fast", kernel, with_dither))
                same, _ = render(gpu, image, planes, pl.color_repr(**repr_kw), color,
                                 params_for("fast", None, with_dither))
                assert errors == 0 and "k_errdiff" not in kernels, kernels
                assert np.array_equal(got[0], same[0]), with_dither
                frames.append(got)
            assert not np.array_equal(frames[-1][0], frames[-2][0])      # ordered vs undithered
        src.destroy()
    return h, need


@pytest.mark.parametrize("limit", [16 * 1024, (453 + 2) * 36])
def test_fall_back_when_the_ring_does_not_fit(capfd, built, limit):
    """a pl_hip of its own with 16 KiB of shared memory -- and with exactly the 16380 bytes of the
    453-row ring: a ring that needs all there is still fits (reference: `shmem_req > max_shmem_size`
    disables, src/renderer.c:2291)"""
    with pl.HipGpu(0, max_shmem_size=limit) as small:
        assert fall_back_pair(small, capfd, limit, 8) == (453, (453 + 2) * 36)


def test_fall_back_on_the_whole_lds(gpu, capfd):
    assert fall_back_pair(gpu, capfd, 160 * 1024, 8) == (4549, (4549 + 2) * 36)


def test_one_renderer_across_changing_heights(capfd, built):
    """a frame that diffuses, one that falls back, the first again -- on one pl_renderer: the
    third equals the first and no error bit is latched by the fall-back"""
    with pl.HipGpu(0, max_shmem_size=16 * 1024) as small:
        h, _ = tallest_that_fits("stucki", 16 * 1024)
        rr = pl.Renderer(small)
        repr_ = pl.color_repr("rgb", "full", **EIGHT_BIT)
        color = pl.color_space("bt709", "srgb")
        outs = []
        for rows, runs in ((h, 1), (h + 1, 0), (h, 1)):
            src = small.tex_create(8, rows, "rgba16", util.random_rgba16(8, rows, seed=rows))
            with util.kernel_trace(capfd) as kernels:
                got, errors = render(small, pl.frame(src, components=3), [("rgba8", 8, rows, [0, 1, 2, 3])],
                                     repr_, color, params_for("fast", "stucki", True), rr=rr)
            assert errors == 0 and kernels.count("k_errdiff") == runs, (rows, errors, kernels)
            outs.append(got[0])
            src.destroy()
        assert np.array_equal(outs[2], outs[0])
        rr.destroy()
