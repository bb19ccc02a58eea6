"""pl_shader_deinterlace and pl_render_params.deinterlace_params against the oracle's restatement
of src/shaders/deinterlacing.c. No transcendental anywhere: bit-exact, for every algorithm, field
order, set of neighbouring frames, texel format and the sizes where the mirrored borders and the
last odd row matter."""
import ctypes as C
import itertools

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

ALGOS = {"weave": pl.DEINTERLACE_WEAVE, "bob": pl.DEINTERLACE_BOB,
         "yadif": pl.DEINTERLACE_YADIF, "bwdif": pl.DEINTERLACE_BWDIF}


@pytest.fixture()
def rr(gpu):
    r = pl.Renderer(gpu)
    yield r
    r.destroy()


def frames(w, h, fmt, n=3, seed=0):
    """n consecutive frames of a moving pattern (so that the temporal terms are all live) as
    texel arrays of `fmt`"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        img = np.zeros((h, w, 4), np.float32)
        for c in range(4):
            img[..., c] = 0.5 + 0.35 * np.sin((xx + 3 * t) * (0.31 + 0.07 * c) + yy * 0.23 * (c + 1)) \
                          + 0.1 * rng.random((h, w))
        img[h // 3:, : w // 2, :] += 0.2 * ((xx[h // 3:, : w // 2, None] + t) % 5 == 0)   # combing
        out.append(orc.tex_encode(np.clip(img, 0, 1), fmt))
    return out


@pytest.mark.parametrize("fmt", ["r8", "rg8", "rgba8", "r16", "rgba16", "rgba16hf", "rgba32f"])
@pytest.mark.parametrize("algo", ["bob", "yadif", "bwdif"])
def test_every_algorithm_on_every_format(gpu, fmt, algo):
    w, h = 70, 37          # odd height: the last row has no partner; widths off the block size
    arr = frames(w, h, fmt)
    tex = [gpu.tex_create(w, h, fmt, a) for a in arr]
    dec = [orc.tex_decode(a, fmt) for a in arr]
    dst = gpu.tex_create(w, h, "rgba32f")
    ncomp = arr[0].shape[2] if arr[0].ndim == 3 else 1
    for field, first in itertools.product((pl.FIELD_TOP, pl.FIELD_BOTTOM), repeat=2):
        sh = gpu.begin()
        sh.deinterlace(tex[1], tex[0], tex[2], field=field, first_field=first, algo=ALGOS[algo])
        assert sh.finish(dst), gpu.messages[-4:]
        got = dst.download()
        ref = orc.deinterlace(dec[1], dec[0], dec[2], field, first, ALGOS[algo],
                              comp_mask=(1 << ncomp) - 1)
        assert np.array_equal(got, ref), (field, first, util.diff_stats(got, ref))
    for t in tex + [dst]:
        t.destroy()


@pytest.mark.parametrize("algo", ["yadif", "bwdif"])
@pytest.mark.parametrize("have", [(False, False), (True, False), (False, True)])
def test_missing_neighbours(gpu, algo, have):
    """No previous and / or next frame: the current one stands in (yadif), or bwdif falls back to
    its spatial filter where the frame it needs is the missing one (:79-83)."""
    w, h = 48, 32
    arr = frames(w, h, "rgba16", seed=3)
    tex = [gpu.tex_create(w, h, "rgba16", a) for a in arr]
    dec = [orc.tex_decode(a, "rgba16") for a in arr]
    dst = gpu.tex_create(w, h, "rgba32f")
    for field, first in itertools.product((pl.FIELD_TOP, pl.FIELD_BOTTOM), repeat=2):
        sh = gpu.begin()
        sh.deinterlace(tex[1], tex[0] if have[0] else None, tex[2] if have[1] else None,
                       field=field, first_field=first, algo=ALGOS[algo])
        assert sh.finish(dst), gpu.messages[-4:]
        got = dst.download()
        ref = orc.deinterlace(dec[1], dec[0] if have[0] else None, dec[2] if have[1] else None,
                              field, first, ALGOS[algo])
        assert np.array_equal(got, ref), (field, first, util.diff_stats(got, ref))
    for t in tex + [dst]:
        t.destroy()


@pytest.mark.parametrize("size", [(1, 1), (1, 2), (2, 1), (3, 3), (5, 2), (64, 8), (65, 9), (200, 3)])
def test_tiny_and_ragged_sizes(gpu, size):
    """frames smaller than the stencil: everything comes from the mirrored borders"""
    w, h = size
    arr = frames(w, h, "rgba16", seed=5)
    tex = [gpu.tex_create(w, h, "rgba16", a) for a in arr]
    dec = [orc.tex_decode(a, "rgba16") for a in arr]
    dst = gpu.tex_create(w, h, "rgba32f")
    for algo in ("bob", "yadif", "bwdif"):
        for field in (pl.FIELD_TOP, pl.FIELD_BOTTOM):
            sh = gpu.begin()
            sh.deinterlace(tex[1], tex[0], tex[2], field=field, algo=ALGOS[algo])
            assert sh.finish(dst), gpu.messages[-4:]
            got = dst.download()
            ref = orc.deinterlace(dec[1], dec[0], dec[2], field, pl.FIELD_TOP, ALGOS[algo])
            assert np.array_equal(got, ref), (algo, field, util.diff_stats(got, ref))
    for t in tex + [dst]:
        t.destroy()


def test_weave_no_field_mask_and_skip_spatial_check(gpu):
    w, h = 40, 24
    arr = frames(w, h, "rgba16", seed=7)
    tex = [gpu.tex_create(w, h, "rgba16", a) for a in arr]
    dec = [orc.tex_decode(a, "rgba16") for a in arr]
    dst = gpu.tex_create(w, h, "rgba32f")
    cases = [
        dict(field=pl.FIELD_TOP, algo=pl.DEINTERLACE_WEAVE),
        dict(field=pl.FIELD_NONE, algo=pl.DEINTERLACE_YADIF),               # sampled as it is
        dict(field=pl.FIELD_BOTTOM, algo=pl.DEINTERLACE_YADIF, skip_spatial_check=True),
        dict(field=pl.FIELD_TOP, algo=pl.DEINTERLACE_BWDIF, component_mask=0b0110),
        dict(field=pl.FIELD_TOP, first_field=pl.FIELD_NONE, algo=pl.DEINTERLACE_YADIF),   # = top
    ]
    for kw in cases:
        sh = gpu.begin()
        sh.deinterlace(tex[1], tex[0], tex[2], **kw)
        assert sh.finish(dst), gpu.messages[-4:]
        got = dst.download()
        ref = orc.deinterlace(dec[1], dec[0], dec[2], kw["field"], kw.get("first_field", pl.FIELD_TOP),
                              kw["algo"], kw.get("skip_spatial_check", False),
                              kw.get("component_mask", 0xf) or 0xf)
        assert np.array_equal(got, ref), (kw, util.diff_stats(got, ref))
    for t in tex + [dst]:
        t.destroy()


def test_colour_ops_run_behind_the_sampler_and_rects_flip(gpu):
    """The deinterlacer is a sampling stage like any other: colour ops follow it in the same pass,
    and the pass may land mirrored in a sub-rect of its target."""
    w, h = 48, 30
    arr = frames(w, h, "rgba16", seed=9)
    tex = [gpu.tex_create(w, h, "rgba16", a) for a in arr]
    dec = [orc.tex_decode(a, "rgba16") for a in arr]
    dst = gpu.tex_create(64, 40, "rgba16")
    under = util.random_rgba16(64, 40, seed=2)
    dst.upload(under)
    sh = gpu.begin()
    sh.deinterlace(tex[1], tex[0], tex[2], field=pl.FIELD_BOTTOM, algo=pl.DEINTERLACE_YADIF)
    pl.lib().plh_test_op_scale.argtypes = [C.c_void_p, C.c_float]
    pl.lib().plh_test_op_scale(sh.sh, C.c_float(0.5))
    assert sh.finish(dst, rect=(56, 35, 8, 5)), gpu.messages[-4:]      # flipped both ways
    got = dst.download()
    ref = orc.deinterlace(dec[1], dec[0], dec[2], pl.FIELD_BOTTOM, pl.FIELD_TOP, orc.DEINT_YADIF)
    ref = orc.op_scale(ref, 0.5)
    want = under.copy()
    want[5:35, 8:56] = orc.tex_encode(ref, "rgba16")[::-1, ::-1]
    assert np.array_equal(got, want), util.diff_stats(got, want)
    # a size other than the frame's is refused, as the reference's sh_require does
    sh = gpu.begin()
    sh.deinterlace(tex[1], field=pl.FIELD_TOP, algo=pl.DEINTERLACE_BOB)
    assert not sh.finish(dst), "a deinterlacing pass has the size of its frame"
    for t in tex + [dst]:
        t.destroy()


def interlaced_frame(gpu, texs, field, first=pl.FIELD_TOP, prev=None, nxt=None, **kw):
    f = pl.frame(texs, **kw) if not isinstance(texs, capi.Frame) else texs
    f.field, f.first_field = field, first
    f._refs = (prev, nxt)
    f.prev = C.cast(C.pointer(prev), C.c_void_p) if prev is not None else None
    f.next = C.cast(C.pointer(nxt), C.c_void_p) if nxt is not None else None
    return f


@pytest.mark.parametrize("algo", ["bob", "yadif", "bwdif"])
def test_renderer_deinterlaces_a_packed_frame(gpu, rr, algo):
    """pl_render_image with deinterlace_params: the plane is deinterlaced before anything else
    (src/renderer.c:1591-1612), the rest of the frame is what it would be for the deinterlaced
    picture -- here a 1:1 sRGB passthrough into 16 bits, so the frame IS the oracle's."""
    w, h = 64, 40
    arr = frames(w, h, "rgba16", seed=11)
    tex = [gpu.tex_create(w, h, "rgba16", a) for a in arr]
    dec = [orc.tex_decode(a, "rgba16") for a in arr]
    dst = gpu.tex_create(w, h, "rgba16")
    params = pl.render_params("fast", dither_params=None,
                              deinterlace_params=capi.DeinterlaceParams(ALGOS[algo], False))
    prev, nxt = pl.frame(tex[0], components=3), pl.frame(tex[2], components=3)
    for field, first in ((pl.FIELD_TOP, pl.FIELD_TOP), (pl.FIELD_BOTTOM, pl.FIELD_TOP),
                         (pl.FIELD_TOP, pl.FIELD_BOTTOM)):
        image = interlaced_frame(gpu, tex[1], field, first, prev, nxt, components=3)
        assert rr.render(image, pl.frame(dst), params), gpu.messages[-4:]
        assert rr.errors() == 0, gpu.messages[-4:]
        got = dst.download()
        ref = orc.deinterlace(dec[1], dec[0], dec[2], field, first, ALGOS[algo], comp_mask=0x7)
        ref[..., 3] = 1.0
        want = orc.tex_encode(ref, "rgba16")
        assert np.array_equal(got, want), (field, first, util.diff_stats(got, want))
    # without deinterlace_params the frame is shown woven
    image = interlaced_frame(gpu, tex[1], pl.FIELD_TOP, pl.FIELD_TOP, prev, nxt, components=3)
    assert rr.render(image, pl.frame(dst), pl.render_params("fast", dither_params=None))
    woven = dec[1].copy()
    woven[..., 3] = 1.0
    assert np.array_equal(dst.download(), orc.tex_encode(woven, "rgba16"))
    for t in tex + [dst]:
        t.destroy()


def nv12_frame(gpu, y, uv, luma_fmt="r8"):
    ty = gpu.tex_create(y.shape[1], y.shape[0], luma_fmt, y)
    tuv = gpu.tex_create(uv.shape[1], uv.shape[0], "rg8", uv)
    f = capi.Frame(num_planes=2)
    f.planes[0].texture, f.planes[0].components = ty.ptr, 1
    f.planes[1].texture, f.planes[1].components = tuv.ptr, 2
    for c in range(4):
        f.planes[0].component_mapping[c] = 0 if c == 0 else -1
        f.planes[1].component_mapping[c] = c + 1 if c < 2 else -1
    f.repr = pl.color_repr("bt709", "limited", sample_depth=8, color_depth=8)
    f.color = pl.color_space("bt709", "bt1886")
    pl.lib().pl_frame_set_chroma_location.argtypes = [C.POINTER(capi.Frame), C.c_int]
    pl.lib().pl_frame_set_chroma_location(C.byref(f), 1)
    f._tex = (ty, tuv)
    return f


@pytest.mark.parametrize("algo", ["bob", "yadif", "bwdif"])
def test_renderer_deinterlaces_every_plane_of_interlaced_nv12(gpu, rr, algo):
    """1080i-style input: both planes of NV12 frames are deinterlaced, each with its own
    neighbours, then merged, converted and scaled as usual (pl_render_default_params, 2x). Against
    the same renderer fed the planes the ORACLE deinterlaced, in the form the renderer holds them:
    the chroma plane goes through a scaler and is therefore stored first -- in the plane's own
    format (rg8: rounded, clamped; src/renderer.c:1575, :1603) --, the luma plane is the reference
    grid and continues unrounded (an r32f plane here). Identical frames."""
    w, h = 64, 48
    ys = frames(w, h, "r8", seed=21)
    uvs = frames(w // 2, h // 2, "rg8", seed=22)
    fr = [nv12_frame(gpu, ys[i], uvs[i]) for i in range(3)]
    dst = gpu.tex_create(2 * w, 2 * h, "rgba16")
    target = pl.frame(dst, color=pl.color_space("bt709", "bt1886"))
    base = pl.render_params("default", dither_params=None)
    params = pl.render_params("default", dither_params=None,
                              deinterlace_params=capi.DeinterlaceParams(ALGOS[algo], False))
    for field, first in ((pl.FIELD_TOP, pl.FIELD_TOP), (pl.FIELD_BOTTOM, pl.FIELD_TOP)):
        image = interlaced_frame(gpu, fr[1], field, first, fr[0], fr[2])
        assert rr.render(image, target, params), gpu.messages[-4:]
        assert rr.errors() == 0, gpu.messages[-4:]
        got = dst.download()

        dy = orc.deinterlace(*[orc.tex_decode(ys[i], "r8") for i in (1, 0, 2)], field, first,
                             ALGOS[algo], comp_mask=0x1)
        duv = orc.deinterlace(*[orc.tex_decode(uvs[i], "rg8") for i in (1, 0, 2)], field, first,
                              ALGOS[algo], comp_mask=0x3)
        prog = nv12_frame(gpu, np.ascontiguousarray(dy[..., :1]), orc.tex_encode(duv, "rg8"),
                          luma_fmt="r32f")
        assert rr.render(prog, target, base), gpu.messages[-4:]
        want = dst.download()
        assert np.array_equal(got, want), (field, util.diff_stats(got, want))
        # and it is not the woven frame
        assert rr.render(image, target, base)
        assert np.abs(dst.download().astype(np.int64) - got).max() > 3000
        for t in prog._tex:
            t.destroy()
    for f in fr:
        for t in f._tex:
            t.destroy()
    dst.destroy()


def test_bad_neighbour_frames_are_refused(gpu, rr):
    w, h = 32, 16
    a = gpu.tex_create(w, h, "rgba16", util.chirp_rgba16(w, h))
    b = gpu.tex_create(w, h + 2, "rgba16", util.chirp_rgba16(w, h + 2))
    dst = gpu.tex_create(w, h, "rgba16")
    params = pl.render_params("fast", deinterlace_params=capi.DeinterlaceParams(pl.DEINTERLACE_YADIF, False))
    image = interlaced_frame(gpu, a, pl.FIELD_TOP, pl.FIELD_TOP, pl.frame(b), None)
    assert not rr.render(image, pl.frame(dst), params)
    image = interlaced_frame(gpu, a, pl.FIELD_TOP, pl.FIELD_NONE, None, None)
    assert not rr.render(image, pl.frame(dst), params)
    sh = gpu.begin()
    sh.deinterlace(a, prev=b)
    assert sh.failed()
    sh.abort()
    for t in (a, b, dst):
        t.destroy()


F32_OF = {1: "r32f", 2: "rg32f", 4: "rgba32f"}


@pytest.mark.parametrize("fmt", ["r8", "rg8", "rgba8", "r16", "rg16", "rgba16"])
@pytest.mark.parametrize("size", [(70, 37), (1, 1), (5, 3), (257, 16), (3, 8), (131, 10), (16, 6)])
def test_whole_plane_kernel_equals_the_oracle(gpu, fmt, size, monkeypatch):
    """A whole unorm plane into a texture of its own format or of floats with the same components
    -- what the renderer asks for -- runs as k_deint_rows (a dword of a row pair per lane: bob,
    weave, bwdif) or k_deint_rows_yadif. Bit-exact against the oracle, rows that end inside a dword included, and equal
    to the general kernel (which is what every other test here runs, against the same oracle)."""
    w, h = size
    arr = frames(w, h, fmt, seed=31)
    nc = arr[0].shape[2]
    tex = [gpu.tex_create(w, h, fmt, a) for a in arr]
    dec = [orc.tex_decode(a, fmt) for a in arr]
    for dfmt in (fmt, F32_OF[nc]):
        dst = gpu.tex_create(w, h, dfmt)
        for algo, field, first, have_prev in (("bwdif", pl.FIELD_TOP, pl.FIELD_TOP, True),
                                              ("bwdif", pl.FIELD_BOTTOM, pl.FIELD_TOP, True),
                                              ("bwdif", pl.FIELD_TOP, pl.FIELD_TOP, False),    # intra
                                              ("bob", pl.FIELD_BOTTOM, pl.FIELD_TOP, True),
                                              ("weave", pl.FIELD_TOP, pl.FIELD_TOP, True),
                                              # (k_deint_rows_yadif: windows of dwords to either side;
                                              # rgba16 stays on the general kernel)
                                              ("yadif", pl.FIELD_TOP, pl.FIELD_TOP, True),
                                              ("yadif", pl.FIELD_BOTTOM, pl.FIELD_BOTTOM, True),
                                              ("yadif", pl.FIELD_BOTTOM, pl.FIELD_TOP, False)):
            sh = gpu.begin()
            sh.deinterlace(tex[1], tex[0] if have_prev else None, tex[2], field=field,
                           first_field=first, algo=ALGOS[algo])
            assert sh.finish(dst), gpu.messages[-4:]
            got = dst.download()
            ref = orc.deinterlace(dec[1], dec[0] if have_prev else None, dec[2], field, first,
                                  ALGOS[algo], comp_mask=(1 << nc) - 1)
            want = orc.tex_encode(ref, dfmt)
            assert np.array_equal(got, want), (dfmt, algo, field, util.diff_stats(got, want))
        dst.destroy()
    for t in tex:
        t.destroy()
