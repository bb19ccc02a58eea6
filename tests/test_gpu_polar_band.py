"""EWA downscales steeper than k_polar's LDS tile allows (about 4x from an integer source, 6x from
rgba16hf) up to the reference's own radius cap: k_polar_band (csrc/hip/k_polar_band.hip) walks the
footprint through a ring of source rows, one lane per output pixel, taps in the list's order.

Every case asserts that k_polar_band took the pass (PL_HIP_PASS_TRACE) and that nothing was logged
as an error, and compares with the oracle's gather-order evaluation through util.assert_polar_equal:
bit for bit under the suite's PL_HIP_POLAR_MFMA=0. The shapes are the smallest at which each thing
can go wrong; the oracle costs output pixels x 4 bound^2 taps, milliseconds here."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util
from libplacebo_amd import _capi as capi
from test_gpu_sampling import polar_oracle, polar_pipeline

pytestmark = pytest.mark.gpu

RENDER_ERR_SAMPLING = 1 << 1    # renderer.h
LOG_ERR = 2                     # log.h: PL_LOG_FATAL = 1, PL_LOG_ERR = 2
FMT_RGBA16, FMT_RGBA16F = 6, 9  # plh_device.h: enum plh_fmt, as PL_HIP_PASS_TRACE prints it


@contextlib.contextmanager
def band_only(gpu, capfd, **e):
    """the polar launches inside the block all went to k_polar_band, and no error was logged"""
    n0 = len(gpu.messages)
    with util.kernel_trace(capfd, **e) as kernels:
        yield kernels
    polar = [k for k in kernels if k.startswith("k_polar")]
    assert polar and set(polar) == {"k_polar_band"}, kernels
    errors = [m for lvl, m in gpu.messages[n0:] if lvl <= LOG_ERR]
    assert not errors, errors


def lanczos_for(sw, sh, dw, dh):
    """the widened filter: blur = 1 / the smaller ratio, in setup_src's and pl_shader_sample_polar's
    own arithmetic (sampling.c:146-147, :608-631: float ratios, the quotient rounded to float)"""
    ratio = min(np.float32(dw / float(sw)), np.float32(dh / float(sh)))
    return orc.ewa_lanczos(blur=max(float(np.float32(1.0 / float(ratio))), 1.0))


# 1. 6x isotropic: radius 18.95, bound 19, the f16 tile of 32 x 8 outputs would be 232 x 88 texels
@pytest.mark.parametrize("comps", [3, 4])
def test_six_times_isotropic(gpu, capfd, comps):
    src = util.random_rgba16(96, 72, seed=21)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, 16, 12, comps=comps)
    ref = polar_oracle(src, 16, 12, lanczos_for(96, 72, 16, 12), comps=comps)
    util.assert_polar_equal(got, ref)


# 2. close to the cap: 9.5x, bound 31
def test_at_the_radius_cap(gpu, capfd):
    src = util.random_rgba16(152, 95, seed=22)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, 16, 10)
    ref = polar_oracle(src, 16, 10, lanczos_for(152, 95, 16, 10))
    util.assert_polar_equal(got, ref)


def direct_pipeline(gpu, src, fmt, dw, dh, comps, out_fmt):
    """the polar pass straight out of a texture of format `fmt` (no rgba16hf image in front)"""
    h, w = src.shape[:2]
    t = gpu.tex_create(w, h, fmt, src)
    d = gpu.tex_create(dw, dh, out_fmt)
    lut = pl.ShaderObj()
    s = gpu.begin()
    assert s.sample_polar(t, pl.filter_config("ewa_lanczos"), lut, new_w=dw, new_h=dh,
                          components=comps), gpu.messages[-3:]
    assert s.finish(d), gpu.messages[-3:]
    got = d.download()
    for o in (t, d, lut):
        o.destroy()
    return got


def direct_oracle(src, fmt, dw, dh, comps, out_fmt):
    h, w = src.shape[:2]
    lut, radius, radius_zero = orc.filter_generate_polar(lanczos_for(w, h, dw, dh))
    ref = orc.sample_polar(orc.tex_decode(src, fmt), lut, radius, radius_zero, dw, dh,
                           mask=(1 << comps) - 1, gather_order=not radius < 6.0)
    return orc.tex_encode(ref, out_fmt)


# 3. anisotropic, 6x by 1.5x: the widening follows the steeper axis, the ring is sized per axis.
#    Out of the rgba16 texture itself (fp32 texels): k_polar's tile of 232 x 52 texels is above the
#    LDS only at 16 bytes a texel. Its tile is 32 outputs wide and 8 high, so the transposed pass
#    (88 x 88 texels) still fits it: that one is put on the band kernel by the switch.
@pytest.mark.parametrize("shape,switch", [(((96, 48), (16, 32)), {}),
                                          (((48, 96), (32, 16)), {"PL_HIP_POLAR_BAND": "1"})])
def test_anisotropic(gpu, capfd, shape, switch):
    (sw, sh), (dw, dh) = shape
    src = util.random_rgba16(sw, sh, seed=23)
    with band_only(gpu, capfd, **switch):
        got = direct_pipeline(gpu, src, "rgba16", dw, dh, 3, "rgba16")
    util.assert_polar_equal(got, direct_oracle(src, "rgba16", dw, dh, 3, "rgba16"))


# 4. more than one workgroup each way, ragged edges (70 = 2 x 32 + 6, 21 = 2 x 8 + 5)
def test_several_workgroups_ragged_edges(gpu, capfd):
    src = util.random_rgba16(420, 126, seed=24)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, 70, 21)
    ref = polar_oracle(src, 70, 21, lanczos_for(420, 126, 70, 21))
    util.assert_polar_equal(got, ref)


# 5. source formats, sampled directly: fp32 ring for unorm and fp32 texels, f16 ring for rgba16hf
#    (at 6x the 8-byte tile is past its limit too)
@pytest.mark.parametrize("fmt,comps", [("rgba8", 4), ("r8", 1), ("rgba16hf", 4), ("rgba32f", 4)])
def test_source_formats(gpu, capfd, fmt, comps):
    sw, sh, dw, dh = 96, 72, 16, 12
    dt, nc = pl._FMT_DTYPES[fmt]
    rng = np.random.default_rng(25)
    if np.issubdtype(dt, np.integer):
        src = rng.integers(0, np.iinfo(dt).max + 1, (sh, sw, nc)).astype(dt)
    else:
        src = rng.random((sh, sw, nc)).astype(dt)
    out_fmt = "rgba32f" if fmt == "rgba32f" else "rgba16"
    with band_only(gpu, capfd):
        got = direct_pipeline(gpu, src, fmt, dw, dh, comps, out_fmt)
    util.assert_polar_equal(got, direct_oracle(src, fmt, dw, dh, comps, out_fmt))


# 6. rects and address modes
@pytest.mark.parametrize("rect", [(96, 0, 0, 72), (0, 72, 96, 0), (10.5, 7.25, 90.0, 60.5)])
def test_rects(gpu, capfd, rect):
    src = util.random_rgba16(96, 72, seed=26)
    rw, rh = util.rect_size(rect)
    dw, dh = round(rw / 6), round(rh / 6)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, dw, dh, rect=rect)
    ref = polar_oracle(src, dw, dh, lanczos_for(rw, rh, dw, dh), rect=rect)
    util.assert_polar_equal(got, ref)


@pytest.mark.parametrize("mode", [pl.ADDRESS_CLAMP, pl.ADDRESS_REPEAT, pl.ADDRESS_MIRROR])
def test_address_modes_source_smaller_than_a_footprint(gpu, capfd, mode):
    # 30 x 24 texels under a footprint of 38 x 38: every pixel's taps wrap on both sides
    src = util.random_rgba16(30, 24, seed=27)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, 5, 4, address_mode=mode)
    ref = polar_oracle(src, 5, 4, lanczos_for(30, 24, 5, 4), address_mode=mode)
    util.assert_polar_equal(got, ref)


# 7. anti-ringing
def test_antiring(gpu, capfd):
    src = util.random_rgba16(96, 72, seed=28)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, 16, 12, antiring=0.8)
    ref = polar_oracle(src, 16, 12, lanczos_for(96, 72, 16, 12), antiring=0.8)
    util.assert_polar_equal(got, ref)


# 8. post-ops behind the sampler
@pytest.mark.parametrize("depth,fmt", [(8, "rgba8"), (10, "rgba16")])
def test_blue_noise_dither_behind_the_sampler(gpu, capfd, depth, fmt):
    src = util.chirp_rgba16(96, 72)
    mat = util.blue_noise(pl)
    with band_only(gpu, capfd):
        got = polar_pipeline(gpu, src, 16, 12, dither_depth=depth, out_fmt=fmt)
    ref = polar_oracle(src, 16, 12, lanczos_for(96, 72, 16, 12), dither_depth=depth, out_fmt=fmt,
                       matrix=mat)
    util.assert_polar_equal(got, ref, step={8: 1, 10: 65}[depth])


# 9. A/B where both kernels can run: the same bits
def test_band_equals_k_polar_at_a_quarter(gpu, capfd):
    src = util.random_rgba16(128, 96, seed=5)
    with band_only(gpu, capfd, PL_HIP_POLAR_BAND="1"):
        band = polar_pipeline(gpu, src, 32, 24)
    with util.kernel_trace(capfd, PL_HIP_POLAR_BAND="0") as kernels:
        whole = polar_pipeline(gpu, src, 32, 24)
    assert [k for k in kernels if k.startswith("k_polar")] == ["k_polar"], kernels
    assert np.array_equal(band, whole), util.diff_stats(band, whole)


@contextlib.contextmanager
def pass_trace(capfd):
    """as util.kernel_trace, with the source format of the pass each kernel took: (name, src.fmt)"""
    launches = []
    capfd.readouterr()
    with util.env(PL_HIP_PASS_TRACE="1"):
        yield launches
    fmt = None
    for ln in capfd.readouterr().err.splitlines():
        if ln.startswith("[plh] pass "):
            fmt = int(ln.split("src.fmt=")[1].split()[0])
        elif ln.startswith("[plh] kernel "):
            launches.append((ln.split()[-1], fmt))


# 4.5x out of an integer texture (2160p -> 480p): fp32 texels, k_polar's tile would be 176 x 68 of them
def test_integer_source_at_four_and_a_half(gpu, capfd):
    src = util.random_rgba16(288, 162, seed=29)
    with band_only(gpu, capfd):
        got = direct_pipeline(gpu, src, "rgba16", 64, 36, 4, "rgba16")
    util.assert_polar_equal(got, direct_oracle(src, "rgba16", 64, 36, 4, "rgba16"))


# 10. the renderer out of an rgba16 plane. The main scaler never reads the integer plane itself: the
#     plane's fetch is folded into the polar pass (an f16 tile) or lands in an rgba16hf image, so a
#     renderer's limit is the 8-byte one, 5.9x.
#     * 6x with the library's defaults: on the parent the shader failed, PL_RENDER_ERR_SAMPLING stuck,
#       and every later frame of that renderer -- its upscales too -- was scaled by a bare bilinear
#       fetch. Now the fold is declined because the pass takes the band walk, the pending image
#       becomes the intermediate it is for every other scaler, and the band kernel reads that.
#     * 4.5x (k_polar still holds its f16 tile, 94 KiB, and renders it by default): the same frame
#       structure with the band kernel switched in.
@pytest.mark.parametrize("size,switch", [((384, 216), {}), ((288, 162), {"PL_HIP_POLAR_BAND": "1"})])
def test_renderer_integer_source_and_no_sticky_error(gpu, capfd, size, switch):
    (sw, sh), (dw, dh), comps = size, (64, 36), 3
    img = util.random_rgba16(sw, sh, seed=30)
    img[..., 3] = 65535
    src = gpu.tex_create(sw, sh, "rgba16", img)
    dst = gpu.tex_create(dw, dh, "rgba16")
    rr = pl.Renderer(gpu)
    params = pl.render_params("fast", downscaler=pl.filter_config("ewa_lanczos", 2),
                              disable_linear_scaling=True)
    n0 = len(gpu.messages)
    with util.env(**switch), pass_trace(capfd) as launches:
        assert rr.render(pl.frame(src, components=comps), pl.frame(dst), params), gpu.messages[-4:]
    assert rr.errors() == 0, gpu.messages[-4:]
    assert not [m for lvl, m in gpu.messages[n0:] if lvl <= LOG_ERR]
    assert [l for l in launches if l[0].startswith("k_polar")] == [("k_polar_band", FMT_RGBA16F)], launches
    got = dst.download()
    a = orc.tex_decode(img, "rgba16")
    a[..., 3] = 1.0
    a = orc.op_quant_f16(a)     # the intermediate image
    w, r, rz = orc.filter_generate_polar(lanczos_for(sw, sh, dw, dh))
    ref = orc.sample_polar(a, w, r, rz, dw, dh, mask=(1 << comps) - 1, gather_order=True)
    util.assert_polar_equal(got, orc.tex_encode(ref, "rgba16"))

    # the same renderer still scales with the filter it is asked for
    up = gpu.tex_create(2 * dw, 2 * dh, "rgba16")
    small = gpu.tex_create(dw, dh, "rgba16", got)
    with util.kernel_trace(capfd) as kernels:
        assert rr.render(pl.frame(small, components=3), pl.frame(up),
                         pl.render_params("fast", upscaler=pl.filter_config("ewa_lanczos")))
    assert rr.errors() == 0
    assert any(k.startswith("k_polar") for k in kernels), kernels
    for o in (src, dst, up, small):
        o.destroy()
    rr.destroy()


# 11. the renderer, rgba16hf intermediate: HDR10 -> SDR at 6x with the default parameters. The source
#     is linearised into an rgba16hf image (nothing is fused into the band walk), scaled in linear
#     light, measured, mapped.
def test_renderer_f16_intermediate_hdr(gpu, capfd):
    import colormap_f64 as c64
    import colormap_ref as cr
    from test_gpu_color import luma_coeffs, nominal
    from test_gpu_fullsize import colormap_tolerance, hdr_frame16, inferred, resolve_with_peak
    sw, sh, dw, dh = 384, 216, 64, 36
    img = hdr_frame16(sw, sh)
    src = gpu.tex_create(sw, sh, "rgba16", img)
    dst = gpu.tex_create(dw, dh, "rgba16")
    rr = pl.Renderer(gpu)
    hdr = pl.color_space("bt2020", "pq")
    sdr = pl.color_space("bt709", "bt1886")
    params = pl.render_params("default", dither_params=None,
                              downscaler=pl.filter_config("ewa_lanczos", 2))
    n0 = len(gpu.messages)
    with pass_trace(capfd) as launches:
        assert rr.render(pl.frame(src, components=3, color=hdr), pl.frame(dst, color=sdr), params), \
            gpu.messages[-4:]
    assert rr.errors() == 0, gpu.messages[-4:]
    assert not [m for lvl, m in gpu.messages[n0:] if lvl <= LOG_ERR]
    assert [l for l in launches if l[0].startswith("k_polar")] == [("k_polar_band", FMT_RGBA16F)], launches
    got = dst.download()
    meta = capi.HdrMetadata()
    assert pl.lib().pl_renderer_get_hdr_metadata(rr.rr, C.byref(meta))

    # The chain of test_gpu_fullsize.py::test_cfg5_8k_to_4k_deband_ewa_tone_map without its debanding,
    # from the linearised rgba16hf image on. That image is taken from the GPU (the same pass, recorded
    # by hand): the kernels' PQ EOTF and the oracle's libm one round about 1 % of its texels to
    # neighbouring f16 codes (test_cfg5_stage_by_stage holds that stage to float64), and through a
    # 38 x 38 footprint one such texel moves 130 output samples -- with the oracle's own image in
    # front, 117 of 5330 trusted samples were more than 1.5 codes away, up to 39: figures about that
    # stage, which a CPU rehearsal with 1.5 % of the texels moved by one f16 ulp reproduces (108, 35).
    hdr_i, _ = inferred(hdr, sdr)
    mn, mx = nominal(hdr_i)
    fbo = gpu.tex_create(sw, sh, "rgba16hf")
    s = gpu.begin()
    assert s.sample("direct", src, components=3)
    s.linearize(hdr_i)
    assert s.finish(fbo), gpu.messages[-3:]
    a = fbo.download().astype(np.float32)
    fbo.destroy()
    a[..., 3] = 1.0
    want = orc.tex_decode(img, "rgba16")
    want[..., 3] = 1.0
    orc.linearize(want, pl.TRC["pq"], mn, mx, luma_coeffs(hdr_i.primaries))
    u16 = lambda x: x[..., :3].astype(np.float16).view(np.uint16).astype(np.int32)
    ulps = np.abs(u16(a) - u16(want))
    assert (ulps <= 1).mean() >= 0.9999 and (ulps > 0).mean() <= 0.03, \
        (int(ulps.max()), float((ulps > 0).mean()))
    w, r, rz = orc.filter_generate_polar(lanczos_for(sw, sh, dw, dh))
    b = orc.sample_polar(a, w, r, rz, dw, dh, mask=0x7, gather_order=True)
    orc.op_quant_f16(b)
    res = resolve_with_peak(meta)
    sel = np.arange(dw * dh)
    truth, _ = c64.hdr10_to_sdr(b.reshape(-1, 1, 4)[sel], res, 0.0, prelinearized=True)
    ref16 = orc.tex_encode(cr.apply(b, res, prelinearized=True), "rgba16")
    # the colour-map statement of tests/util.py, quantiles and per sample, maximum included
    colormap_tolerance(got, ref16, truth.reshape(-1, 4), sel)
    assert np.all(got[..., 3] == 65535)
    for o in (src, dst):
        o.destroy()
    rr.destroy()


# 12. the cap itself is the reference's: ceil(radius) = 35 at 10.5x
def test_beyond_the_cap_is_refused_as_the_reference_refuses_it(gpu):
    sw, sh, dw, dh = 168, 105, 16, 10
    src = gpu.tex_create(sw, sh, "rgba16", util.random_rgba16(sw, sh, seed=32))
    dst = gpu.tex_create(dw, dh, "rgba16")
    rr = pl.Renderer(gpu)
    params = pl.render_params("fast", downscaler=pl.filter_config("ewa_lanczos", 2),
                              disable_linear_scaling=True)
    n0 = len(gpu.messages)
    # (what becomes of this frame is not the subject: the error and its wording are)
    rr.render(pl.frame(src, components=3), pl.frame(dst), params)
    assert rr.errors() & RENDER_ERR_SAMPLING
    assert any("exceeds implementation capacity" in m for _, m in gpu.messages[n0:]), gpu.messages[n0:]
    for o in (src, dst):
        o.destroy()
    rr.destroy()
