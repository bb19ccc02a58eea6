"""ICC colour management on the GPU: the two ops of pl_icc_decode / pl_icc_encode against numpy
models of them, and the renderer's use of pl_frame.icc / pl_frame.profile (reference
src/renderer.c:1948-1953, :2249-2272, :3235-3281, :3788).

Tolerance of every comparison with a model: CONDITIONING + one 16-bit code (the project's parity
unit), where CONDITIONING is the largest distance between the model evaluated in float32 with the
kernel's operation order and in float64, over the inputs of the comparison. Measured (printed by
the tests): decode 2.0e-7, encode 1.7e-7, round trip 2.7e-7 (sRGB profile, 17^3), all far below one code
(1.5e-5).

Profiles are made by the test with lcms2 through ctypes (tests/icc_ref.py); tables come from
the library's hook, which tests/test_icc.py holds to lcms2 entry for entry."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import icc_ref
import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

if icc_ref.CMS is None:
    pytest.skip("liblcms2.so.2 cannot be loaded", allow_module_level=True)

CODE = 1.0 / 65535.0
W, H = 48, 32
LUT_CONVERSION = 3      # enum pl_lut_type
PL_LOG_WARN = 3


# ---- shared, computed once -------------------------------------------------------------------

@pytest.fixture(scope="module")
def srgb(built):
    """the sRGB profile at 17^3: object, both tables, the curve's constants"""
    data = icc_ref.srgb_profile()
    icc = pl.Icc(data, size=(17,) * 3)
    a, b, scale = icc_ref.approx_constants(icc.gamma, icc.csp.hdr.min_luma, icc.csp.hdr.max_luma)
    d = dict(data=data, icc=icc, dec=icc.lut(False), enc=icc.lut(True),
             consts=(a, b, icc.gamma, scale))
    yield d
    icc.close()


def probe_points(size, consts):
    """36 x 24 rgb points: LUT vertices, one interior point in each of the six tetrahedra, ties
    between the fractional parts, 0, 1, values outside [0, 1]; the second half are the same
    positions taken through the approximation curve (what the encode op maps back onto them)"""
    rng = np.random.default_rng(7)
    n = size - 1
    pts = []
    pts += [rng.integers(0, size, 3) / n for _ in range(96)]                    # vertices
    base = np.array([3, 7, 11])
    for fr in ((.7, .5, .2), (.7, .2, .5), (.5, .2, .7), (.2, .5, .7), (.2, .7, .5), (.5, .7, .2)):
        pts += [(base + fr) / n, (base[::-1] + fr) / n, (np.array([0, n - 1, 5]) + fr) / n]
    for fr in ((.5, .5, .2), (.5, .5, .8), (.2, .6, .6), (.9, .6, .6), (.4, .1, .4), (.4, .9, .4),
               (.3, .3, .3), (0., 0., .5), (.5, 0., 0.), (0., .5, 0.)):
        pts += [(base + fr) / n, (base[[1, 2, 0]] + fr) / n]
    pts += [(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1), (-0.5, 0.5, 0.5), (0.5, -1e-3, 0.5),
            (0.5, 0.5, 1.0001), (2.0, 0.25, -3.0), (-1, -1, -1), (1.5, 1.5, 1.5)]
    pts = np.array(pts, np.float64)
    fill = rng.uniform(-0.1, 1.1, (432 - len(pts), 3))
    direct = np.concatenate([pts, fill]).astype(np.float32)
    a, b, gamma, scale = (float(v) for v in consts)
    through = (scale * (a * np.clip(direct.astype(np.float64), 0, None) + b) ** gamma).astype(np.float32)
    rgb = np.concatenate([direct, through]).reshape(24, 36, 3)
    img = np.empty((24, 36, 4), np.float32)
    img[..., :3] = rgb
    img[..., 3] = np.linspace(0.0, 1.0, 24 * 36, dtype=np.float32).reshape(24, 36)
    return img


def conditioning(model, *args):
    """largest distance between the model's float32 and float64 runs; the float64 run"""
    ref = model(*args, ftype=np.float64)
    r32 = model(*args, ftype=np.float32)
    return float(np.abs(r32.astype(np.float64) - ref).max()), ref


def run_ops(gpu, img, stages):
    """img (rgba32f) -> the ICC stages -> rgba32f; returns the frame and the shader's listing"""
    h, w = img.shape[:2]
    src = gpu.tex_create(w, h, "rgba32f", img)
    dst = gpu.tex_create(w, h, "rgba32f")
    states = [pl.ShaderObj() for _ in stages]
    sh = gpu.begin()
    assert sh.sample("nearest", src)
    out_csp = None
    for (kind, icc), st in zip(stages, states):
        if kind == "decode":
            out_csp = sh.icc_decode(icc, st)
        else:
            sh.icc_encode(icc, st)
    assert not sh.failed(), gpu.messages[-3:]
    listing = sh.listing()
    assert sh.finish(dst), gpu.messages[-3:]
    out = dst.download()
    for st in states:
        st.destroy()
    src.destroy(); dst.destroy()
    return out, listing, out_csp


# ---- the ops -----------------------------------------------------------------------------------

def test_decode_op(gpu, srgb):
    img = probe_points(17, srgb["consts"])
    cond, ref = conditioning(icc_ref.decode_model, srgb["dec"], img[..., :3], *srgb["consts"])
    got, listing, out_csp = run_ops(gpu, img, [("decode", srgb["icc"])])
    d = np.abs(got[..., :3].astype(np.float64) - ref)
    print("icc_decode: conditioning %.3g, GPU max |diff| %.3g (%.2f codes)" % (cond, d.max(), d.max() / CODE))
    assert d.max() <= cond + CODE
    assert np.array_equal(got[..., 3], img[..., 3])
    assert "icc_decode(17x17x17, tetrahedral)" in listing
    # the colour space the reference leaves the shader in: containing primaries, linear, the profile's hdr
    icc = srgb["icc"]
    assert (out_csp.primaries, out_csp.transfer) == (icc.containing_primaries, 3)   # PL_COLOR_TRC_LINEAR
    assert bytes(out_csp.hdr) == bytes(icc.csp.hdr)


def test_encode_op(gpu, srgb):
    img = probe_points(17, srgb["consts"])
    cond, ref = conditioning(icc_ref.encode_model, srgb["enc"], img[..., :3], *srgb["consts"])
    got, listing, _ = run_ops(gpu, img, [("encode", srgb["icc"])])
    d = np.abs(got[..., :3].astype(np.float64) - ref)
    print("icc_encode: conditioning %.3g, GPU max |diff| %.3g (%.2f codes)" % (cond, d.max(), d.max() / CODE))
    assert d.max() <= cond + CODE
    assert np.array_equal(got[..., 3], img[..., 3])
    assert "icc_encode(17x17x17, tetrahedral)" in listing


def round_trip_model(dec, enc, rgb, a, b, gamma, scale, ftype=np.float64):
    lin = icc_ref.decode_model(dec, rgb, a, b, gamma, scale, ftype)
    return icc_ref.encode_model(enc, lin, a, b, gamma, scale, ftype)


def test_round_trip(gpu, srgb):
    img = probe_points(17, srgb["consts"])
    cond, ref = conditioning(round_trip_model, srgb["dec"], srgb["enc"], img[..., :3], *srgb["consts"])
    got, _, _ = run_ops(gpu, img, [("decode", srgb["icc"]), ("encode", srgb["icc"])])
    d = np.abs(got[..., :3].astype(np.float64) - ref)
    print("round trip: conditioning %.3g, GPU max |diff| %.3g (%.2f codes)" % (cond, d.max(), d.max() / CODE))
    assert d.max() <= cond + CODE


# ---- the renderer --------------------------------------------------------------------------------

def picture(w, h, seed=3):
    img = util.chirp_rgba16(w, h)
    rng = np.random.default_rng(seed)
    img[:4, :, :3] = rng.integers(0, 65536, (4, w, 3))      # + a band of arbitrary colours
    img[-1, :, :3] = 0
    img[-2, :, :3] = 65535
    return img


def render(gpu, img, out_fmt="rgba16", image_kw=None, target_kw=None, params=None, out_size=(W, H),
           rr=None):
    h, w = img.shape[:2]
    src = gpu.tex_create(w, h, "rgba16", img)
    dst = gpu.tex_create(out_size[0], out_size[1], out_fmt)
    own = rr is None
    rr = rr or pl.Renderer(gpu)
    image = pl.frame(src, components=3, **(image_kw or {}))
    target = pl.frame(dst, **(target_kw or {}))
    params = params if params is not None else pl.render_params("fast", dither_params=None)
    ok = rr.render(image, target, params)
    assert ok and rr.errors() == 0, gpu.messages[-5:]
    out = dst.download()
    if own:
        rr.destroy()
    src.destroy(); dst.destroy()
    return out


def icc_color(icc, transfer):
    """the pl_color_space the renderer forces onto a frame that carries `icc`"""
    csp = capi.ColorSpace(primaries=icc.containing_primaries,
                          transfer=icc.csp.transfer or transfer, hdr=icc.csp.hdr)
    return csp


def linear_space(icc):
    return capi.ColorSpace(primaries=icc.containing_primaries, transfer=3, hdr=icc.csp.hdr)


def encoded_by_model(gpu, srgb, img, **kw):
    """the construction of (b): the frame rendered without a profile into an rgba32f target in
    {containing primaries, linear, the profile's hdr}, through the float64 encode model, quantised;
    returns it with the conditioning margin in codes"""
    lin = render(gpu, img, "rgba32f", target_kw=dict(color=linear_space(srgb["icc"])), **kw)
    cond, ref = conditioning(icc_ref.encode_model, srgb["enc"], lin[..., :3], *srgb["consts"])
    return np.rint(np.clip(ref, 0, 1) * 65535.0), cond / CODE


def test_image_icc_and_profile_render_the_same(gpu, srgb):
    img = picture(W, H)
    tgt = dict(color=pl.color_space("bt2020", "bt1886"))
    icc = pl.Icc(srgb["data"])      # (default parameters: what the renderer opens `profile` with)
    with_icc = render(gpu, img, image_kw=dict(icc=icc), target_kw=tgt)
    with_profile = render(gpu, img, image_kw=dict(profile=pl.icc_profile(srgb["data"])), target_kw=tgt)
    icc.close()
    assert np.array_equal(with_icc, with_profile)
    # ... and the profile acts: a frame that only claims the profile's colour space is another frame
    plain = render(gpu, img, image_kw=dict(color=icc_color(srgb["icc"], 2)), target_kw=tgt)
    assert not np.array_equal(with_icc, plain)
    assert with_icc[..., :3].std() > 1000


def test_target_profile(gpu, srgb):
    img = picture(W, H)
    got = render(gpu, img, target_kw=dict(icc=srgb["icc"]))
    want, margin = encoded_by_model(gpu, srgb, img)
    d = np.abs(got[..., :3].astype(np.float64) - want)
    print("target profile: max |diff| %.2f codes (margin %.3f + 1)" % (d.max(), margin))
    assert d.max() <= 1 + margin
    assert np.all(got[..., 3] == 65535)


def test_image_and_target_carry_the_same_profile(gpu, srgb):
    img = picture(W, H)
    got = render(gpu, img, image_kw=dict(icc=srgb["icc"]), target_kw=dict(icc=srgb["icc"]))
    rgb = img[..., :3].astype(np.float32) / np.float32(65535)
    cond, ref = conditioning(round_trip_model, srgb["dec"], srgb["enc"], rgb, *srgb["consts"])
    d = np.abs(got[..., :3].astype(np.float64) - np.rint(np.clip(ref, 0, 1) * 65535.0))
    print("same profile on both sides: max |diff| %.2f codes (margin %.3f + 1)" % (d.max(), cond / CODE))
    assert d.max() <= 1 + cond / CODE


def test_conversion_lut_overrides_the_image_profile(gpu, srgb):
    img = picture(W, H)
    grid = np.stack(np.meshgrid(*[np.linspace(0, 1, 3)] * 3, indexing="ij")[::-1], -1).reshape(-1, 3)
    lut = pl.custom_lut((grid ** 1.1).astype(np.float32), (3, 3, 3))
    params = pl.render_params("fast", dither_params=None, lut=lut, lut_type=LUT_CONVERSION)
    color = icc_color(srgb["icc"], 2)
    tgt = dict(color=pl.color_space("bt709", "bt1886"))
    plain = render(gpu, img, image_kw=dict(color=color), target_kw=tgt, params=params)
    with_icc = render(gpu, img, image_kw=dict(color=color, icc=srgb["icc"]), target_kw=tgt, params=params)
    assert np.array_equal(plain, with_icc)


def upscale_check(gpu, srgb):
    img = picture(24, 16)
    params = pl.render_params("fast", dither_params=None, upscaler=pl.filter_config("ewa_lanczos"))
    got = render(gpu, img, target_kw=dict(icc=srgb["icc"]), params=params)
    want, margin = encoded_by_model(gpu, srgb, img, params=params)
    d = np.abs(got[..., :3].astype(np.float64) - want)
    print("ewa_lanczos upscale + target profile (PL_HIP_POLAR_MFMA=%s): max |diff| %.2f codes "
          "(margin %.3f + 1)" % (os.environ.get("PL_HIP_POLAR_MFMA"), d.max(), margin))
    assert d.max() <= 1 + margin
    return got


def test_upscale_with_target_profile(gpu, srgb):
    """the scaler's pass is split off the ICC pass: the polar kernels do not carry the op"""
    got = upscale_check(gpu, srgb)
    assert got.shape == (H, W, 4) and got[..., :3].std() > 1000


def test_upscale_with_target_profile_on_the_matrix_pipe():
    """the same with the library's default polar kernel (k_polar_mx), in a process of its own"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PL_HIP_POLAR_MFMA="1",
               PYTHONPATH=os.pathsep.join(filter(None, [root, os.environ.get("PYTHONPATH")])))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "upscale"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "upscale ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_profile_that_does_not_open(srgb):
    img = picture(W, H)
    bad = pl.icc_profile(np.random.default_rng(9).integers(0, 256, 512, dtype=np.uint8).tobytes())
    tgt = dict(color=pl.color_space("bt709", "bt1886"))
    with pl.HipGpu(0, log_level=PL_LOG_WARN) as g:
        rr = pl.Renderer(g)
        first = render(g, img, image_kw=dict(profile=bad), target_kw=tgt, rr=rr)
        second = render(g, img, image_kw=dict(profile=bad), target_kw=tgt, rr=rr)
        msgs = [m for _, m in g.messages]
        plain = render(g, img, target_kw=tgt, rr=rr)
        rr.destroy()
    assert sum("Failed opening ICC profile... ignoring" in m for m in msgs) == 1, msgs
    assert sum(m == "Failed opening ICC profile" for m in msgs) == 1, msgs      # not retried
    assert not any("not interpreted by this build" in m for m in msgs)
    assert np.array_equal(first, plain) and np.array_equal(second, plain)


def test_mix_with_a_target_profile(gpu):
    """two frames blended onto a target that carries `profile`; the cached frames are rendered
    again when the profile changes although the target's pl_color_space stays what it was"""
    prof_a = pl.icc_profile(icc_ref.gamma_profile(icc_ref.BT709, 2.2))
    prof_b = pl.icc_profile(icc_ref.gamma_profile(icc_ref.BT709, 2.205))
    imgs = [picture(W, H, seed=s) for s in (1, 2)]
    texs = [gpu.tex_create(W, H, "rgba16", i) for i in imgs]
    frames = [pl.frame(t, components=3, color=pl.color_space("bt709", "bt1886")) for t in texs]
    mixer = capi.FilterConfig()
    C.memmove(C.byref(mixer), C.byref(pl.filter_config("linear", pl.FILTER_FRAME_MIXING)), C.sizeof(mixer))
    params = pl.render_params("fast", dither_params=None, frame_mixer=mixer)
    dst = gpu.tex_create(W, H, "rgba16")

    def mix(rr, prof):
        target = pl.frame(dst, color=pl.color_space("bt709", "gamma22"), profile=prof)
        assert rr.render_mix(frames, [11, 12], [-0.7, 0.3], 1.0, target, params), gpu.messages[-4:]
        assert rr.errors() == 0
        return dst.download()

    rr = pl.Renderer(gpu)
    a1 = mix(rr, prof_a)
    a2 = mix(rr, prof_a)            # from the cache
    b_after_a = mix(rr, prof_b)
    rr.destroy()
    rr = pl.Renderer(gpu)
    b_fresh = mix(rr, prof_b)
    rr.destroy()
    assert np.array_equal(a1, a2)
    assert np.array_equal(b_after_a, b_fresh)
    assert not np.array_equal(a1, b_fresh)
    # a real blend of the two frames, encoded for the display: neither input
    for i in imgs:
        assert np.abs(a1[..., :3].astype(int) - i[..., :3].astype(int)).max() > 500
    for t in texs + [dst]:
        t.destroy()


if __name__ == "__main__":
    # the child of test_upscale_with_target_profile_on_the_matrix_pipe
    assert sys.argv[1:] == ["upscale"]
    data = icc_ref.srgb_profile()
    icc = pl.Icc(data, size=(17,) * 3)
    consts = icc_ref.approx_constants(icc.gamma, icc.csp.hdr.min_luma, icc.csp.hdr.max_luma)
    d = dict(data=data, icc=icc, enc=icc.lut(True), consts=(consts[0], consts[1], icc.gamma, consts[2]))
    with pl.HipGpu(0) as g:
        upscale_check(g, d)
    icc.close()
    print("upscale ok")
