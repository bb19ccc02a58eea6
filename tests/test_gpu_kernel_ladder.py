"""Which kernel takes which pass: one table of tiny launches, each held to the COMPLETE list of kernel
names the trace gives (util.kernel_trace: PL_HIP_PASS_TRACE), in order. At least one row for every
candidate of every launcher's table (the 1:1 passes, the measuring pass, the separable
scalers, debanding, the deinterlacer, the polar scalers) and one for each fall-through between them
that a switch, a format, a tap count or a size decides.

The expected lists were recorded on the commit before the launchers became tables and must not
change with them. The deinterlacer's rows are the exception: its launches put no name in the trace
before that commit, so their names were read off its variant test by hand (deint_rows_variant then,
deint_rows_plan now: k_deinterlace.hip) -- an unorm plane into a texture of its own format or of
floats goes row-wise (k_deint_rows, with yadif k_deint_rows_yadif for one or two components, of
either width, and for rgba8), everything else to k_deinterlace.

What the frames hold is other tests' matter (test_gpu_kernel_variants.py, test_gpu_peak_shapes.py,
test_gpu_ortho_deband.py, test_gpu_deinterlace.py): here only the decisions."""
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

# Odd: the last column is a single pixel, the last tiles are partial. And a size whose whole-texture
# rect normalises to exactly 1.0 (float32: (1 / 95) * 95 == 1 and (1 / 59) * 59 == 1), which is what the
# kernels written for a pass that "covers its source" ask (plh_pass_covers_source). 97 x 61 does not
# -- (1 / 97) * 97 < 1 -- and such a pass takes the general kernels: the rows named "97x61".
W, H = 95, 59
TEN_BIT = dict(sample_depth=16, color_depth=10, bit_shift=6)
SDR, HDR = ("bt709", "bt1886"), ("bt2020", "pq")


def hdr16(w=W, h=H):
    from test_gpu_fullsize import hdr_frame16
    return hdr_frame16(w, h)


def f16(img, gain=1.0):
    return (img.astype(np.float32) / 65535.0 * gain).astype(np.float16)


def plane(fmt, w=W, h=H):
    """the chirp's first components as a texel array of `fmt`"""
    dt, n = pl._FMT_DTYPES[fmt]
    img = util.chirp_rgba16(w, h)[..., :n]
    if dt is np.uint8:
        return (img >> 8).astype(np.uint8)
    if dt is np.uint16:
        return img.copy()
    return (img.astype(np.float32) / 65535.0).astype(dt)


def csp_of(trc):
    from test_gpu_fullsize import inferred
    prim = "bt2020" if trc == "pq" else "bt709"
    return inferred(pl.color_space(prim, trc, max_luma=1000.0), pl.color_space(*SDR))[0]


# ---- the renderer's passes ---------------------------------------------------------------------

def render(gpu, preset="fast", scale=(1, 1), hdr=False, ten_bit=True, src_fmt="rgba16", size=(W, H), **kw):
    W, H = size
    img = hdr16(W, H) if hdr else util.chirp_rgba16(W, H)
    if src_fmt == "rgba16hf":
        img = f16(img)
    if ten_bit and preset == "fast":
        kw.update(dither_params=capi.DitherParams(method=pl.DITHER_BLUE_NOISE, lut_size=6, transfer=0),
                  disable_dither_gamma_correction=True)
    if hdr:
        kw.setdefault("peak_detect_params", pl.peak_detect_params(percentile=99.995))
    src = gpu.tex_create(W, H, src_fmt, img)
    dst = gpu.tex_create(int(W * scale[0]), int(H * scale[1]), "rgba16")
    rr = pl.Renderer(gpu)
    util.srand(1)
    image = pl.frame(src, components=3, color=pl.color_space(*HDR, max_luma=1000.0) if hdr else None)
    target = pl.frame(dst, repr_=pl.color_repr("rgb", "full", **TEN_BIT) if ten_bit else None,
                      color=pl.color_space(*SDR) if hdr else None)
    assert rr.render(image, target, pl.render_params(preset, **kw)), gpu.messages[-4:]
    assert rr.errors() == 0
    rr.destroy(); src.destroy(); dst.destroy()


def render_planar(gpu):
    """NV12: the pass that assembles the planes (k_pass_merge) behind the chroma plane's scaler"""
    from test_gpu_renderer import planar_frame
    w, h = 66, 46
    f, texs, _ = planar_frame(gpu, w, h, seed=5)
    f.repr = pl.color_repr("bt709", "limited", sample_depth=8, color_depth=8)
    f.color = pl.color_space(*SDR)
    pl.lib().pl_frame_set_chroma_location.argtypes = [C.POINTER(capi.Frame), C.c_int]
    pl.lib().pl_frame_set_chroma_location(C.byref(f), 1)
    dst = gpu.tex_create(w, h, "rgba16")
    rr = pl.Renderer(gpu)
    util.srand(1)
    assert rr.render(f, pl.frame(dst, repr_=pl.color_repr("rgb", "full", **TEN_BIT), color=pl.color_space(*SDR)),
                     pl.render_params("fast", deband_params=None)), gpu.messages[-4:]
    assert rr.errors() == 0
    rr.destroy(); dst.destroy()
    for t in texs:
        t.destroy()


def render_mix(gpu):
    """two cached frames blended by pl_render_image_mix: k_pass_mix"""
    cfg = capi.FilterConfig()
    C.memmove(C.byref(cfg), C.byref(pl.filter_config("linear", pl.FILTER_FRAME_MIXING)), C.sizeof(cfg))
    base = util.chirp_rgba16(W, H)
    texs = [gpu.tex_create(W, H, "rgba16", np.roll(base, 5 * i, axis=1)) for i in range(2)]
    frames = [pl.frame(t, components=3, color=pl.color_space(*SDR)) for t in texs]
    dst = gpu.tex_create(W, H, "rgba16")
    rr = pl.Renderer(gpu)
    assert rr.render_mix(frames, [1000, 1001], [-0.7, 0.3], 1.0, pl.frame(dst, color=pl.color_space(*SDR)),
                         pl.render_params("fast", frame_mixer=cfg)), gpu.messages[-4:]
    assert rr.errors() == 0
    rr.destroy(); dst.destroy()
    for t in texs:
        t.destroy()


# ---- single passes through the shader interface ------------------------------------------------

def features_pass(gpu):
    """pl_shader_extract_features of a linear-light image into an r16hf plane: the one op"""
    src = gpu.tex_create(W, H, "rgba16", util.chirp_rgba16(W, H))
    dst = gpu.tex_create(W, H, "r16hf")
    sh = gpu.begin()
    assert sh.sample("direct", src, components=3)
    sh.extract_features(csp_of("linear"))
    assert sh.finish(dst), gpu.messages[-3:]
    src.destroy(); dst.destroy()


def peak(gpu, trc="pq", src_fmt="rgba16", w=W, h=H, target="rgba16hf", features=False):
    """the measuring pass: plane texel for texel + PEAK_DETECT [+ [LINEARIZE] FEATURES], into the
    f16 intermediate, into the r16hf feature plane or (target None) nowhere"""
    img = hdr16(w, h)
    csp = csp_of(trc)
    src = gpu.tex_create(w, h, src_fmt, f16(img, 4.0) if src_fmt == "rgba16hf" else img)
    dst = gpu.tex_create(w, h, target) if target else None
    state = pl.ShaderObj()
    sh = gpu.begin()
    assert sh.sample("direct", src, components=3)
    assert sh.detect_peak(csp, state, percentile=99.995)
    if features:
        sh.extract_features(csp)
    assert (sh.finish(dst) if dst else sh.compute(w, h)), gpu.messages[-3:]
    state.destroy(); src.destroy()
    if dst:
        dst.destroy()


def ortho(gpu, name, new, src_fmt="rgba16", dst_fmt="rgba16", linearize=False):
    """one separable pass along the axis `new` = (new_w, new_h) rescales"""
    cfg = pl.filter_config(name, pl.FILTER_DOWNSCALING if min(new) < H else pl.FILTER_UPSCALING)
    src = gpu.tex_create(W, H, src_fmt, plane(src_fmt))
    dst = gpu.tex_create(new[0], new[1], dst_fmt)
    lut = pl.ShaderObj()
    sh = gpu.begin()
    assert sh.sample_ortho(src, cfg, lut, new_w=new[0], new_h=new[1]), gpu.messages[-3:]
    if linearize:
        sh.linearize(csp_of("bt1886"))
    assert sh.finish(dst), gpu.messages[-3:]
    lut.destroy(); src.destroy(); dst.destroy()


def deband(gpu, src_fmt="rgba16", dst_fmt="rgba16hf"):
    src = gpu.tex_create(W, H, src_fmt, plane(src_fmt))
    dst = gpu.tex_create(W, H, dst_fmt)
    gpu.reset_frame()
    sh = gpu.begin()
    assert sh.deband(src), gpu.messages[-3:]
    assert sh.finish(dst), gpu.messages[-3:]
    src.destroy(); dst.destroy()


def deinterlace(gpu, fmt, algo, dst_fmt=None):
    tex = [gpu.tex_create(W, H, fmt, np.roll(plane(fmt), 3 * i, axis=1)) for i in range(3)]
    dst = gpu.tex_create(W, H, dst_fmt or fmt)
    sh = gpu.begin()
    sh.deinterlace(tex[1], tex[0], tex[2], algo=algo)
    assert sh.finish(dst), gpu.messages[-3:]
    for t in tex + [dst]:
        t.destroy()


def polar(gpu, scale):
    ewa = pl.filter_config("ewa_lanczos")
    render(gpu, scale=(scale, scale), size=(96, 64), upscaler=ewa, downscaler=pl.filter_config("ewa_lanczos", pl.FILTER_DOWNSCALING))


YADIF, BOB = pl.DEINTERLACE_YADIF, pl.DEINTERLACE_BOB
PEAK = pl.peak_detect_params(percentile=99.995)

# (id, what to run, switches, the complete trace)
ROWS = [
    # -- 1:1 passes: plh_launch_pass (k_pass.hip)
    ("nearest_fast", lambda g: render(g, scale=(2, 3), upscaler=pl.filter_config("nearest")), {},
     ["k_pass_native", "k_nearest_fast"]),
    ("nearest_fast-f16-source", lambda g: render(g, src_fmt="rgba16hf", upscaler=pl.filter_config("nearest")), {},
     ["k_nearest_fast"]),
    ("bilinear_fast", lambda g: render(g, scale=(2, 2)), {}, ["k_bilinear_fast"]),
    ("bilinear_fast-4-cells", lambda g: render(g, scale=(2, 2)), {"PL_HIP_BILIN_ITERS": "4"}, ["k_bilinear_fast"]),
    ("bilinear-switched-off", lambda g: render(g, scale=(2, 2)), {"PL_HIP_BILIN_ITERS": "0"}, ["k_pass_generic"]),
    ("merge", render_planar, {}, ["k_pass_merge"]),
    ("merge-switched-off", render_planar, {"PL_HIP_PASS_NATIVE": "0"}, ["k_pass_generic"]),
    ("mix", render_mix, {}, ["k_pass_native", "k_pass_native", "k_pass_mix"]),
    ("mix-switched-off", render_mix, {"PL_HIP_PASS_NATIVE": "0"}, ["k_pass_generic", "k_pass_generic", "k_pass_generic"]),
    ("features", features_pass, {}, ["k_pass_features"]),
    ("features-switched-off", features_pass, {"PL_HIP_PASS_NATIVE": "0"}, ["k_pass_generic"]),
    ("chain-into-rgba16", lambda g: render(g, "default", hdr=True), {}, ["k_peak_tiles", "k_pass_chain"]),
    ("chain-into-rgba16hf", lambda g: render(g, "default", scale=(2, 2)), {},
     ["k_pass_chain", "k_ortho_fast", "k_ortho_fast"]),
    ("chain-contrast-recovery", lambda g: render(g, "high_quality", hdr=True), {},
     ["k_deband_lds", "k_peak_tiles", "k_lowpass2", "k_pass_chain"]),
    ("native", lambda g: render(g, "default", hdr=True), {"PL_HIP_MAP_CHAIN": "0"}, ["k_peak_tiles", "k_pass_native"]),
    ("native-into-rgba16hf", lambda g: render(g, "default", scale=(2, 2)), {"PL_HIP_MAP_CHAIN": "0"},
     ["k_pass_native", "k_ortho_fast", "k_ortho_fast"]),
    ("native-97x61", lambda g: render(g, "default", hdr=True, size=(97, 61)), {}, ["k_pass_peak", "k_pass_generic"]),
    ("native-switched-off", lambda g: render(g, "default", hdr=True), {"PL_HIP_PASS_NATIVE": "0"},
     ["k_peak_tiles", "k_pass_generic"]),
    # -- the measuring pass: plh_launch_peak (k_peak.hip)
    ("peak_tiles-pq", peak, {}, ["k_peak_tiles"]),
    ("peak_tiles-linear-f16", lambda g: peak(g, "linear", "rgba16hf"), {}, ["k_peak_tiles"]),
    ("peak_tiles-no-target", lambda g: peak(g, target=None), {}, ["k_peak_tiles"]),
    ("peak-tiles-off", peak, {"PL_HIP_PEAK_TILES": "0"}, ["k_peak_fast"]),
    ("peak-fast-off", peak, {"PL_HIP_PEAK_FAST": "0"}, ["k_pass_peak"]),
    ("peak-97x61", lambda g: peak(g, w=97, h=61), {}, ["k_pass_peak"]),
    ("peak-one-pixel-wide", lambda g: peak(g, w=1), {}, ["k_peak_fast"]),
    ("peak-feature-plane-two-ops", lambda g: peak(g, "linear", "rgba16hf", target="r16hf", features=True), {},
     ["k_peak_tiles"]),
    ("peak-feature-plane-three-ops", lambda g: peak(g, target="r16hf", features=True), {}, ["k_peak_tiles"]),
    ("peak-feature-plane-tiles-off", lambda g: peak(g, target="r16hf", features=True), {"PL_HIP_PEAK_TILES": "0"},
     ["k_peak_fast"]),
    ("peak-feature-plane-fast-off", lambda g: peak(g, target="r16hf", features=True), {"PL_HIP_PEAK_FAST": "0"},
     ["k_pass_peak"]),
    # -- separable scalers: plh_launch_ortho (k_ortho.hip)
    ("ortho-4-taps", lambda g: ortho(g, "mitchell", (2 * W, H)), {}, ["k_ortho_fast"]),
    ("ortho-6-taps-vertical", lambda g: ortho(g, "lanczos", (W, 2 * H)), {}, ["k_ortho_fast"]),
    ("ortho-8-taps", lambda g: ortho(g, "mitchell", (48, H)), {}, ["k_ortho_fast"]),
    ("ortho-14-taps", lambda g: ortho(g, "mitchell", (28, H)), {}, ["k_ortho_fast"]),
    ("ortho-16-taps-vertical", lambda g: ortho(g, "lanczos", (W, 24)), {}, ["k_ortho_fast"]),
    ("ortho-linear-4-taps", lambda g: ortho(g, "bicubic", (2 * W, H)), {}, ["k_ortho_fast"]),
    ("ortho-linear-6-taps", lambda g: ortho(g, "bicubic", (64, H)), {}, ["k_ortho_fast"]),
    ("ortho-linear-10-taps", lambda g: ortho(g, "gaussian", (39, H)), {}, ["k_ortho_fast"]),
    ("ortho-plane", lambda g: ortho(g, "lanczos", (2 * W, H), "r8", "r16hf"), {}, ["k_ortho_fast"]),
    ("ortho-plane-with-colour-ops", lambda g: ortho(g, "lanczos", (2 * W, H), "r8", "r16hf", linearize=True), {},
     ["k_ortho"]),
    ("ortho-with-colour-ops", lambda g: ortho(g, "lanczos", (2 * W, H), dst_fmt="rgba16hf", linearize=True), {},
     ["k_ortho_fast"]),
    ("ortho-switched-off", lambda g: ortho(g, "lanczos", (2 * W, H)), {"PL_HIP_ORTHO_FAST": "0"}, ["k_ortho"]),
    # -- debanding: plh_launch_deband (k_deband.hip)
    ("deband_lds", deband, {}, ["k_deband_lds"]),
    ("deband-lds-off", deband, {"PL_HIP_DEBAND_LDS": "0"}, ["k_deband_fast"]),
    ("deband-fast-off", deband, {"PL_HIP_DEBAND_FAST": "0"}, ["k_deband"]),
    ("deband-r8-plane", lambda g: deband(g, "r8", "r16hf"), {}, ["k_deband"]),
    # -- the deinterlacer: plh_launch_deinterlace (k_deinterlace.hip); names read by hand, see above
    ("deint-r8-bob", lambda g: deinterlace(g, "r8", BOB), {}, ["k_deint_rows"]),
    ("deint-r8-yadif", lambda g: deinterlace(g, "r8", YADIF), {}, ["k_deint_rows_yadif"]),
    ("deint-r8-into-floats", lambda g: deinterlace(g, "r8", BOB, "r32f"), {}, ["k_deint_rows"]),
    ("deint-rg16-yadif", lambda g: deinterlace(g, "rg16", YADIF), {}, ["k_deint_rows_yadif"]),
    ("deint-rg16-yadif-into-floats", lambda g: deinterlace(g, "rg16", YADIF, "rg32f"), {}, ["k_deint_rows_yadif"]),
    ("deint-rgba16-bob", lambda g: deinterlace(g, "rgba16", BOB), {}, ["k_deint_rows"]),
    ("deint-rgba16-yadif", lambda g: deinterlace(g, "rgba16", YADIF), {}, ["k_deinterlace"]),
    ("deint-float-texture", lambda g: deinterlace(g, "rgba32f", YADIF), {}, ["k_deinterlace"]),
    ("deint-r8-into-rgba", lambda g: deinterlace(g, "r8", BOB, "rgba16hf"), {}, ["k_deinterlace"]),
    # -- polar scalers: plh_launch_polar (k_polar.hip)
    ("polar_mxd", lambda g: polar(g, 0.5), {"PL_HIP_POLAR_MFMA": "1"}, ["k_polar_mxd"]),
    ("polar_mxr", lambda g: polar(g, 3), {"PL_HIP_POLAR_MFMA": "1"}, ["k_polar_mxr"]),
    ("polar_mxp", lambda g: polar(g, 2), {"PL_HIP_POLAR_MFMA": "1"}, ["k_polar_mxp"]),
    ("polar_mx", lambda g: polar(g, 2), {"PL_HIP_POLAR_MFMA": "1", "PL_HIP_MX_PERSIST": "0"}, ["k_polar_mx"]),
    ("polar_pp", lambda g: polar(g, 2), {"PL_HIP_POLAR_MFMA": "0"}, ["k_polar_pp"]),
    ("polar-per-pixel", lambda g: polar(g, 2), {"PL_HIP_POLAR_MFMA": "0", "PL_HIP_POLAR_PER_PIXEL": "1"}, ["k_polar"]),
]


@pytest.mark.parametrize("run,switches,want", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_kernel_ladder(gpu, capfd, run, switches, want):
    with util.kernel_trace(capfd, **switches) as kernels:
        run(gpu)
    print("kernel ladder:", kernels)
    assert kernels == want, kernels
