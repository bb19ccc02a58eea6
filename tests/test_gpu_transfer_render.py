"""The transfer curves as the RENDERER's kernels evaluate them -- the compile-time instances
lin_values<TRC, N> / delin_values<TRC, N, RESCALED> (transfer.hiph: sRGB, BT.1886, PQ and the shared
power-law instance), reached only from kernels the shader-level API does not launch -- against the
float64 truth of tests/transfer_f64.py, behind a texel decode (rgba16 / rgba16hf) instead of rgba32f.

Every case reads the launcher's trace (PL_HIP_PASS_TRACE: "[plh] kernel <name>") and asserts WHICH
kernel took the launch, with the library's default selection and with the native 1:1 kernels switched
off (PL_HIP_PASS_NATIVE=0: the op interpreter, k_pass_generic), so that neither can pass by silently
running the other.

1:1, per curve (sRGB, BT.1886, gamma 2.2, gamma 2.8, ST 428, ProPhoto, HLG, PQ):
* a 256 x 256 rgba16 frame with every code (three planes) tagged (BT.709, curve) into a target tagged
  (BT.709, linear): rgba32f (the interpreter, whatever the switch says: the native kernels store 16-bit
  formats only) and rgba16hf (k_pass_native by default). Bound: that of
  test_gpu_transfer_sweep.py per sample, plus half an f16 ulp where the target is rgba16hf.
* the reverse: the linear images of every code (moved 0.44 code towards the rounding boundary in two of
  the planes) as an rgba32f and as an rgba16hf frame into an rgba16 target tagged with the curve. The stored code must be round(truth * 65535), the truth taken from
  the fp32 / f16 value the kernel was given; where the truth lies within the sweep's bound of a rounding
  boundary either neighbour may be stored. tests/test_transfer_f64.py::
  test_oracle_alone_stores_the_right_code checks on the CPU that the oracle meets this on every sample.

Scaling: the scalers linearise while staging. The source is an 8 x 8 grid of 32 x 32 blocks of constant
colour whose 192 values are drawn from the knees, the codes next to black and the top of the range;
output pixels farther from every block edge than the filter's radius reproduce the constant, so they
are lin(code) up to the contraction's normalisation error (4e-6 of the data's scale,
util.assert_polar_equal) and -- the scalers work on f16 planes and tiles -- the f16 roundings stated per
path in SCALERS, which also says where on each path the curve sits. At least half of every block's
pixels take part. What this sees is therefore what f16 resolves: a wrong curve, a missing black
scaling (next to black an f16 ulp is 1e-6 of the range), a wrong branch of a curve whose pieces differ.
"""

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import transfer_f64 as t64
from test_transfer_f64 import RENDER_CURVES, luma_coeffs, nominal, oracle
from util import env

pytestmark = pytest.mark.gpu

# PQ and HLG: source and target carry the same luminance range, so that the renderer has nothing to
# tone-map and the frame is the curve alone
HDR = dict(min_luma=0.005, max_luma=1000.0)


def color_kw(trc):
    return dict(HDR) if trc in ("pq", "hlg") else {}




def render(gpu, capfd, img, sfmt, scsp, dw, dh, dfmt, dcsp, params, **e):
    """one frame through a fresh renderer -> (frame, the kernels that took its launches)"""
    h, w = img.shape[:2]
    capfd.readouterr()
    with env(PL_HIP_PASS_TRACE="1", **e):
        rr = pl.Renderer(gpu)
        src = gpu.tex_create(w, h, sfmt, img)
        dst = gpu.tex_create(dw, dh, dfmt)
        assert rr.render(pl.frame(src, components=3, color=scsp), pl.frame(dst, color=dcsp), params), \
            gpu.messages[-4:]
        assert rr.errors() == 0
        out = dst.download()
        rr.destroy(); src.destroy(); dst.destroy()
    kernels = [ln.split()[-1] for ln in capfd.readouterr().err.splitlines()
               if ln.startswith("[plh] kernel ")]
    return out, kernels


def codes16():
    v = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    img = np.full((256, 256, 4), 65535, np.uint16)
    img[..., 0], img[..., 1], img[..., 2] = v, v[::-1, ::-1], v.T
    return img


def the_case(trc, direction):
    kw = color_kw(trc)
    csp = pl.color_space("bt709", trc, **kw)
    mn, mx = nominal(csp)
    return t64.Case(direction, trc, mn, mx, luma_coeffs(csp.primaries))


# which kernel takes the 1:1 pass: (target / source format of the linear side, PL_HIP_PASS_NATIVE)
def expect_1to1(fmt, native, forward):
    if fmt == "rgba32f" or native == "0":
        return "k_pass_generic"
    # into the f16 intermediate: the plain native kernel (op_linearize_px); out of it into a 16-bit
    # target: the straight-line chain (run_map_chain: op_delinearize_px)
    return "k_pass_native" if forward else "k_pass_chain"


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("dfmt", ["rgba32f", "rgba16hf"])
@pytest.mark.parametrize("trc", RENDER_CURVES)
def test_linearize_1to1_through_the_renderer(gpu, capfd, trc, dfmt, native):
    case = the_case(trc, "linearize")
    img = codes16()
    if t64.is_grey(trc):
        img[..., 1] = img[..., 2] = img[..., 0]
    kw = color_kw(trc)
    out, kernels = render(gpu, capfd, img, "rgba16", pl.color_space("bt709", trc, **kw), 256, 256, dfmt,
                          pl.color_space("bt709", "linear", **kw), pl.render_params("fast"),
                          PL_HIP_PASS_NATIVE=native)
    assert kernels == [expect_1to1(dfmt, native, True)], kernels
    x = orc.tex_decode(img, "rgba16")[..., :3]
    g = t64.Report([case.measure_image(x, out.astype(np.float32))])
    o = t64.Report([case.measure_image(x, oracle(case, x))])
    ex = t64.excess_linear(case, g, o, f16=dfmt == "rgba16hf")
    with capfd.disabled():
        print("\n1:1 %-8s -> linear %-8s on %-14s max error %8.4g (well %8.4g), oracle %8.4g (well %8.4g); "
              "largest excess over the bound %.3g" % (trc, dfmt, kernels[0], g.E, g.E_well, o.E, o.E_well,
                                                      ex.max()))
    assert np.isfinite(g.got).all()
    assert ex.max() <= 0, (trc, float(ex.max()), g.x[ex.argmax()], g.got[ex.argmax()], g.truth[ex.argmax()])
    assert np.all(out[..., 3] == 1.0)


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("sfmt", ["rgba32f", "rgba16hf"])
@pytest.mark.parametrize("trc", RENDER_CURVES)
def test_delinearize_1to1_through_the_renderer(gpu, capfd, trc, sfmt, native):
    case = the_case(trc, "delinearize")
    dt = np.float32 if sfmt == "rgba32f" else np.float16
    # the linear images of every code, moved 0.44 code up (R), down (G) and not at all (B): a stored
    # code is most easily wrong next to a rounding boundary, and least easily on the code itself
    c = t64.codes()
    off = (0.44, 0.44, 0.44) if t64.is_grey(trc) else (0.44, -0.44, 0.0)
    enc = np.stack([np.clip(c + f * t64.H, 0.0, 1.0) for f in off], -1)
    lin = t64.linearize(enc, trc, case.mn, case.mx, case.luma)
    lin = np.stack([t64.planes(lin[..., k], True)[..., 0] if k == 0 else
                    (lin[..., k].reshape(256, 256)[::-1, ::-1] if k == 1 else lin[..., k].reshape(256, 256).T)
                    for k in range(3)], -1)
    if t64.is_grey(trc):
        lin[..., 1] = lin[..., 2] = lin[..., 0]
    src = np.ones((256, 256, 4), dt)
    src[..., :3] = lin.astype(dt)
    kw = color_kw(trc)
    out, kernels = render(gpu, capfd, src, sfmt, pl.color_space("bt709", "linear", **kw), 256, 256, "rgba16",
                          pl.color_space("bt709", trc, **kw),
                          pl.render_params("fast", dither_params=None), PL_HIP_PASS_NATIVE=native)
    assert kernels == [expect_1to1(sfmt, native, False)], kernels
    x = src[..., :3].astype(np.float32)     # what the kernel was given
    ref = oracle(case, x)
    o = t64.Report([case.measure_image(x, ref)])
    g = t64.Report([case.measure_image(x, out[..., :3].astype(np.float64) / 65535.0)])
    ex = t64.excess_stored(out[..., :3], g, o)
    wrong = np.ravel(out[..., :3]).astype(np.int64) != np.rint(np.clip(g.truth, 0, 1) * 65535).astype(np.int64)
    with capfd.disabled():
        print("\n1:1 linear %-8s -> %-8s on %-14s %d of %d codes are not round(truth) (all next to a rounding "
              "boundary: largest excess over the bound %.3g)" % (sfmt, trc, kernels[0], int(wrong.sum()),
                                                                  wrong.size, ex.max()))
    assert ex.max() <= 0, (trc, float(ex.max()), g.x[ex.argmax()], np.ravel(out[..., :3])[ex.argmax()],
                           g.truth[ex.argmax()] * 65535)
    assert np.all(out[..., 3] == 65535)
    # the sweep covers the code range (the f16 frame: what f16 resolves of it)
    assert np.unique(out[..., 0]).size > (60000 if sfmt == "rgba32f" else 2000)


# ---- scaling ---------------------------------------------------------------------------------
def block_values(trc, n):
    """n * n * 3 sixteen-bit codes: next to black, the top of the range, either side of each knee, and
    random ones -- a third each, shuffled so that a texel's channels come from different sets"""
    case = the_case(trc, "linearize")
    count = n * n * 3
    third = count // 3
    vals = list(range(third // 2)) + list(range(65536 - (third - third // 2), 65536))
    for tri in t64.knee_inputs(trc, "linearize", case.mn, case.mx):
        c = int(round(float(tri[len(tri) // 2]) * 65535))
        vals += list(range(max(c - third // 2, 0), c + third // 2))
    rng = np.random.default_rng(7)
    vals += list(rng.integers(0, 65536, count))
    vals = np.asarray(vals[:count], np.uint16)
    return rng.permutation(vals).reshape(n, n, 3)


def block_frame(vals, block):
    n = vals.shape[0]
    img = np.full((n * block, n * block, 4), 65535, np.uint16)
    img[..., :3] = np.repeat(np.repeat(vals, block, 0), block, 1)
    return img


SCALERS = {
    # name: (output size / source size, params, radius in source texels, block size, target format,
    # the kernels that must take the frame's launches, where the curve sits, f16 roundings)
    # Blocks: 32 x 32 in an 8 x 8 grid (192 values); the downscale's widened kernel (radius 6.48
    # texels) leaves a third of such a block, so it gets 64 x 64 blocks in a 4 x 4 grid (48 values).
    # Where the curve sits (the passes' op lists, PL_HIP_PASS_TRACE):
    # * "staging": a downscale runs in linear light. k_polar_mxd linearises the decoded rgba16 texel
    #   while it stages it, as f16: the output is f16(lin(code)) up to the contraction's error and
    #   the f16 store of that -- two f16 half-ulps at most (the second only where 4e-6 is worth one).
    # * "epilogue": an upscale without sigmoidisation runs in gamma light (renderer.c:1997-2003) on
    #   the f16 plane, and the curve is the first op behind the contraction: its input is f16(code) up
    #   to the contraction's error (and, on the separable path, one more f16 store between the two
    #   passes), which the curve's slope carries into the output.
    "ewa_lanczos 2:1 down": (0.5, lambda: pl.render_params(
        "fast", downscaler=pl.filter_config("ewa_lanczos", pl.FILTER_DOWNSCALING)),
        2 * orc.JINC_R3, 64, "rgba16hf", ["k_polar_mxd"], "staging", 2),
    "ewa_lanczos 2x up": (2.0, lambda: pl.render_params(
        "fast", upscaler=pl.filter_config("ewa_lanczos"), sigmoid_params=None),
        orc.JINC_R3, 32, "rgba32f", ["k_polar_mx"], "epilogue", 0),
    "lanczos 2x up": (2.0, lambda: pl.render_params(
        "fast", upscaler=pl.filter_config("lanczos"), sigmoid_params=None),
        3.0, 32, "rgba32f", ["k_pass_native", "k_ortho_fast", "k_ortho_fast"], "epilogue", 1),
}


@pytest.mark.parametrize("scaler", list(SCALERS))
@pytest.mark.parametrize("trc", ["srgb", "bt1886", "gamma22", "pq", "prophoto"])
def test_linearize_inside_the_scalers(gpu, capfd, trc, scaler):
    ratio, params, radius, block, dfmt, want, where, n16 = SCALERS[scaler]
    case = the_case(trc, "linearize")
    nb = 256 // block
    vals = block_values(trc, nb)
    img = block_frame(vals, block)
    n = int(256 * ratio)
    kw = color_kw(trc)
    out, kernels = render(gpu, capfd, img, "rgba16", pl.color_space("bt709", trc, **kw), n, n, dfmt,
                          pl.color_space("bt709", "linear", **kw), params(), PL_HIP_POLAR_MFMA="1")
    assert kernels == want, (scaler, kernels)
    # Output pixels farther from every block edge than the filter's radius: pixel m of a block (from
    # its edge) samples (m + 0.5) / ratio texels inside it, and every tap's texel lies in the block
    # once that is the radius -- m >= ceil(radius * ratio) with half a texel to spare.
    bs = int(block * ratio)
    margin = int(np.ceil(radius * ratio))
    inner = np.zeros(bs, bool)
    inner[margin:bs - margin] = True
    mask = np.tile(inner, nb)[:, None] & np.tile(inner, nb)[None, :]
    assert mask.reshape(nb, bs, nb, bs).mean(axis=(1, 3)).min() >= 0.5, (bs, margin)
    x = np.repeat(np.repeat(orc.tex_decode(img, "rgba16")[::block, ::block, :3], bs, 0), bs, 1)
    xm = np.ascontiguousarray(x[mask])
    got = out[..., :3][mask].astype(np.float32)
    scale_in = 4e-6 * max(1.0, float(xm.max()))
    if where == "staging":
        g = t64.Report([case.measure_image(xm, got)])
        o = t64.Report([case.measure_image(xm, oracle(case, xm[None])[0])])
        h16 = t64.f16_half_ulp(g.truth)
        extra = 4e-6 * max(1.0, float(np.abs(g.truth).max())) + (n16 - 1) * h16
        ex = t64.excess_linear(case, g, o, f16=True, extra=extra)
    else:
        xin = xm.astype(np.float16).astype(np.float32)      # what the curve is given
        g = t64.Report([case.measure_image(xin, got)])
        o = t64.Report([case.measure_image(xin, oracle(case, xin[None])[0])])
        h16 = t64.f16_half_ulp(g.truth)
        d = scale_in + n16 * t64.f16_half_ulp(xin.astype(np.float64))
        x64 = xin.astype(np.float64)
        moved = np.maximum(np.abs(case.fn(x64 + d) - case.fn(x64)), np.abs(case.fn(x64 - d) - case.fn(x64)))
        ex = t64.excess_linear(case, g, o, f16=dfmt == "rgba16hf", extra=np.ravel(moved))
    with capfd.disabled():
        print("\n%-22s %-8s on %s: %d pixels compared (%.2f of every block), max |out - truth| %.3g, "
              "%.2f f16 half-ulps of it at most, largest excess over the bound %.3g"
              % (scaler, trc, kernels, int(mask.sum()), mask.mean(), np.abs(g.got - g.truth).max(),
                 (np.abs(g.got - g.truth) / h16).max(), ex.max()))
    assert np.isfinite(out).all()
    assert ex.max() <= 0, (trc, scaler, float(ex.max()), g.x[ex.argmax()], g.got[ex.argmax()],
                           g.truth[ex.argmax()])
