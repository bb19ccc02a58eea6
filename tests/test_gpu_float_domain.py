"""Float sources outside [0, 1]: non-finite texels stay local, and the f16 range on the matrix pipe.

1. Containment (tests/test_float_domain_ref.py has the statement, the zones and the geometries, and
   holds the oracle to them on the CPU). Frame B is frame A with six texels replaced (+-Inf, two NaNs,
   +-65504); `out(B) == out(A)` bit for bit at every output pixel outside the bad texels' zones, on every
   kernel and target format. Inside the zones the kernels that are held bit-exact to the oracle
   (k_polar_pp, k_ortho / k_ortho_fast, the simple samplers) equal the oracle on float targets, NaN
   matching NaN; the matrix-pipe kernels stage non-finite texels as +-65504 (mx_tile.hiph) and give
   large finite values there instead: nothing is asserted inside. Frame F carries the two finite
   extremes only and is held to the same statement on its own.
2. The f16 range on the matrix pipe: the noise of tests/test_gpu_polar_mfma.py times S = 2^-10 (mostly
   f16 subnormals), 1, 2^5 and 2^14 (just under the f16 maximum), positive and with a random sign per
   sample. k_polar_pp is exactly homogeneous (scaling by a power of two and negation are exact in f16
   and in an fp32 fma chain); the matrix pipe keeps its bound against it, carried by homogeneity.
3. The per-pixel fast paths with bad lanes: the HDR map chain (behind the metric's launch and as a 1 : 1
   k_pass_chain pass) and the measuring pass (k_peak_tiles / k_peak_fast against k_pass_peak) on f16
   sources with the bad texels added.

Every case asserts from the launcher's trace that the kernel it names took the pass.
"""
import re

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util
from libplacebo_amd import _capi as capi
from test_float_domain_ref import (FINITE_BAD, MIN_SHARE, NAMES, bad_positions, compared, frames, geometries,
                                   poison, same_bits)
from test_gpu_polar_mfma import _traced, dither10, ewa, ewa_down, render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    """a backend of this file's own (the passes by hand; the renderer cases open theirs in render())"""
    assert pl.hip_device_count() >= 1, "no HIP device visible"
    with pl.HipGpu(0) as gpu:
        yield gpu


def contained(name, what, geo, out_a, out_b, which=range(6), nch=3):
    """the statement: `out_b == out_a` bit for bit outside the zones of the bad texels `which`; prints how
    many pixels differ inside and outside, and how far from a bad texel (source texels, per axis) the
    furthest differing pixel lies"""
    keep = compared(geo, which)
    assert keep.mean() >= MIN_SHARE, (name, keep.mean())
    assert out_a.shape == out_b.shape == keep.shape + (out_a.shape[-1],)
    diff = ~same_bits(out_a[..., :nch], out_b[..., :nch]).all(axis=-1)
    ys, xs = np.nonzero(diff)
    reach = (0.0, 0.0)
    if len(ys):
        x0, y0, x1, y1 = geo["rect"]
        cx = x0 + (xs + 0.5) * ((x1 - x0) / geo["dw"]) - 0.5
        cy = y0 + (ys + 0.5) * ((y1 - y0) / geo["dh"]) - 0.5
        bad = np.array([geo["bad"][i] for i in which], np.float64)
        dx = np.abs(cx[:, None] - bad[None, :, 0])
        dy = np.abs(cy[:, None] - bad[None, :, 1])
        near = np.argmin(np.hypot(dx, dy), axis=1)
        reach = (float(dx[np.arange(len(ys)), near].max()), float(dy[np.arange(len(ys)), near].max()))
    outside = diff & keep
    print("%s [%s]: %.1f %% compared; %d pixels differ inside the zones, %d outside; furthest differing pixel "
          "%.1f columns / %.1f rows of source texels from its bad texel; non-finite samples: %d"
          % (name, what, 100 * keep.mean(), (diff & ~keep).sum(), outside.sum(), reach[0], reach[1],
             0 if out_b.dtype.kind in "ui" else (~np.isfinite(out_b[..., :nch].astype(np.float32))).sum()))
    assert not outside.any(), (name, what, int(outside.sum()), np.argwhere(outside)[:6].tolist())
    return keep


# ---- 1. containment: polar ------------------------------------------------------------------------
SIGMOID = dict(sigmoid_params=capi.SigmoidParams(0.75, 6.5))
F32 = dict(src_fmt="rgba16hf", dst_fmt="rgba32f")
U16 = dict(src_fmt="rgba16hf", dst_fmt="rgba16")
F16 = dict(src_fmt="rgba16hf", dst_fmt="rgba16hf")
CROP = dict(image_kw=dict(crop=(7, 13, 407, 193)))

# id: (geometry, kernel, matrix pipe, PL_HIP_* switches, render_params, render() keywords)
POLAR = {}
for _s in ("96x64", "130x77"):
    POLAR["pp-" + _s] = ("polar-2x-" + _s, "k_polar_pp", False, {}, ewa, dict(F32))
    POLAR["mx-c3-" + _s] = ("polar-2x-" + _s, "k_polar_mx", True, dict(PL_HIP_MX_PERSIST="0"), ewa, dict(F32))
    POLAR["mx-c4-" + _s] = ("polar-2x-alpha-" + _s, "k_polar_mx", True, dict(PL_HIP_MX_PERSIST="0"), ewa,
                            dict(F32, components=4))
    POLAR["mxp-rgba16-" + _s] = ("polar-2x-" + _s, "k_polar_mxp", True, dict(PL_HIP_MX_PERSIST="1"), ewa, dict(U16))
    POLAR["mxp-dither10-" + _s] = ("polar-2x-" + _s, "k_polar_mxp", True, dict(PL_HIP_MX_PERSIST="1"),
                                   lambda: ewa(**dither10()), dict(U16, ten_bit=True))
for _r in ("3x", "4x", "3:2"):
    POLAR["mxr-%s-80x48" % _r] = ("polar-%s-80x48" % _r, "k_polar_mxr", True, {}, ewa, dict(U16))
POLAR["mxd-128x64"] = ("polar-2:1-128x64", "k_polar_mxd", True, {}, ewa_down, dict(F16))
POLAR["mxd-200x90"] = ("polar-2:1-200x90", "k_polar_mxd", True, {}, ewa_down, dict(F16))
POLAR["mxd-crop-200x90"] = ("polar-2:1-crop-200x90", "k_polar_mxd", True, {}, ewa_down, dict(F16, **CROP))
POLAR["pp-2:1-128x64"] = ("polar-2:1-128x64", "k_polar_pp", False, {}, ewa_down, dict(F32))
# pre-ops in front of the tile: linearize + sigmoidize of an rgba16hf source (the interpreter's
# values packed into the planes, mx_pair_pack)
# (PL_HIP_NO_FUSION=0: fused wherever it is valid -- by default the renderer keeps an upscale's transfer
# functions in a pass of their own and fuses the cheap ops only)
FUSED = dict(PL_HIP_MX_PERSIST="0", PL_HIP_NO_FUSION="0")
POLAR["mx-preops-130x77"] = ("polar-2x-130x77", "k_polar_mx", True, FUSED, lambda: ewa(**SIGMOID), dict(U16))


# ... and of an rgba32f source (one texel at a time through the generic fetch; the finite +-65504 are far
# beyond the f16 range once linearized), on the matrix pipe and on k_polar_pp's f16 tile
F32SRC = dict(src_fmt="rgba32f", dst_fmt="rgba16")
POLAR["mx-f32-preops-130x77"] = ("polar-2x-130x77", "k_polar_mx", True, FUSED, lambda: ewa(**SIGMOID), dict(F32SRC))
POLAR["pp-f32-preops-130x77"] = ("polar-2x-130x77", "k_polar_pp", False, FUSED, lambda: ewa(**SIGMOID), dict(F32SRC))


def traced_pre_ops(capfd, want, *a, **kw):
    """test_gpu_polar_mfma's _traced, and from the pass's own trace line the number of pre-ops in front
    of the taps"""
    capfd.readouterr()
    with util.env(PL_HIP_PASS_TRACE="1"):
        out = render(*a, **kw)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plh] ")]
    at = [i for i, ln in enumerate(lines) if ln.startswith("[plh] kernel k_polar")]
    assert [lines[i].split()[-1] for i in at] == [want], (want, lines)
    passes = [ln for ln in lines[:at[0]] if ln.startswith("[plh] pass ")]
    return out, int(re.search(r" pre=(\d+) ", passes[-1]).group(1))


@pytest.mark.parametrize("case", list(POLAR))
def test_polar_bad_texels_stay_local(case, capfd):
    """A matrix-pipe kernel that stages a non-finite texel as it is turns the whole band of its wave tile
    into NaN (k_polar_mxd: its whole source tile), far outside the zones; k_polar_pp on its tabulated taps is
    NaN on the few pixels whose dead taps, weight zero, meet the texel. With sampled alpha or pre-ops in
    front of the tile the finite +-65504 overflow f16 on their way in and do the same."""
    name, kernel, mfma, switches, params, kw = POLAR[case]
    geo = geometries()[name]
    nch = kw.get("components", 3)
    a, b, f = frames(geo)
    if kw["src_fmt"] == "rgba32f":
        a = a.astype(np.float32)
        b, f = poison(a, geo["bad"]), poison(a, geo["bad"], which=FINITE_BAD)
    outs = []
    with util.env(**switches):
        for img in (a, b, f):
            out, pre = traced_pre_ops(capfd, kernel, img, geo["dw"], geo["dh"], params(), mfma, **kw)
            # the pre-ops cases run them in front of the tile (linearize, sigmoidize: not the bit copy)
            assert pre >= 2 or "preops" not in case, (case, pre)
            outs.append(out)
    out_a, out_b, out_f = outs
    # the finite extremes first: they hold on every kernel
    contained(case, "+-65504 only", geo, out_a, out_f, which=FINITE_BAD, nch=nch)
    keep = contained(case, "all six", geo, out_a, out_b, nch=nch)
    if out_a.dtype.kind == "f":
        assert np.isfinite(out_b[keep][..., :nch].astype(np.float32)).all()
    if kernel == "k_polar_pp" and "preops" not in case:
        # the reference kernel IS the oracle, inside the zones as well
        for img, out in ((a, out_a), (b, out_b)):
            ref = geo["oracle"](geo, img)[..., :3]
            bad = ~(same_bits(out[..., :3], ref) | (np.isnan(out[..., :3]) & np.isnan(ref)))
            print("  k_polar_pp against the oracle: %d samples differ (%d of them NaN in the kernel's frame only, "
                  "%d in the oracle's only); the oracle's frame has %d NaN samples"
                  % (bad.sum(), (bad & np.isnan(out[..., :3]) & ~np.isnan(ref)).sum(),
                     (bad & ~np.isnan(out[..., :3]) & np.isnan(ref)).sum(), np.isnan(ref).sum()))
            assert not bad.any(), np.argwhere(bad)[:6].tolist()


# ---- 1. containment: separable ---------------------------------------------------------------------
ORTHO_NAMES = [n for n in NAMES if n.startswith("ortho-") and "two-pass" not in n]


def run_ortho(g, geo, img, capfd, kernel, switches):
    t = g.tex_create(geo["sw"], geo["sh"], "rgba16hf", img)
    d = g.tex_create(geo["dw"], geo["dh"], "rgba32f")
    lut = pl.ShaderObj()
    with util.kernel_trace(capfd, **switches) as kernels:
        sh = g.begin()
        assert sh.sample_ortho(t, pl.filter_config(geo["filter"]), lut, new_w=geo["dw"], new_h=geo["dh"],
                               components=4), g.messages[-3:]
        assert sh.finish(d), g.messages[-3:]
        out = d.download()
    t.destroy(); d.destroy(); lut.destroy()
    assert [k for k in kernels if k.startswith("k_ortho")] == [kernel], kernels
    return out


@pytest.mark.parametrize("kernel", ["k_ortho_fast", "k_ortho"])
@pytest.mark.parametrize("name", ORTHO_NAMES)
def test_separable_bad_texels_stay_local(g, name, kernel, capfd):
    geo = geometries()[name]
    switches = dict(PL_HIP_ORTHO_FAST="1" if kernel == "k_ortho_fast" else "0")
    a, b, f = frames(geo, alpha=True)
    out_a, out_b, out_f = (run_ortho(g, geo, img, capfd, kernel, switches) for img in (a, b, f))
    contained(name, kernel + ", +-65504 only", geo, out_a, out_f, which=FINITE_BAD, nch=4)
    contained(name, kernel, geo, out_a, out_b, nch=4)
    # both are held bit-exact to the oracle: inside the zones as well, NaN matching NaN
    for img, out in ((a, out_a), (b, out_b)):
        ref = geo["oracle"](geo, img)
        bad = ~(same_bits(out, ref) | (np.isnan(out) & np.isnan(ref)))
        print("  %s against the oracle: %d samples differ" % (kernel, bad.sum()))
        assert not bad.any(), np.argwhere(bad)[:6].tolist()


def test_two_pass_upscale_through_the_renderer(capfd):
    """the renderer's separable 2x upscale (vertical pass into an rgba16hf intermediate, horizontal
    pass): a bad texel reaches a rectangle"""
    geo = geometries()["ortho-two-pass-64x48"]
    params = pl.render_params("fast", upscaler=pl.filter_config("lanczos"))
    a, b, f = frames(geo)
    outs = []
    for img in (a, b, f):
        with util.kernel_trace(capfd) as kernels:
            outs.append(render(img, geo["dw"], geo["dh"], params, False, **F32))
        assert len([k for k in kernels if k.startswith("k_ortho")]) == 2, kernels
    contained("two-pass", "+-65504 only", geo, outs[0], outs[2], which=FINITE_BAD)
    contained("two-pass", "all six", geo, outs[0], outs[1])


# ---- 1. containment: the simple samplers -----------------------------------------------------------
def run_simple(g, geo, img, fmt, capfd):
    t = g.tex_create(geo["sw"], geo["sh"], fmt, img)
    d = g.tex_create(geo["dw"], geo["dh"], "rgba32f")
    with util.kernel_trace(capfd) as kernels:
        sh = g.begin()
        assert sh.sample(geo["kind"], t, new_w=geo["dw"], new_h=geo["dh"]), g.messages[-3:]
        assert sh.finish(d), g.messages[-3:]
        out = d.download()
    t.destroy(); d.destroy()
    assert len(kernels) == 1 and kernels[0].startswith("k_pass"), kernels
    return out


@pytest.mark.parametrize("fmt", ["rgba16hf", "rgba32f"])
@pytest.mark.parametrize("kind", ["bicubic", "hermite", "gaussian", "oversample", "bilinear", "nearest"])
def test_simple_samplers_bad_texels_stay_local(g, kind, fmt, capfd):
    geo = geometries()["simple-" + kind]
    a, b, f = frames(geo, alpha=True)
    if fmt == "rgba32f":
        a32 = a.astype(np.float32)
        a, b, f = a32, poison(a32, geo["bad"], alpha=True), poison(a32, geo["bad"], which=FINITE_BAD, alpha=True)
    out_a, out_b, out_f = (run_simple(g, geo, img, fmt, capfd) for img in (a, b, f))
    contained(kind, fmt + ", +-65504 only", geo, out_a, out_f, which=FINITE_BAD, nch=4)
    contained(kind, fmt, geo, out_a, out_b, nch=4)
    if kind != "gaussian":      # (v_exp_f32 against libm: within a code of the oracle, not bit-exact)
        for img, out in ((a, out_a), (b, out_b)):
            ref = geo["oracle"](geo, img)
            bad = ~(same_bits(out, ref) | (np.isnan(out) & np.isnan(ref)))
            print("  %s against the oracle: %d samples differ" % (kind, bad.sum()))
            assert not bad.any(), np.argwhere(bad)[:6].tolist()


# ---- 1. containment: deband ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deband-default-128x96", "deband-it3-r8-256x192"])
def test_deband_bad_texels_stay_local(g, name, capfd):
    """the general kernel (an rgba16hf source has no fast one); the same PRNG seed for both frames"""
    geo = geometries()[name]
    a, b, f = frames(geo)
    outs, seeds = [], []
    for img in (a, b, f):
        t = g.tex_create(geo["sw"], geo["sh"], "rgba16hf", img)
        d = g.tex_create(geo["dw"], geo["dh"], "rgba32f")
        with util.kernel_trace(capfd) as kernels:
            sh = g.begin()
            assert sh.deband(t, components=3, **geo["params"]), g.messages[-3:]
            seeds.append(int(sh.listing().split("seed=")[1].split(")")[0]))
            assert sh.finish(d), g.messages[-3:]
            outs.append(d.download())
        t.destroy(); d.destroy()
        assert kernels == ["k_deband"], kernels
    assert len(set(seeds)) == 1, seeds
    contained(name, "+-65504 only", geo, outs[0], outs[2], which=FINITE_BAD)
    contained(name, "all six", geo, outs[0], outs[1])
    # the pass did something: a good part of the samples took an average
    assert (outs[0][..., :3] != a[..., :3].astype(np.float32)).mean() > 0.1


# ---- 2. the f16 range on the matrix pipe ------------------------------------------------------------
SCALES = [2.0 ** -10, 1.0, 2.0 ** 5, 2.0 ** 14]
# name: (source size, target size, render_params, the matrix-pipe kernel, the existing tests' noise)
RANGE_GEO = {
    "2x-96x64": ((96, 64), (192, 128), ewa, "k_polar_mx", "unit"),
    "2x-130x77": ((130, 77), (260, 154), ewa, "k_polar_mx", "unit"),
    "3x-80x48": ((80, 48), (240, 144), ewa, "k_polar_mxr", "unit"),
    "4x-80x48": ((80, 48), (320, 192), ewa, "k_polar_mxr", "unit"),
    "3:2-80x48": ((80, 48), (120, 72), ewa, "k_polar_mxr", "unit"),
    "2:1-128x64": ((256, 128), (128, 64), ewa_down, "k_polar_mxd", "mid"),
    "2:1-200x90": ((400, 180), (200, 90), ewa_down, "k_polar_mxd", "mid"),
}


def range_source(name, scale, signed):
    (sw, sh), _, _, _, kind = RANGE_GEO[name]
    if kind == "unit":      # test_mx_sampled_alpha_and_f16_source
        img = np.random.default_rng(9).random((sh, sw, 4), dtype=np.float32)
    else:                   # test_mxd_2to1_downscale_vs_reference_kernel
        img = 0.05 + 0.9 * np.random.default_rng(11).random((sh, sw, 4), dtype=np.float32)
    img = img.astype(np.float16).astype(np.float32)
    if signed:
        img *= np.random.default_rng(13).choice(np.array([-1.0, 1.0], np.float32), img.shape)
    img[..., 3] = 1.0
    out = (img * np.float32(scale)).astype(np.float16)
    out[..., 3] = 1.0
    # a power of two times an f16 number is an f16 number (or a subnormal that rounds, below 1)
    assert scale < 1 or np.array_equal(out[..., :3].astype(np.float32), img[..., :3] * np.float32(scale))
    return out


_PP = {}


def pp_frame(capfd, name, scale, signed, dst_fmt):
    """k_polar_pp's frame of a source, rendered once per module"""
    key = (name, scale, signed, dst_fmt)
    if key not in _PP:
        _, (dw, dh), params, _, _ = RANGE_GEO[name]
        out = _traced(capfd, "k_polar_pp", range_source(name, scale, signed), dw, dh, params(), False,
                      src_fmt="rgba16hf", dst_fmt=dst_fmt, expect_mx=False)
        out.setflags(write=False)
        _PP[key] = out
    return _PP[key]


def mx_frame(capfd, name, scale, signed, dst_fmt):
    _, (dw, dh), params, kernel, _ = RANGE_GEO[name]
    with util.env(PL_HIP_MX_PERSIST="0"):
        return _traced(capfd, kernel, range_source(name, scale, signed), dw, dh, params(), True,
                       src_fmt="rgba16hf", dst_fmt=dst_fmt, expect_mx=True)


@pytest.mark.parametrize("name", ["2x-96x64", "2x-130x77", "3x-80x48", "2:1-128x64"])
def test_reference_kernel_is_exactly_homogeneous(name, capfd):
    """pp(S * img) == S * pp(img) for S >= 1 and pp(-img) == -pp(img), bit for bit, on rgba32f targets: a
    failure means range-dependent code in the kernel the whole suite leans on"""
    for signed in (False, True):
        base = pp_frame(capfd, name, 1.0, signed, "rgba32f")[..., :3]
        assert np.isfinite(base).all()
        for scale in SCALES[2:]:
            got = pp_frame(capfd, name, scale, signed, "rgba32f")[..., :3]
            assert np.isfinite(got).all()
            bad = ~same_bits(got, base * np.float32(scale))
            print("k_polar_pp %s x %g%s: %d samples differ from the scaled frame" %
                  (name, scale, " signed" if signed else "", bad.sum()))
            assert not bad.any()
    # negation: the positive frame, every sample negated
    (sw, sh), (dw, dh), params, _, _ = RANGE_GEO[name]
    neg = range_source(name, 1.0, False)
    neg[..., :3] = -neg[..., :3]
    got = _traced(capfd, "k_polar_pp", neg, dw, dh, params(), False, src_fmt="rgba16hf", dst_fmt="rgba32f")
    base = pp_frame(capfd, name, 1.0, False, "rgba32f")
    bad = ~same_bits(got[..., :3], -base[..., :3])
    print("k_polar_pp %s negated: %d samples differ" % (name, bad.sum()))
    assert not bad.any()


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("scale", SCALES, ids=["2^-10", "1", "2^5", "2^14"])
@pytest.mark.parametrize("name", ["2x-96x64", "2x-130x77"])
def test_matrix_pipe_fp32_against_reference_kernel_over_the_f16_range(name, scale, signed, capfd):
    """max |mx - pp| <= 4e-6 * max(S, 1): test_mx_vs_reference_kernel_and_oracle's bound on [0, 1] data,
    carried by homogeneity. Not tightened below S = 1, where the first-order term's f16 products round as
    subnormals -- the case catches a flush to zero (the source is then mostly f16 subnormals: a flushed
    tile gives a frame of zeros, 1e-3 away)."""
    pp = pp_frame(capfd, name, scale, signed, "rgba32f")
    mx = mx_frame(capfd, name, scale, signed, "rgba32f")
    assert np.isfinite(pp[..., :3]).all() and np.isfinite(mx[..., :3]).all()
    err = np.abs(mx[..., :3].astype(np.float64) - pp[..., :3])
    bound = 4e-6 * max(scale, 1.0)
    print("%s x %g%s: max |mx - pp| = %.3e (bound %.3e), max |pp| = %.4g" %
          (name, scale, " signed" if signed else "", err.max(), bound, np.abs(pp[..., :3]).max()))
    assert np.abs(pp[..., :3]).max() > 0.5 * scale
    assert err.max() <= bound, (err.max(), bound)


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("scale", SCALES[:2], ids=["2^-10", "1"])
@pytest.mark.parametrize("name", ["3x-80x48", "4x-80x48", "3:2-80x48"])
def test_mxr_against_reference_kernel_below_and_at_unit_scale(name, scale, signed, capfd):
    """k_polar_mxr has instances for rgba16 targets only (plh_polar_mxr_applies), so its frame cannot be
    seen before quantisation and data beyond [0, 1] is clipped by the store: what can be held to
    k_polar_pp is the kernel's own statement -- never more than one 16-bit code apart, identical on the
    bulk -- at S = 2^-10 (f16 subnormals in the tile: a flush to zero gives code 0 where k_polar_pp has
    up to 75) and S = 1, positive and signed (negative results clip to 0 in both). The bound follows
    from the fp32 one: 4e-6 * max(S, 1) is a quarter of a code."""
    from test_gpu_polar_mfma import assert_codes
    _, (dw, dh), params, kernel, _ = RANGE_GEO[name]
    img = range_source(name, scale, signed)
    pp = _traced(capfd, "k_polar_pp", img, dw, dh, params(), False, src_fmt="rgba16hf", expect_mx=False)
    mx = _traced(capfd, kernel, img, dw, dh, params(), True, src_fmt="rgba16hf", expect_mx=True)
    d = np.abs(mx.astype(np.int64) - pp.astype(np.int64))
    print("%s x %g%s -> rgba16: max %d codes, %.4f of the samples differ; k_polar_pp's largest code %d" %
          (name, scale, " signed" if signed else "", d.max(), (d > 0).mean(), pp[..., :3].max()))
    assert pp[..., :3].max() >= (40 if scale < 1 else 65535)
    assert_codes(mx, pp)


def monotone(h):
    """f16 codes -> integers in the order of the values (sign-magnitude -> monotone; -0 and +0 coincide)"""
    c = np.ascontiguousarray(h).view(np.uint16).astype(np.int64)
    return np.where(c & 0x8000, -(c & 0x7fff), c)


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("scale", SCALES, ids=["2^-10", "1", "2^5", "2^14"])
@pytest.mark.parametrize("name", ["2x-96x64", "2x-130x77", "2:1-128x64", "2:1-200x90"])
def test_matrix_pipe_half_float_targets_over_the_f16_range(name, scale, signed, capfd):
    """k_polar_mxd, and k_polar_mx into an rgba16hf target. Positive data: the existing statement at every
    S -- at most one f16 ulp from k_polar_pp, fewer than 2 % of the samples differing. Signed data: each
    sample within one f16 ulp of k_polar_pp's or within 4e-6 * max(S, 1) of it, whichever is larger.
    (The 2x frames are held to the second form for positive data as well, with the 2 % on top: their
    noise spans [0, 1), the filter rings, and results come out next to zero -- where an f16 ulp is far
    below the contraction's absolute error and tests/util.py: assert_polar_equal already states the
    bound as "one ulp, or 4e-6 of the data's scale". k_polar_mxd's data, 0.05 + 0.9 x, stays clear of
    zero and keeps the plain ulp form.)"""
    pp = pp_frame(capfd, name, scale, signed, "rgba16hf")
    mx = mx_frame(capfd, name, scale, signed, "rgba16hf")
    # 2^14 is the largest of the scales: the reference kernel's frame is still finite
    assert np.isfinite(pp[..., :3].astype(np.float32)).all()
    assert np.array_equal(mx[..., 3], pp[..., 3])
    ulps = np.abs(monotone(mx[..., :3]) - monotone(pp[..., :3]))
    err = np.abs(mx[..., :3].astype(np.float64) - pp[..., :3].astype(np.float64))
    print("%s x %g%s -> rgba16hf: max %d f16 ulp, %.4f of the samples differ, max |mx - pp| = %.3e" %
          (name, scale, " signed" if signed else "", ulps.max(), (ulps > 0).mean(), err.max()))
    assert np.abs(pp[..., :3].astype(np.float32)).max() > 0.5 * scale
    if (ulps > 1).any():
        print("  samples more than one ulp apart: %d, max |mx - pp| among them %.3e (4e-6 * max(S, 1) = %.3e)" %
              ((ulps > 1).sum(), err[ulps > 1].max(), 4e-6 * max(scale, 1.0)))
    if signed or name.startswith("2x"):
        ok = (ulps <= 1) | (err <= 4e-6 * max(scale, 1.0))
        assert ok.all(), (int(ulps[~ok].max()), float(err[~ok].max()), int((~ok).sum()))
    if not signed:
        assert (ulps > 0).mean() < 0.02, float((ulps > 0).mean())
        if not name.startswith("2x"):
            assert ulps.max() <= 1, int(ulps.max())


# ---- 3. per-pixel fast paths with bad lanes: the HDR chain ---------------------------------------------
def pq_f16_frame(w, h):
    """the rgba16hf frame of test_gpu_kernel_variants.py::test_pq_segments_against_closed_forms: PQ code
    values, the left half scaled up to 1.6 (beyond the tables of pqseg.hiph)"""
    from test_gpu_fullsize import hdr_frame16
    f16 = hdr_frame16(w, h).astype(np.float32) / 65535.0
    f16[:, : w // 2, :3] *= 1.6 / max(float(f16[..., :3].max()), 1e-3)
    return f16.astype(np.float16)


def render_hdr(g, capfd, img, dw, dh, params, segments, dst_fmt="rgba16"):
    h, w = img.shape[:2]
    with util.kernel_trace(capfd, PL_HIP_PQ_SEGMENTS=segments, PL_HIP_POLAR_MFMA="1") as kernels:
        src = g.tex_create(w, h, "rgba16hf", img)
        dst = g.tex_create(dw, dh, dst_fmt)
        rr = pl.Renderer(g)
        util.srand(1)
        assert rr.render(pl.frame(src, components=3, color=pl.color_space("bt2020", "pq", max_luma=1000.0)),
                         pl.frame(dst, color=pl.color_space("bt709", "bt1886")), params), g.messages[-4:]
        assert rr.errors() == 0
        out = dst.download()
        rr.destroy(); src.destroy(); dst.destroy()
    return out, kernels


def within_chain_bound(what, x, y, keep):
    """test_pq_segments_against_closed_forms' bound on its out-of-range frame, on the compared pixels"""
    d = np.abs(x[keep][..., :3].astype(np.int64) - y[keep][..., :3].astype(np.int64))
    print("  %s: max %d codes, %.5f of the samples more than one code apart" % (what, d.max(), (d > 1).mean()))
    assert d.max() <= 24 and (d > 1).mean() < 0.005, (what, int(d.max()), float((d > 1).mean()))


@pytest.mark.parametrize("launch", ["ewa_2x_map", "map_pass"])
@pytest.mark.parametrize("size", [(97, 61), (256, 130)])
def test_hdr_chain_with_bad_lanes(g, size, launch, capfd):
    """The HDR10 -> SDR map chain on that frame with the six bad texels added, behind the EWA 2x upscale
    on the matrix pipe (the metric's launch) and as a 1 : 1 pass (k_pass_chain). A wave that holds a bad
    lane legitimately takes the closed forms of the PQ pair, so outside the bad texels' zones frame B lies
    within the bound of the two forms of frame A -- and PL_HIP_PQ_SEGMENTS=0 and =1 agree on B to the same
    bound. (Frame A against B without peak detection: the measurement is a property of the whole frame,
    and six texels out of range move it. The two switches are compared with it as well.) The data-
    dependent gathers behind these texels clamp their positions NaN-safely: pqseg.hiph (v_med3_f32 /
    fmaxf in front of the piece index), cmfast.hiph (v_med3_f32 in front of the tone table's and the gamut
    LUT's), k_peak.hip (the integer bin)."""
    from test_float_domain_ref import polar_radius
    w, h = size
    up = 2 if launch == "ewa_2x_map" else 1
    kw = dict(upscaler=pl.filter_config("ewa_lanczos")) if up == 2 else {}
    no_peak = pl.render_params("default", peak_detect_params=None, dither_params=None, **kw)
    peak = pl.render_params("default", peak_detect_params=pl.peak_detect_params(percentile=99.995),
                            dither_params=None, **kw)
    a = pq_f16_frame(w, h)
    geo = dict(rect=(0, 0, w, h), dw=up * w, dh=up * h, bad=bad_positions(w, h),
               zone=("disc", polar_radius() + 1) if up == 2 else ("rect", 0.75, 0.75))
    b = poison(a, geo["bad"])
    keep = compared(geo)
    assert keep.mean() >= MIN_SHARE
    # (a 1 : 1 pass is k_pass_chain's where it covers its source exactly -- fp32(1 / 97) * 97 is not 1, as in
    # tests/test_gpu_peak_shapes.py: there the op interpreter takes it, and is held to the same statement)
    from test_gpu_peak_shapes import covers_exactly
    want = "k_polar_mx" if up == 2 else "k_pass_chain" if covers_exactly(w) and covers_exactly(h) else "k_pass_generic"
    outs = {}
    for key, img, params, seg in (("A", a, no_peak, "1"), ("B", b, no_peak, "1"), ("B closed", b, no_peak, "0"),
                                  ("B peak", b, peak, "1"), ("B peak closed", b, peak, "0")):
        outs[key], kernels = render_hdr(g, capfd, img, geo["dw"], geo["dh"], params, seg)
        assert want in kernels, (key, kernels)
    print("%s %dx%d: %.1f %% compared" % (launch, w, h, 100 * keep.mean()))
    assert outs["A"][..., :3].std() > 1000
    within_chain_bound("B against A", outs["B"], outs["A"], keep)
    within_chain_bound("B, closed forms against pieces", outs["B closed"], outs["B"], keep)
    within_chain_bound("B with peak detection, closed forms against pieces", outs["B peak closed"], outs["B peak"], keep)
    # the bad pixels themselves are unspecified (pqseg.hiph); what they come out as, for the log
    for key in ("B", "B closed"):
        print("  %s: the bad pixels' own outputs %s" %
              (key, [outs[key][up * y, up * x, :3].tolist() for x, y in geo["bad"]]))


# ---- 3. per-pixel fast paths with bad lanes: the measuring pass ---------------------------------------
@pytest.mark.parametrize("setting", ["hist_cut", "nohist_nocut"])
@pytest.mark.parametrize("size", [(16, 16), (99, 59), (160, 90)])
def test_measuring_pass_with_bad_texels(g, size, setting, capfd):
    """tests/test_gpu_peak_shapes.py's statement (a) on its f16 source with the six bad texels added: the
    measuring kernel of the launcher's choice (k_peak_tiles / k_peak_fast) and the op interpreter
    (k_pass_peak, PL_HIP_PEAK_FAST=0) agree word for word on the 816 words of the measurement and bit for
    bit on the intermediate (NaN matching NaN). (The histogram bin of a NaN or Inf luma: both kernels clamp the integer bin
    to 0 .. 63 after the conversion, k_peak.hip: peak_measure and k_peak_tiles.)"""
    from test_gpu_peak_shapes import measure_env, source_image
    w, h = size
    seam = (min(63, w - 2), min(31, h - 2)) if w > 16 else (7, 7)
    img = poison(source_image("f16", w, h), bad_positions(w, h, seam=seam))
    capfd.readouterr()
    buf_t, out_t = measure_env(g, "f16", img, setting, {"PL_HIP_PASS_TRACE": "1"})
    kernels = [l.split()[-1] for l in capfd.readouterr().err.splitlines() if l.startswith("[plh] kernel k_p")]
    assert any(k in ("k_peak_tiles", "k_peak_fast") for k in kernels), kernels
    buf_g, out_g = measure_env(g, "f16", img, setting, {"PL_HIP_PEAK_FAST": "0", "PL_HIP_PASS_TRACE": "1"})
    kernels = [l.split()[-1] for l in capfd.readouterr().err.splitlines() if l.startswith("[plh] kernel k_p")]
    assert "k_pass_peak" in kernels and "k_peak_tiles" not in kernels and "k_peak_fast" not in kernels, kernels
    diff = out_t != out_g
    nan_t, nan_g = ((o & 0x7fff) > 0x7c00 for o in (out_t, out_g))
    print("measuring pass %dx%d %s: %d of 816 words differ, %d samples of the intermediate differ: %s against %s"
          % (w, h, setting, (buf_t != buf_g).sum(), diff.sum(), [hex(v) for v in out_t[diff][:6]],
             [hex(v) for v in out_g[diff][:6]]))
    assert buf_g[0:12].sum() == (-(-w // 16)) * (-(-h // 16))
    assert np.array_equal(buf_t, buf_g), np.nonzero(buf_t != buf_g)
    # (the signalling NaN leaves the interpreter quieted -- its texels pass through fp32 -- and the
    # measuring kernels, which move the codes, as it is: a NaN of either kind matches a NaN)
    assert not (diff & ~(nan_t & nan_g)).any(), util.diff_stats(out_t, out_g)
