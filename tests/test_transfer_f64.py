"""The float64 truth of the transfer stages (tests/transfer_f64.py), pinned without a GPU, and the
yardstick the GPU sweep (tests/test_gpu_transfer_sweep.py) is held to.

* self-consistency: delinearize(linearize(v)) == v to 1e-12 on every 16-bit code, for every curve
  at three black levels -- a constant mistyped in one direction only cannot survive it;
* the oracle (oracle/pl_oracle.c: the reference's formulas in fp32 on libm) against the truth on the
  sweep's full input set: its maximum error per curve and direction is printed -- E_orc, which the
  GPU tests recompute the same way at run time;
* the float32 emulation of the device's primitives (exp2(y * log2 x) and kin) on the same inputs:
  its ratio to max(E_orc, E_ulp) sets K (transfer_f64.K), and it passes the very statement the GPU
  is held to -- so the statement is one an honest fp32 evaluation can meet.

Errors are in 16-bit codes of the output (delinearize, sigmoidize) or in local codes (linearize,
unsigmoidize): |error| over the change of the true curve per 16-bit input code.

Measured here (maxima over the three black levels; "well": the well-conditioned samples, which
leaves out the few next to black on which ONE fp32 rounding of a black-scaled power law is worth
more than a twentieth of a code):

    curve      linearize E_orc (well)   delinearize E_orc (well)   emulation / oracle, worst
    sRGB       0.0092                   0.0092                     1.11
    BT.1886    0.0054                   0.0076                     1.48
    gamma 2.2  0.90   (0.0044)          2.1    (0.018)             1.76
    gamma 2.8  8.2    (0.0046)          19     (0.021)             1.83
    ST 428     4.6    (0.0047)          10     (0.020)             2.19
    ProPhoto   0.0045                   0.058 (its 16x / pow step) 2.03
    PQ         0.51                     0.83                       1.07
    HLG        0.013                    0.014                      1.03
    V-Log      0.0023                   0.0059                     1.68
    S-Log1/2   0.0042                   0.0049                     1.58
    scRGB      0.019 (= half an ulp)    0.016                      0.99
    sigmoid    0.0048 (inverse)         0.0086                     1.9
"""
import ctypes as C
import math

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import transfer_f64 as t64
from libplacebo_amd import _capi as capi

CURVES = [k for k in pl.TRC if k != "linear"]


_LIB = None


def _lib():
    """A handle of its own on the library: other test modules rebind the prototypes of the shared one
    (tests/ref_structs.py), and these helpers must not depend on which of them ran before."""
    global _LIB
    if _LIB is None:
        pl.lib()
        _LIB = C.CDLL(capi.LIB_PATH)
        _LIB.pl_raw_primaries_get.restype = C.c_void_p
        _LIB.pl_raw_primaries_get.argtypes = [C.c_int]
        _LIB.pl_get_rgb2xyz_matrix.restype = capi.Matrix3x3
        _LIB.pl_get_rgb2xyz_matrix.argtypes = [C.c_void_p]
        _LIB.pl_color_space_nominal_luma_ex.restype = None
        _LIB.pl_color_space_nominal_luma_ex.argtypes = [C.c_void_p]
    return _LIB


def nominal(csp):
    """(csp_min, csp_max) as pl_shader_linearize derives them (colorspace.c:597-604)"""
    mn, mx = C.c_float(), C.c_float()

    class NLP(C.Structure):
        _fields_ = [("color", C.POINTER(capi.ColorSpace)), ("metadata", C.c_int),
                    ("scaling", C.c_int), ("out_min", C.POINTER(C.c_float)),
                    ("out_max", C.POINTER(C.c_float)), ("out_avg", C.POINTER(C.c_float))]
    p = NLP(color=C.pointer(csp), metadata=2, scaling=0, out_min=C.pointer(mn),
            out_max=C.pointer(mx))
    _lib().pl_color_space_nominal_luma_ex(C.byref(p))
    return mn.value, mx.value


def luma_coeffs(primaries):
    m = _lib().pl_get_rgb2xyz_matrix(_lib().pl_raw_primaries_get(int(primaries)))
    return [m.m[1][0], m.m[1][1], m.m[1][2]]


def color_space(trc, black):
    return pl.color_space("bt2020" if trc in ("pq", "hlg") else "bt709", trc, **t64.BLACKS[black])


def transfer_case(trc, direction, black):
    csp = color_space(trc, black)
    mn, mx = nominal(csp)
    return t64.Case(direction, trc, mn, mx, luma_coeffs(csp.primaries)), csp


SIGMOIDS = {"default": (0.75, 6.5), "steep": (0.6, 11.0)}


def sigmoid_case(inverse, which):
    c, s = SIGMOIDS[which]
    return t64.Case("unsigmoidize" if inverse else "sigmoidize", center=c, slope=s)


def rgba(img):
    src = np.ones(img.shape[:2] + (4,), np.float32)
    src[..., :3] = img
    return src


def oracle(case, img):
    if case.kind in ("linearize", "delinearize"):
        return getattr(orc, case.kind)(rgba(img), pl.TRC[case.trc], case.mn, case.mx, case.luma)
    return orc.sigmoid(rgba(img), case.center, case.slope, inverse=case.kind == "unsigmoidize")


def oracle_report(case):
    return case.measure([oracle(case, img) for _, img in case.images()])


def emulation_report(case):
    return case.measure([case.fn(img, be=t64.Emu32) for _, img in case.images()])


def ratio(rep, orc_rep):
    """an implementation's error over the oracle's yardstick, on all samples and on the
    well-conditioned ones: the larger of the two"""
    return max(rep.E / max(orc_rep.E, orc_rep.E_ulp),
               rep.E_well / max(orc_rep.E_well, orc_rep.E_ulp_well))


@pytest.mark.parametrize("trc", CURVES + ["linear"])
def test_truth_round_trip_on_every_code(trc):
    """delinearize(linearize(v)) == v to 1e-12 on every code, with the constants as written and in
    extended precision (transfer_f64.exact_constants: with the rounded constants the shader receives
    the reference's two directions are not inverses). Left out, because the reference's own curve
    is not invertible there: codes whose linear value is negative and is clamped on the way back
    (below V-Log's 0.125, S-Log1's 0.0903, S-Log2's 0.030001), and HLG codes so dark that the inverse
    OOTF's max(1e-6, luma) cuts in."""  # noqa: D301
    v = t64.codes().astype(np.longdouble)
    rgb = np.stack([v, v, v] if t64.is_grey(trc) else [v, v[::-1], np.roll(v, 4099)], -1)
    csp = color_space(trc, "default")
    luma = luma_coeffs(csp.primaries)
    levels = [nominal(color_space(trc, b)) for b in t64.BLACKS]
    levels.append((0.0, levels[-1][1]))         # min_luma = 0 exactly, max_luma scaled
    for mn, mx in levels:
        with t64.exact_constants():
            lin = t64.linearize(rgb, trc, mn, mx, luma, be=t64.F80)
            back = t64.delinearize(lin, trc, mn, mx, luma, be=t64.F80)
        keep = np.ones(rgb.shape, bool)
        if trc in ("vlog", "slog1", "slog2"):
            keep = lin >= 0
            with t64.exact_constants():
                at0 = t64.delinearize(np.zeros(3), trc, mn, mx, luma, be=t64.F80)[0]
            assert np.all(back[~keep] == at0)
        if trc == "hlg":
            keep = (lin / mx) @ np.asarray(luma, np.longdouble) >= 1e-6
            keep = np.stack([keep] * 3, -1)
        assert keep.mean() >= 0.87, (trc, keep.mean())
        err = np.where(keep, np.abs(back - rgb), 0)
        # (the darkest codes of a black-lifted power law: min + (max - min) * v^2.8 is so flat there
        # that the doubles the constants are held in cannot resolve v to 1e-12. There, and only below
        # code 32,
        # the statement is that the value recovered has the same linear image to 2^-50: the constants
        # are doubles)
        bad = err > 1e-12
        if bad.any():
            assert rgb[bad].max() < 32 / 65535, (trc, mn, mx, float(err.max()), float(rgb[bad].max()))
            with t64.exact_constants():
                again = t64.linearize(back, trc, mn, mx, luma, be=t64.F80)
            assert np.all(np.abs(again - lin)[bad] <= 2.0 ** -50 * np.abs(lin[bad]))


def test_truth_sigmoid_round_trip():
    v = t64.codes().astype(np.longdouble)
    for c, s in SIGMOIDS.values():
        with t64.exact_constants():
            back = t64.unsigmoidize(t64.sigmoidize(v, c, s, be=t64.F80), c, s, be=t64.F80)
            ends = t64.sigmoidize(np.array([0.0, 1.0]), c, s, be=t64.F80)
        assert np.abs(back - v).max() <= 1e-12
        assert np.abs(ends - [0, 1]).max() <= 1e-12     # through (0, 0) and (1, 1)


def cases_of(group):
    if group == "sigmoid":
        for inverse in (False, True):
            for which in SIGMOIDS:
                yield "%s %s" % ("unsigmoidize" if inverse else "sigmoidize", which), \
                    sigmoid_case(inverse, which)
        return
    for direction in ("linearize", "delinearize"):
        for black in t64.BLACKS:
            yield "%s %s %s" % (group, direction, black), transfer_case(group, direction, black)[0]


_RATIOS = {}


def yardstick(group, show=None):
    """E_orc, E_ulp and the emulation's figures for every case of one curve (or the sigmoid);
    returns the largest emulation / oracle ratio among them"""
    if group in _RATIOS:
        return _RATIOS[group]
    worst = 0.0
    for name, case in cases_of(group):
        o, e = oracle_report(case), emulation_report(case)
        r = ratio(e, o)
        worst = max(worst, r)
        if show:
            show("%-28s E_orc %9.4g (well %8.4g)  E_ulp %9.4g (well %8.4g)  emulation %9.4g "
                 "(well %8.4g)  ratio %.2f" % (name, o.E, o.E_well, o.E_ulp, o.E_ulp_well,
                                               e.E, e.E_well, r))
        if group != "pq":
            # the emulation meets the statement the GPU is held to (PQ apart: the device evaluates
            # it in a well-conditioned form of its own, pqmath.hiph, the emulation and the oracle in
            # the reference's) ...
            t64.check(case, e, o, what="emulation: " + name)
            # ... and the oracle is never half a code off on a well-conditioned sample
            assert o.E_well <= 0.5, (name, o.E_well)
    _RATIOS[group] = worst
    return worst


@pytest.mark.parametrize("group", CURVES + ["sigmoid"])
def test_oracle_and_emulation_against_truth(capsys, group):
    """E_orc per curve, direction and black level, and the emulation's ratio to it (printed)."""
    lines = []
    yardstick(group, lines.append)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_k_is_twice_the_emulations_ratio(capsys):
    worst = max(yardstick(g) for g in CURVES + ["sigmoid"])
    with capsys.disabled():
        print("\nlargest emulation / oracle ratio %.2f -> K = %d" % (worst, math.ceil(2 * worst)))
    assert math.ceil(2 * worst) == t64.K, worst


# the curves the renderer tests cover (tests/test_gpu_transfer_render.py)
RENDER_CURVES = ["srgb", "bt1886", "gamma22", "gamma28", "st428", "prophoto", "hlg", "pq"]


@pytest.mark.parametrize("trc", RENDER_CURVES)
def test_oracle_alone_stores_the_right_code(trc):
    """The statement the renderer test makes of a 16-bit target -- the stored code is
    round(truth * 65535), either neighbour where the truth is within the bound of a rounding
    boundary -- holds for the oracle on every sample of the sweep."""
    case, _ = transfer_case(trc, "delinearize", "default")
    name, img = case.images()[0]
    ref = oracle(case, img)
    rep = t64.Report([case.measure_image(img, ref)])
    stored = orc.tex_encode(ref, "rgba16")[..., :3]
    ex = t64.excess_stored(stored, rep, rep)
    assert ex.max() <= 0, (trc, float(ex.max()), int((ex > 0).sum()))


# ---- the statement catches the mistakes it is there for (a broken emulation in place of the GPU) --
def _emulate(case, fn=None):
    fn = fn or (lambda img: case.fn(img, be=t64.Emu32))
    return case.measure([fn(img) for _, img in case.images()])


def test_statement_catches_a_knee_taken_on_the_wrong_side():
    """`<` for `<=` at V-Log's knee moves one sample, the knee itself, onto the other piece: 0.02
    local code, twice the bound. (The same slip at the sRGB knee cannot be seen by ANY fp32 statement: the two sRGB
    pieces meet at 0.04045 to 2e-9, 0.0017 local code, a quarter of the oracle's own error there.
    ProPhoto's meet exactly.)"""
    case, _ = transfer_case("vlog", "linearize", "default")
    knee = np.float32(0.181)

    def flipped(img):
        out = case.fn(img, be=t64.Emu32)
        other = case.fn(img, be=t64.Emu32, branch=False)
        return np.where(img == knee, other, out)
    o = oracle_report(case)
    t64.check(case, _emulate(case), o)
    with pytest.raises(AssertionError):
        t64.check(case, _emulate(case, flipped), o)
    srgb, _ = transfer_case("srgb", "linearize", "default")
    x = np.full((1, 3), np.float32(0.04045), np.float64)
    gap = abs(srgb.fn(x, branch=True) - srgb.fn(x, branch=False))[0, 0] / t64.local_slope(srgb.fn, x)[0, 0]
    assert gap < 0.002


def test_statement_catches_a_truncated_exponent():
    """0.4166 for 1 / 2.4 in the sRGB OETF: 0.7 code at the dark end of the power segment"""
    case, _ = transfer_case("srgb", "delinearize", "default")

    class Trunc(t64.Emu32):
        @staticmethod
        def pow(x, y):
            return t64.Emu32.pow(x, 0.4166 if abs(y - 1 / 2.4) < 1e-6 else y)
    o = oracle_report(case)
    with pytest.raises(AssertionError):
        t64.check(case, _emulate(case, lambda img: case.fn(img, be=Trunc)), o)


def test_statement_catches_a_dropped_black_scaling():
    """delinearize without its black-scaling step (PLH_TRC_RESCALE): the stored codes move"""
    case, _ = transfer_case("srgb", "delinearize", "default")
    name, img = case.images()[0]
    bare = t64.Case("delinearize", "srgb", 0.0, 1.0, case.luma)
    ref = oracle(case, img)
    o = t64.Report([case.measure_image(img, ref)])
    got = bare.fn(img, be=t64.Emu32)
    stored = orc.tex_encode(rgba(got.astype(np.float32)), "rgba16")[..., :3]
    g = t64.Report([case.measure_image(img, got)])
    assert t64.excess_stored(stored, g, o).max() > 0
    with pytest.raises(AssertionError):
        t64.check(case, g, o)


def test_statement_catches_swapped_luma_coefficients():
    """HLG's OOTF with two luma coefficients exchanged: invisible on grey, caught by the colours"""
    case, _ = transfer_case("hlg", "linearize", "default")
    swapped = t64.Case("linearize", "hlg", case.mn, case.mx, [case.luma[1], case.luma[0], case.luma[2]])
    o = oracle_report(case)
    t64.check(case, _emulate(case, lambda img: swapped.fn(img, be=t64.Emu32)), o)    # grey: blind
    (name, img), = t64.colour_images(case)
    t64.check_colours(case, case.fn(img, be=t64.Emu32), oracle(case, img), img)
    with pytest.raises(AssertionError, match="colours"):
        t64.check_colours(case, swapped.fn(img, be=t64.Emu32), oracle(case, img), img)
