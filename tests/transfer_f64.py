"""float64 truth for the transfer stages: pl_shader_linearize / pl_shader_delinearize
(reference src/shaders/colorspace.c:589-720, :722-847) and pl_shader_sigmoidize /
pl_shader_unsigmoidize (:851-894), restated in numpy for all 18 pl_color_transfer values.

Every constant is taken as the fp32 value the shader receives -- SH_FLOAT embeds a float, "%f" prints
six decimals, a GLSL constant expression such as 1.0/2.4 folds to one float -- and host-side
constants that the reference derives with powf / expf / log2f / sqrtf (BT.1886's a and b, HLG's
system gamma and black lift, the sigmoid's offset and scale) are derived with the C library's own
float functions. The ARITHMETIC on the samples is float64. So what is measured against this truth
is the rounding of an implementation's evaluation, not the rounding of 0.055.

The curves are written once over a small "backend" (dtype + pow / exp / exp10 / log): `F64` is the
truth; `Emu32` is the yardstick for fp32 evaluations on native units, numpy float32 with
pow(x, y) = exp2(y * log2 x), exp10(x) = exp2(x * log2 10), log(x) = log2(x) * ln 2.

Also here, because the CPU tests and the GPU sweep share them: the input sets (every 16-bit code,
the knees with their fp32 neighbours, the out-of-range runs), the error units ("local codes") and
the statement held per case (`check`).

Test infrastructure only.
"""
import ctypes as C

import numpy as np

import colormap_f64 as c64

TRC = dict(unknown=0, bt1886=1, srgb=2, linear=3, gamma18=4, gamma20=5, gamma22=6, gamma24=7,
           gamma26=8, gamma28=9, prophoto=10, st428=11, pq=12, hlg=13, vlog=14, slog1=15,
           slog2=16, scrgb=17)
NAME = {v: k for k, v in TRC.items()}
GAMMA = {0: 2.2, 4: 1.8, 5: 2.0, 6: 2.2, 7: 2.4, 8: 2.6, 9: 2.8}
# pl_color_space_is_black_scaled
NOT_BLACK_SCALED = {TRC["bt1886"], TRC["pq"], TRC["scrgb"], TRC["vlog"], TRC["slog1"], TRC["slog2"]}
BT709_LUMA = (0.2126390039920807, 0.7151686549186707, 0.0721923187375069)

f32 = np.float32
_libm = C.CDLL("libm.so.6")
for _n in ("powf", "expf", "log2f", "sqrtf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float] * (2 if _n == "powf" else 1)


_EXACT = False


class exact_constants:
    """with exact_constants(): every constant is taken as written, unrounded (no fp32, no "%f"), and
    the host-side ones are derived in double. The two directions of a curve are then inverses of each
    other to the last bits, which the self-consistency test needs; with the constants the shader
    receives they are not (1 / (max - min) and max - min are rounded separately, VLOG_C / ln 10 is
    printed to six decimals)."""

    def __enter__(self):
        global _EXACT
        _EXACT = True

    def __exit__(self, *exc):
        global _EXACT
        _EXACT = False


def F(x):
    """the fp32 value of x, as a Python float"""
    return float(x) if _EXACT else float(f32(x))


def pf(x):
    """a float printed with "%f" and read back by the GLSL compiler"""
    return float(x) if _EXACT else F("%f" % F(x))


def rcp(x):
    """1.0 / x folded to one float"""
    return 1.0 / x if _EXACT else float(f32(1.0) / f32(x))


def fdiv(a, b):
    """a / b between floats"""
    return a / b if _EXACT else float(f32(a) / f32(b))


def fsub(a, b):
    return a - b if _EXACT else float(f32(a) - f32(b))


def powf(x, y):
    return float(x) ** float(y) if _EXACT else float(_libm.powf(F(x), F(y)))


# the reference's macros (src/shaders/colorspace.c's includes), as written
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
VLOG_B, VLOG_C, VLOG_D = 0.00873, 0.241514, 0.598206
SLOG_A, SLOG_B, SLOG_C = 0.432699, 0.037584, 0.616596 + 0.03
SLOG_P, SLOG_Q, SLOG_K2 = 3.538813, 0.030001, 155.0 / 219.0
LN10 = 2.302585092994046


def pq_k():
    return pf(fdiv(10000.0, 203.0))


def bt1886_ab(csp_min, csp_max):
    lb, lw = powf(csp_min, rcp(2.4)), powf(csp_max, rcp(2.4))
    d = fsub(lw, lb)
    return powf(d, 2.4), fdiv(lb, d)


def hlg_yb(csp_min, csp_max):
    if _EXACT:
        y = 1.2 * 1.111 ** np.log2(csp_max / (1000.0 / 203.0))
        return float(y), float(np.sqrt(3 * (csp_min / csp_max) ** (1 / y)))
    ref = f32(1000.0) / f32(203.0)
    y = f32(1.2) * f32(_libm.powf(F(1.111), _libm.log2f(F(f32(csp_max) / ref))))
    b = _libm.sqrtf(F(f32(3) * f32(_libm.powf(F(f32(csp_min) / f32(csp_max)), F(f32(1) / y)))))
    return float(y), float(b)


class F64:
    dt = np.float64
    pow = staticmethod(np.power)
    exp = staticmethod(np.exp)
    log = staticmethod(np.log)
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def exp10(x):
        return np.power(10.0, x)

    @staticmethod
    def pq_eotf(v):
        return c64.pq_eotf(v)

    @staticmethod
    def pq_oetf(x):
        return c64.pq_oetf(x)


class F80(F64):
    """x87 extended precision: the self-consistency test's (float64 cannot hold a black-lifted
    power law's round trip to 1e-12 next to black)"""
    dt = np.longdouble

    @staticmethod
    def exp10(x):
        return np.power(np.longdouble(10), x)


class Emu32:
    """fp32 on native base-2 units, as transfer.hiph states its primitives"""
    dt = np.float32
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def pow(x, y):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.exp2(f32(y) * np.log2(x))

    @staticmethod
    def exp(x):
        return np.exp2(x * f32(1.44269504088896340736))

    @staticmethod
    def exp10(x):
        return np.exp2(x * f32(3.32192809488736234787))

    @staticmethod
    def log(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.log2(x) * f32(0.69314718055994530942)

    @classmethod
    def pq_eotf(cls, v):
        p = cls.pow(np.maximum(v, f32(0)), rcp(c64.M2))
        return cls.pow(np.maximum(p - f32(c64.C1), f32(0)) / (f32(c64.C2) - f32(c64.C3) * p),
                       rcp(c64.M1))

    @classmethod
    def pq_oetf(cls, x):
        y = cls.pow(np.maximum(x, f32(0)), F(c64.M1))
        return cls.pow((f32(c64.C1) + f32(c64.C2) * y) / (f32(1) + f32(c64.C3) * y), F(c64.M2))


def _where(cond, a, b):
    return np.where(cond, a, b)


def linearize(rgb, trc, csp_min, csp_max, luma=BT709_LUMA, be=F64, branch=None):
    """pl_shader_linearize over rgb (..., 3). branch: force the upper (True) / lower (False) piece
    of a piecewise curve, whatever the comparison says (the knee tests' "other branch")."""
    trc = TRC.get(trc, trc)
    dt = be.dt
    k = lambda x: dt(x)     # noqa: E731  (a constant in the backend's type)
    v = np.asarray(rgb, dt)
    if trc == TRC["linear"]:
        return v.copy()
    if trc != TRC["scrgb"]:
        v = np.maximum(v, k(0))                                                  # :613
    pick = (lambda c: c) if branch is None else (lambda c: np.full(c.shape, branch))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if trc == TRC["srgb"]:                                                   # :617-620
            v = _where(pick(k(F(0.04045)) < v),
                       be.pow((v + k(F(0.055))) / k(F(1.055)), F(2.4)), v * k(rcp(12.92)))
        elif trc == TRC["bt1886"]:                                               # :622-629
            a, b = bt1886_ab(csp_min, csp_max)
            return k(a) * be.pow(v + k(b), F(2.4))
        elif trc in GAMMA:                                                       # :631-649
            v = be.pow(v, F(GAMMA[trc]))
        elif trc == TRC["prophoto"]:                                             # :650-653
            v = _where(pick(k(0.03125) < v), be.pow(v, F(1.8)), v * k(0.0625))
        elif trc == TRC["st428"]:                                                # :655-656
            v = k(fdiv(52.37, 48.0)) * be.pow(v, F(2.6))
        elif trc == TRC["pq"]:                                                   # :658-667
            return be.pq_eotf(v) * k(pq_k())
        elif trc == TRC["hlg"]:                                                  # :668-683
            y, b = hlg_yb(csp_min, csp_max)
            v = k(fsub(1.0, b)) * v + k(b)
            v = _where(pick(k(0.5) < v), be.exp((v - k(pf(HLG_C))) * k(rcp(pf(HLG_A)))) + k(pf(HLG_B)),
                       k(4) * v * v)
            v = v * k(rcp(12.0))
            l = k(F(luma[0])) * v[..., 0] + k(F(luma[1])) * v[..., 1] + k(F(luma[2])) * v[..., 2]
            g = k(F(csp_max)) * be.pow(np.maximum(l, k(0)), fsub(y, 1.0))
            return v * g[..., None]
        elif trc == TRC["vlog"]:                                                 # :685-691
            return _where(pick(k(F(0.181)) <= v),
                          be.exp10((v - k(pf(VLOG_D))) * k(rcp(pf(VLOG_C)))) - k(pf(VLOG_B)),
                          (v - k(0.125)) * k(rcp(5.6)))
        elif trc == TRC["slog1"]:                                                # :692-696
            return be.exp10((v - k(pf(SLOG_C))) * k(rcp(pf(SLOG_A)))) - k(pf(SLOG_B))
        elif trc == TRC["slog2"]:                                                # :697-703
            return _where(pick(k(pf(SLOG_Q)) <= v),
                          (be.exp10((v - k(pf(SLOG_C))) * k(rcp(pf(SLOG_A)))) - k(pf(SLOG_B)))
                          * k(rcp(pf(SLOG_K2))),
                          (v - k(pf(SLOG_Q))) * k(rcp(pf(SLOG_P))))
        elif trc == TRC["scrgb"]:                                                # :704-707
            return v * k(pf(fdiv(80.0, 203.0)))
        else:
            raise ValueError(trc)
    if csp_max != 1 or csp_min != 0:                                             # :715-719
        v = k(fsub(csp_max, csp_min)) * v + k(F(csp_min))
    return v


def black_scale_in(trc, csp_min, csp_max):
    """(m, c) of delinearize's black scaling v = m * x + c as floats, or None (:740-747)"""
    trc = TRC.get(trc, trc)
    if trc in NOT_BLACK_SCALED or trc in (TRC["hlg"], TRC["linear"]) or \
            (csp_max == 1 and csp_min == 0):
        return None
    d = fsub(csp_max, csp_min)
    return fdiv(1.0, d), fdiv(-csp_min, d)


def delinearize(rgb, trc, csp_min, csp_max, luma=BT709_LUMA, be=F64, branch=None, dv=0.0):
    """pl_shader_delinearize over rgb (..., 3). dv: a perturbation added behind the black scaling
    (conditioning: what one rounding of that step does to the result)."""
    trc = TRC.get(trc, trc)
    dt = be.dt
    k = lambda x: dt(x)     # noqa: E731
    v = np.asarray(rgb, dt)
    if trc == TRC["linear"]:
        return v.copy()
    mc = black_scale_in(trc, csp_min, csp_max)
    if mc:
        v = k(mc[0]) * v + k(mc[1]) + dv                                         # :740-747
    if trc != TRC["scrgb"]:
        v = np.maximum(v, k(0))                                                  # :749-750
    pick = (lambda c: c) if branch is None else (lambda c: np.full(c.shape, branch))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if trc == TRC["srgb"]:                                                   # :753-758
            return _where(pick(k(F(0.0031308)) <= v),
                          k(F(1.055)) * be.pow(v, rcp(2.4)) - k(F(0.055)), v * k(F(12.92)))
        if trc == TRC["bt1886"]:                                                 # :759-767
            a, b = bt1886_ab(csp_min, csp_max)
            return be.pow(k(F(1.0 / a)) * v, rcp(2.4)) - k(b)
        if trc in GAMMA:                                                         # :768-786
            return be.pow(v, rcp(GAMMA[trc]))
        if trc == TRC["st428"]:                                                  # :787-789
            return be.pow(v * k(fdiv(48.0, 52.37)), rcp(2.6))
        if trc == TRC["prophoto"]:                                               # :790-794
            return _where(pick(k(F(0.001953)) <= v), be.pow(v, rcp(1.8)), v * k(16))
        if trc == TRC["pq"]:                                                     # :795-802
            return be.pq_oetf(v * k(rcp(pq_k())))
        if trc == TRC["hlg"]:                                                    # :803-818
            y, b = hlg_yb(csp_min, csp_max)
            v = v * k(rcp(csp_max))
            l = k(F(luma[0])) * v[..., 0] + k(F(luma[1])) * v[..., 1] + k(F(luma[2])) * v[..., 2]
            g = k(12) * be.pow(np.maximum(k(F(1e-6)), l), fdiv(fsub(1.0, y), y))
            v = v * g[..., None]
            v = _where(pick(k(1) < v),
                       k(pf(HLG_A)) * be.log(v - k(pf(HLG_B))) + k(pf(HLG_C)),
                       k(0.5) * be.sqrt(v))
            ib = fsub(1.0, b)
            return k(fdiv(1.0, ib)) * v + k(fdiv(-b, ib))
        if trc == TRC["vlog"]:                                                   # :819-825
            return _where(pick(k(F(0.01)) <= v),
                          k(pf(VLOG_C / LN10)) * be.log(v + k(pf(VLOG_B))) + k(pf(VLOG_D)),
                          k(F(5.6)) * v + k(0.125))
        if trc == TRC["slog1"]:                                                  # :826-829
            return k(pf(SLOG_A / LN10)) * be.log(v + k(pf(SLOG_B))) + k(pf(SLOG_C))
        if trc == TRC["slog2"]:                                                  # :830-836
            return _where(pick(k(0) <= v),
                          k(pf(SLOG_A / LN10)) * be.log(k(pf(SLOG_K2)) * v + k(pf(SLOG_B)))
                          + k(pf(SLOG_C)),
                          k(pf(SLOG_P)) * v + k(pf(SLOG_Q)))
        if trc == TRC["scrgb"]:                                                  # :837-840
            return v * k(pf(fdiv(203.0, 80.0)))
    raise ValueError(trc)


def sigmoid_consts(center, slope):
    """offset and scale as floats (colorspace.c:862-863)"""
    if _EXACT:
        offset = 1.0 / (1 + np.exp(slope * center))
        return offset, 1.0 / (1 + np.exp(slope * (center - 1))) - offset
    c, s = f32(center), f32(slope)
    offset = F(1.0 / (1 + float(f32(_libm.expf(F(s * c))))))
    scale = F(1.0 / (1 + float(f32(_libm.expf(F(s * (c - f32(1))))))) - offset)
    return offset, scale


def sigmoidize(rgb, center=0.75, slope=6.5, be=F64):                             # :865-871
    k = lambda x: be.dt(x)  # noqa: E731
    offset, scale = sigmoid_consts(center, slope)
    v = np.clip(np.asarray(rgb, be.dt), k(0), k(1))
    return k(F(center)) - k(F(1.0 / F(slope))) * be.log(k(1) / (v * k(scale) + k(offset)) - k(1))


def unsigmoidize(rgb, center=0.75, slope=6.5, be=F64):                           # :886-893
    k = lambda x: be.dt(x)  # noqa: E731
    offset, scale = sigmoid_consts(center, slope)
    v = np.clip(np.asarray(rgb, be.dt), k(0), k(1))
    return k(F(1.0 / scale)) / (k(1) + be.exp(k(F(slope)) * (k(F(center)) - v))) \
        - k(fdiv(offset, scale))


# ---- knees ------------------------------------------------------------------------------------
def knees(trc, direction, csp_min=0.0, csp_max=1.0):
    """The comparison thresholds of a piecewise curve as (value at the comparison, strict), where
    strict: the upper piece is taken for threshold < v (else threshold <= v). The value is the one
    the COMPARISON sees: behind the clamp, black scaling and (HLG) black lift / OOTF^-1."""
    trc = TRC.get(trc, trc)
    lin = direction == "linearize"
    table = {
        TRC["srgb"]: (F(0.04045), True) if lin else (F(0.0031308), False),
        TRC["prophoto"]: (0.03125, True) if lin else (F(0.001953), False),
        TRC["vlog"]: (F(0.181), False) if lin else (F(0.01), False),
        TRC["slog2"]: (pf(SLOG_Q), False) if lin else (0.0, False),
        TRC["hlg"]: (0.5, True) if lin else (1.0, True),
    }
    return [table[trc]] if trc in table else []


def knee_inputs(trc, direction, csp_min, csp_max):
    """fp32 inputs at every knee. Where the comparison sees the input itself: the threshold's lower
    fp32 neighbour, the threshold, its upper neighbour (np.nextafter). Where an fp32 affine step lies
    in front of the comparison (black scaling, HLG's lift and OOTF^-1) the side of an input within a
    rounding of the threshold depends on how that step is rounded (fused or not), so the pair is the
    nearest inputs either side on which float64 and every fp32 order agree: a few ulps away."""
    trc = TRC.get(trc, trc)
    out = []
    for t, _strict in knees(trc, direction, csp_min, csp_max):
        t32 = f32(t)
        m, c = 1.0, 0.0
        if direction == "linearize":
            if trc == TRC["hlg"]:
                _, b = hlg_yb(csp_min, csp_max)
                m, c = fsub(1.0, b), b
        elif trc == TRC["hlg"]:
            # grey: v = 12 * (x / max)^(1/y); the comparison sees 1.0 at x = max * 12^-y
            y, _ = hlg_yb(csp_min, csp_max)
            x0 = F(csp_max) * 12.0 ** -y
            out.append(tuple(f32(x0 * (1 + d)) for d in (-4e-6, 4e-6)))
            continue
        else:
            m, c = black_scale_in(trc, csp_min, csp_max) or (1.0, 0.0)
        if m == 1.0 and c == 0.0:
            out.append((np.nextafter(t32, f32(-np.inf)), t32, np.nextafter(t32, f32(np.inf))))
            continue
        x0 = f32((float(t32) - c) / m)
        ulp = float(np.spacing(x0)) + float(np.spacing(t32)) / m
        out.append((f32(float(x0) - 3 * ulp), f32(float(x0) + 3 * ulp)))
    return out


# ---- the input sets ---------------------------------------------------------------------------
N = 256
H = 1.0 / 65535.0
# the three black levels: pl_color_space.hdr as given to the library
BLACKS = dict(default={}, raised=dict(min_luma=1.0), scaled=dict(min_luma=1e-6, max_luma=400.0))


def is_grey(trc):
    """HLG's OOTF couples the channels: its sweeps run as grey"""
    return TRC.get(trc, trc) == TRC["hlg"]


def planes(v, grey=False):
    """256 x 256 values -> three planes: as is, reversed, transposed (so a texel's channels differ)"""
    v = np.asarray(v).reshape(N, N)
    return np.stack([v, v, v] if grey else [v, v[::-1, ::-1], v.T], -1)


def codes():
    """every 16-bit code i / 65535 (float64)"""
    return np.arange(65536, dtype=np.float64) / 65535.0


def lin_edge_values(trc, csp_min, csp_max):
    """The second, small set of linearize inputs (fp32, 1-D): each knee with its fp32 neighbours,
    +-0, the smallest values, a run of negatives down to -0.25, values above 1 up to 1.25 (scRGB:
    up to 7.5 and down to -0.5)."""
    trc = TRC.get(trc, trc)
    vals = [0.0, -0.0, 1e-30, 1e-12, 1e-7, 0.25 * H, 0.5 * H,
            1.0, float(np.nextafter(f32(1), f32(0))), float(np.nextafter(f32(1), f32(2)))]
    vals += list(-np.geomspace(1e-8, 0.25, 24))
    vals += list(np.linspace(1.0, 1.25, 17)[1:])
    if trc == TRC["scrgb"]:
        vals += list(np.linspace(1.25, 7.5, 26)[1:]) + list(-np.linspace(0.25, 0.5, 6))
    for tri in knee_inputs(trc, "linearize", csp_min, csp_max):
        vals += [float(x) for x in tri]
    return np.asarray(vals, np.float32)


def delin_edge_values(trc, csp_min, csp_max, luma=BT709_LUMA):
    """The small set of delinearize inputs (fp32, 1-D): the images of lin_edge_values, linear 0 and
    -0, values below black, and each linear-side knee with its neighbours."""
    trc = TRC.get(trc, trc)
    e = lin_edge_values(trc, csp_min, csp_max).astype(np.float64)
    img = linearize(np.stack([e, e, e], -1), trc, csp_min, csp_max, luma)[..., 0]
    vals = [float(x) for x in img.astype(np.float32)] + [0.0, -0.0, 1e-30, F(csp_min)]
    vals += list(F(csp_min) - np.geomspace(1e-8, 0.25, 12))
    for tri in knee_inputs(trc, "delinearize", csp_min, csp_max):
        vals += [float(x) for x in tri]
    return np.asarray(vals, np.float32)


def pad_image(values, grey=False, fill=0.25, w=64):
    """1-D fp32 values -> an (rows x 64 x 3) fp32 image: the values in R, shifted copies in G and B
    (grey: the same in all three), padded with `fill`"""
    n = values.size
    rows = (n + w - 1) // w
    buf = np.full(rows * w, fill, np.float32)
    buf[:n] = values
    ch = [buf, buf, buf] if grey else [buf, np.roll(buf, 7), np.roll(buf, 19)]
    return np.ascontiguousarray(np.stack(ch, -1).reshape(rows, w, 3))


def hlg_colours(seed=5):
    """64 x 64 random saturated colours (HLG's OOTF couples the channels)"""
    rng = np.random.default_rng(seed)
    c = rng.random((64, 64, 3))
    weak = rng.integers(0, 3, (64, 64))
    for ch in range(3):
        c[..., ch] = np.where(weak == ch, c[..., ch] * 0.05, c[..., ch])
    return c.astype(np.float32)


def sigmoid_values():
    """every code, 0 and 1 and their fp32 neighbours inside and outside [0, 1], and a run outside"""
    e = [0.0, -0.0, 1.0]
    e += [float(np.nextafter(f32(a), f32(b))) for a, b in ((0, 1), (0, -1), (1, 0), (1, 2))]
    e += [-1e-30, -1e-3, -0.25, 1.001, 1.25, 0.25 * H, 1 - 0.25 * H]
    return np.asarray(e, np.float32)


def inputs(trc, direction, csp_min, csp_max, luma=BT709_LUMA):
    """The fp32 images of one sweep case: [(name, rgb image (h, w, 3) float32)]"""
    grey = is_grey(trc)
    if direction == "linearize":
        out = [("codes", planes(codes(), grey).astype(np.float32)),
               ("edges", pad_image(lin_edge_values(trc, csp_min, csp_max), grey))]
    else:
        c = codes()
        lin = linearize(np.stack([c, c, c], -1), trc, csp_min, csp_max, luma)[..., 0]
        out = [("codes", planes(lin, grey).astype(np.float32)),
               ("edges", pad_image(delin_edge_values(trc, csp_min, csp_max, luma), grey,
                                   fill=F(csp_max) * 0.25))]
    return out


# ---- error units -------------------------------------------------------------------------------
def local_slope(fn, x):
    """change of the true curve per 16-bit input code at x: central difference at +-1/65535"""
    x = np.asarray(x, np.float64)
    return np.abs(fn(x + H) - fn(x - H)) / 2.0


def half_ulp(truth):
    """half an fp32 ulp of the result: the floor of any fp32 evaluation"""
    t = np.abs(np.asarray(truth, np.float64)).astype(np.float32)
    return 0.5 * np.spacing(np.maximum(t, np.finfo(np.float32).tiny)).astype(np.float64)


def errors(got, truth, slope=None):
    """(err, floor, flat, unit): per-sample error and fp32 floor in the stage's unit -- 16-bit codes of the
    output (slope None: delinearize, sigmoidize) or local codes, |got - truth| / slope (linearize,
    unsigmoidize) -- and the mask of samples whose slope is 0: the clamped region, where err is 0
    and the caller requires exact equality (assert_flat); unit: err = |got - truth| * unit."""
    got = np.asarray(got, np.float64)
    d = np.abs(got - truth)
    fl = half_ulp(truth)
    if slope is None:
        return d * 65535.0, fl * 65535.0, np.zeros(d.shape, bool), np.full(d.shape, 65535.0)
    flat = slope == 0
    unit = np.where(flat, 0.0, 1.0 / np.where(flat, 1.0, slope))
    return d * unit, fl * unit, flat, unit


def assert_flat(got, truth, x, flat, at_lo, at_hi=None):
    """Where the true curve does not move with the input (the clamped region) the result is exact:
    equal to the truth where that is an fp32 number, else bit for bit what the implementation
    itself returns at the clamp (at_lo: its value for input 0; at_hi: for input 1)."""
    if not flat.any():
        return
    g, t, xx = got[flat], truth[flat], x[flat]
    same = g.astype(np.float64) == t
    edge = np.where(xx < 0.5, at_lo, at_hi if at_hi is not None else at_lo)
    ok = same | (g == edge)
    assert ok.all(), ("clamped region not exact", xx[~ok][:4], g[~ok][:4], t[~ok][:4])


# ---- one case of the sweep: inputs, truth, unit, and the statement held ----------------------
WELL = 0.05
"""A sample is "well-conditioned" where its conditioning floor (Case.measure: cond) is at most this:
a tenth of the half code that decides a 16-bit store."""
K = 5
"""max error(implementation) <= K * max(E_orc, E_ulp). Set from the float32 emulation (Emu32) on
the same inputs: its largest ratio to max(E_orc, E_ulp) over every curve, direction, black level and
the sigmoid cases is 2.19 (test_transfer_f64.py recomputes and prints it); the emulation's
primitives round to 0.5 ulp and the hardware's to 1, hence twice that, rounded up."""


class Report:
    """per-sample figures of one implementation on one case (1-D, all images concatenated)"""

    def __init__(self, parts):
        cat = lambda i: np.concatenate([np.ravel(p[i]) for p in parts])     # noqa: E731
        self.err, self.fl, self.cond, self.flat, self.truth, self.got, self.x, self.unit = \
            map(cat, range(8))
        self.well = self.cond <= WELL

    @property
    def E(self):
        return float(self.err.max())

    @property
    def E_well(self):
        return float(self.err[self.well].max())

    @property
    def E_ulp(self):
        return float(self.fl.max())

    @property
    def E_ulp_well(self):
        return float(self.fl[self.well].max())


class Case:
    def __init__(self, kind, trc=None, csp_min=0.0, csp_max=1.0, luma=BT709_LUMA,
                 center=0.75, slope=6.5):
        self.kind, self.trc, self.mn, self.mx, self.luma = kind, trc, csp_min, csp_max, luma
        self.center, self.slope = center, slope
        self.local = kind in ("linearize", "unsigmoidize")      # unit: local codes

    def fn(self, rgb, be=F64, branch=None, **kw):
        if self.kind == "linearize":
            return linearize(rgb, self.trc, self.mn, self.mx, self.luma, be=be, branch=branch)
        if self.kind == "delinearize":
            return delinearize(rgb, self.trc, self.mn, self.mx, self.luma, be=be, branch=branch,
                               **kw)
        f = sigmoidize if self.kind == "sigmoidize" else unsigmoidize
        return f(rgb, self.center, self.slope, be=be)

    def images(self):
        """[(name, (h, w, 3) float32)]: what the implementation is given"""
        if self.kind in ("linearize", "delinearize"):
            return inputs(self.trc, self.kind, self.mn, self.mx, self.luma)
        c = codes()
        if self.kind == "unsigmoidize":
            # (sweep the output over the code range too: the images of every code)
            c = np.concatenate([c[::2], sigmoidize(c[1::2], self.center, self.slope)])
        return [("codes", planes(c).astype(np.float32)), ("edges", pad_image(sigmoid_values()))]

    def measure_image(self, img, got):
        """per-sample figures of one result image: the tuple Report concatenates"""
        x = img.astype(np.float64)
        got = np.asarray(got)[..., :3]
        truth = self.fn(x)
        slope = local_slope(self.fn, x) if self.local else None
        err, fl, flat, unit = errors(got, truth, slope)
        cond = fl
        mc = black_scale_in(self.trc, self.mn, self.mx) if self.kind == "delinearize" else None
        if mc:
            # what one rounding of m * x + c (half an ulp of the larger term) does behind the
            # curve, whose slope is unbounded towards black for a pure power law
            d = half_ulp(np.maximum(np.abs(mc[0] * x), abs(mc[1])))
            with np.errstate(invalid="ignore"):
                c2 = np.maximum(np.abs(self.fn(x, dv=d) - truth), np.abs(self.fn(x, dv=-d) - truth))
            cond = np.maximum(fl, c2 * 65535.0)
        return err, fl, cond, flat, truth, got.astype(np.float64), x, unit

    def measure(self, results):
        """Report of an implementation's results on images()"""
        return Report([self.measure_image(img, got)
                       for (name, img), got in zip(self.images(), results)])

    def knee_samples(self):
        """fp32 inputs at the knees (1-D), all of them among images()["edges"]"""
        if self.kind not in ("linearize", "delinearize"):
            return np.zeros(0, np.float32)
        tri = knee_inputs(self.trc, self.kind, self.mn, self.mx)
        return np.asarray([x for t in tri for x in t], np.float32)


def check(case, rep, orc_rep, k=K, what="GPU", knees=True):
    """The statement of tests/test_gpu_transfer_sweep.py for one implementation's Report, given the
    oracle's on the same inputs. Returns the figures it printed."""
    assert np.isfinite(rep.got).all(), (what, "not finite", rep.x[~np.isfinite(rep.got)][:4])
    # the clamped region is exact
    at_lo = rep.got[np.argmin(np.abs(rep.x))]       # (input +-0 is in every set)
    at_hi = rep.got[np.argmin(np.abs(rep.x - 1.0))]
    assert_flat(rep.got, rep.truth, rep.x, rep.flat, at_lo, at_hi)
    # condition: half a code from float64 -- beyond it a 16-bit store lands on the wrong code --
    # wherever fp32 can state that at all (cond <= 0.5 / k), else k roundings of the floor
    pq_lin = case.kind == "linearize" and TRC.get(case.trc, case.trc) == TRC["pq"]
    if pq_lin:
        # (7.5e-6 relative IS half a code where the curve is steepest, and is stated over the codes;
        # below code 1 -- the edge set's 1e-30 .. half a code -- the half code itself holds)
        nz = rep.x >= H
        rel = np.abs(rep.got - rep.truth)[nz] / rep.truth[nz]
        assert rel.max() <= 7.5e-6, (what, "PQ EOTF relative error", float(rel.max()))
        assert rep.err.max() <= 0.5, (what, "PQ EOTF", float(rep.err.max()))
        assert np.all(rep.got[rep.truth == 0] == 0.0)
    else:
        lim = np.maximum(0.5, k * rep.cond)
        bad = rep.err > lim
        assert not bad.any(), (what, "more than half a code from float64", int(bad.sum()),
                               rep.x[bad][:4], rep.err[bad][:4], rep.cond[bad][:4])
    # measured against the oracle: on every sample, and on the well-conditioned ones alone (where
    # the floor is not set by a handful of samples next to black)
    b_all = k * max(orc_rep.E, orc_rep.E_ulp)
    b_well = k * max(orc_rep.E_well, orc_rep.E_ulp_well)
    assert rep.E <= b_all, (what, rep.E, "bound", b_all)
    assert rep.E_well <= b_well, (what, rep.E_well, "bound (well-conditioned samples)", b_well)
    # knees: on the truth's branch, and not on the other one
    ks = case.knee_samples() if knees else np.zeros(0)
    if ks.size:
        x = np.stack([ks.astype(np.float64)] * 3, -1)
        up, lo, tr = case.fn(x, branch=True)[..., 0], case.fn(x, branch=False)[..., 0], case.fn(x)[..., 0]
        other = np.where(tr == up, lo, up)
        for i, v in enumerate(ks):
            j = np.flatnonzero(rep.x == np.float64(v))
            assert j.size, ("knee sample not in the input set", v)
            j = j[0]
            unit = rep.unit[j]
            assert rep.err[j] <= b_well, (what, "knee: off the truth's branch", v, rep.err[j])
            if abs(tr[i] - other[i]) * unit > 2 * b_well:
                assert abs(rep.got[j] - other[i]) * unit > b_well, (what, "knee: on the other branch", v)
    return dict(E=rep.E, E_well=rep.E_well, bound=b_all, bound_well=b_well)


def colour_images(case):
    """HLG only: 64 x 64 random saturated colours (delinearize: their linear images), which the grey
    sweeps cannot see -- the OOTF's luma couples the channels"""
    if not is_grey(case.trc) or case.kind not in ("linearize", "delinearize"):
        return []
    c = hlg_colours()
    if case.kind == "delinearize":
        c = linearize(c.astype(np.float64), case.trc, case.mn, case.mx, case.luma).astype(np.float32)
    return [("colours", c)]


def check_colours(case, got, orc_got, img, k=K, what="GPU"):
    """maximum absolute errors compared directly: (E, E_orc, E_ulp)"""
    truth = case.fn(img.astype(np.float64))
    e = float(np.abs(np.asarray(got, np.float64)[..., :3] - truth).max())
    eo = float(np.abs(np.asarray(orc_got, np.float64)[..., :3] - truth).max())
    eu = float(half_ulp(truth).max())
    assert np.isfinite(np.asarray(got)).all()
    assert e <= k * max(eo, eu), (what, "colours", e, "bound", k * max(eo, eu))
    return e, eo, eu


# ---- the same statement for results that went through a texel format (the renderer's kernels) ----
def sample_bounds(rep, orc_rep, k=K):
    """the bound of `check`, per sample and in the case's unit: k * max(E_orc, E_ulp) of the
    well-conditioned samples on those, max(0.5, k * cond) on the others"""
    b = k * max(orc_rep.E_well, orc_rep.E_ulp_well)
    return np.where(rep.well, b, np.maximum(0.5, k * rep.cond))


def f16_half_ulp(truth):
    t = np.abs(np.asarray(truth, np.float64)).astype(np.float16)
    return 0.5 * np.spacing(t).astype(np.float64)


def excess_linear(case, rep, orc_rep, f16=False, extra=0.0):
    """How far a linearize result is beyond what it may be, in absolute terms (<= 0: fine): the bound
    of `check`, plus half an f16 ulp where the value went through an f16 texel, plus `extra`.
    PQ: 7.5e-6 relative, as everywhere."""
    d = np.abs(rep.got - rep.truth)
    if TRC.get(case.trc, case.trc) == TRC["pq"]:
        tol = 7.5e-6 * np.abs(rep.truth)
    else:
        with np.errstate(divide="ignore"):
            tol = np.where(rep.unit > 0, sample_bounds(rep, orc_rep) / rep.unit, 0.0)
    if f16:
        tol = tol + f16_half_ulp(rep.truth) * (1 + 2.0 ** -10)
    return d - tol - extra


def excess_stored(stored, rep, orc_rep, top=65535.0):
    """How far a 16-bit code stored from a delinearize result is beyond what it may be (<= 0: fine):
    round(truth * 65535), either neighbour where the truth lies within the bound of `check` of a
    rounding boundary -- |stored - truth * 65535| <= 0.5 + bound."""
    t = np.clip(rep.truth, 0.0, 1.0) * top
    return np.abs(np.ravel(stored).astype(np.float64) - t) - 0.5 - sample_bounds(rep, orc_rep)
