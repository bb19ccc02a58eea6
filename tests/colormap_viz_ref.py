"""numpy restatement of the colour map's full path WITH its diagnostics
(pl_color_map_params.show_clipping / .visualize_lut; reference src/shaders/colorspace.c:1409-1581,
:1791-2017), in the reference's operation order.

run(..., dt=np.float64) is the truth the GPU is held to; run(..., dt=np.float32) rounds every
intermediate to float32 (numpy's float32 arithmetic does exactly that) and so models a faithful
fp32 shader: the distance between the two runs, per pixel class, is the R32 the tolerance of
tests/test_gpu_colormap_viz.py is derived from. Every comparison the path takes is recorded with the
margin it was taken by, so that the samples whose decisions are ill-conditioned can be set aside.

Parameter inference and the two LUTs come from tests/colormap_ref.py (Tier-0 code); the PQ pair
and the LUT interpolation are the formulas of tests/colormap_f64.py, written once for both
precisions (tests/test_colormap_viz_ref.py pins them to that module in float64).

Test infrastructure only.
"""
import ctypes as C

import numpy as np

import colormap_f64 as c64
import colormap_ref as cr
import ref_structs as R

EPS = 1e-6
MARGIN = 1e-4           # a decision taken by less is ill-conditioned: the sample is set aside
SET_ASIDE_CAP = 0.02    # ... and at most this share of a test's samples may be
UNMARKED, CLIP_HI, CLIP_LO, TONE_PLOT, GAMUT_PLOT = range(5)
CLASS_NAMES = ["unmarked", "clip_hi", "clip_lo", "tone plot", "gamut plot"]


class Decisions:
    """Every comparison of the path: its outcome as one bit per pixel, and the smallest margin"""

    def __init__(self, shape):
        self.margin = np.full(shape, np.inf)
        self.bits = np.zeros(shape, np.int64)
        self.n = 0

    def take(self, cond, margin, where=True):
        w = np.broadcast_to(np.asarray(where, bool), self.margin.shape)
        self.margin = np.where(w, np.minimum(self.margin, np.asarray(margin, np.float64)), self.margin)
        self.bits = self.bits | (np.where(w, cond, False).astype(np.int64) << self.n)
        self.n += 1
        return cond


def mix(x, y, a):
    return x * (1 - a) + y * a


def smoothstep(e0, e1, x):
    t = np.clip((x - e0) / (e1 - e0), 0, 1)
    return t * t * (3 - 2 * t)


def fract(x):
    return x - np.floor(x)


def fract_margin(f, thr):
    """distance of fract(..) = f from where `f < thr` changes: thr itself, and the wrap at 0 = 1"""
    return np.minimum(np.abs(f - thr), np.minimum(f, 1 - f))


def pq_oetf(x, dt):
    y = np.maximum(x, dt(0)) ** dt(c64.M1)
    return ((dt(c64.C1) + dt(c64.C2) * y) / (dt(1) + dt(c64.C3) * y)) ** dt(c64.M2)


def pq_eotf(v, dt):
    p = np.maximum(v, dt(0)) ** (dt(1) / dt(c64.M2))
    return (np.maximum(p - dt(c64.C1), dt(0)) / (dt(c64.C2) - dt(c64.C3) * p)) ** (dt(1) / dt(c64.M1))


def mat3(m, v, dt):
    """row-major 3x3 `m` times the colour `v` (.., 3), summed in component order"""
    m = np.asarray(m, np.float64).reshape(3, 3).astype(dt)
    return np.stack([m[k, 0] * v[..., 0] + m[k, 1] * v[..., 1] + m[k, 2] * v[..., 2]
                     for k in range(3)], -1)


def lut1d(lut, x, dt):
    n = len(lut)
    pos = np.clip(x, dt(0), dt(1)) * dt(n - 1)
    base = np.floor(pos)
    i0, i1 = base.astype(int), np.ceil(pos).astype(int)
    lut = lut.astype(dt)
    return mix(lut[i0], lut[i1], pos - base)


def lut3d(lut_u16, size, idx, dt):
    """trilinear: x, then y, then z (shaders/lut.c:700-715)"""
    sx, sy, sz = size
    lut = (lut_u16.reshape(sz, sy, sx, 4)[..., :3].astype(dt) / dt(65535))
    pos = [np.clip(idx[k], dt(0), dt(1)) * dt(s - 1) for k, s in enumerate(size)]
    i0 = [np.floor(p).astype(int) for p in pos]
    i1 = [np.minimum(i + 1, s - 1) for i, s in zip(i0, size)]
    f = [(p - np.floor(p))[..., None] for p in pos]
    c = {}
    for dz in (0, 1):
        for dy in (0, 1):
            z, y = (i1 if dz else i0)[2], (i1 if dy else i0)[1]
            c[dz, dy] = mix(lut[z, y, i0[0]], lut[z, y, i1[0]], f[0])
    return mix(mix(c[0, 0], c[0, 1], f[1]), mix(c[1, 0], c[1, 1], f[1]), f[2])


def lut3d_cubic(lut_u16, size, idx, dt):
    """shaders/lut.c:718-760: B-spline weights, eight linear fetches"""
    g0, h = [], []
    for k, n in enumerate(size):
        scale = dt(n - 1)
        pos = idx[k] * scale
        fpos = pos - np.floor(pos)
        base = pos - fpos
        inv = dt(1) - fpos
        w0, w3 = dt(1 / 6) * inv * inv * inv, dt(1 / 6) * fpos * fpos * fpos
        w1 = dt(2 / 3) - dt(0.5) * fpos * fpos * (dt(2) - fpos)
        w2 = dt(2 / 3) - dt(0.5) * inv * inv * (dt(2) - inv)
        g0.append(w0 + w1)
        h.append(((w1 / (w0 + w1) - dt(1) + base) / scale, (w3 / (w2 + w3) + dt(1) + base) / scale))
    out = 0
    for t in range(8):
        bits = [(t >> k) & 1 for k in range(3)]
        w = 1
        for k in range(3):
            w = w * ((dt(1) - g0[k]) if bits[k] else g0[k])
        out = out + w[..., None] * lut3d(lut_u16, size, [h[k][bits[k]] for k in range(3)], dt)
    return out


def bt1886_inverse(L, csp_min, csp_max, dt):
    lb, lw = dt(csp_min) ** dt(1 / 2.4), dt(csp_max) ** dt(1 / 2.4)
    a, b = (lw - lb) ** dt(2.4), lb / (lw - lb)
    return np.maximum(L, dt(0)) ** dt(1 / 2.4) * (dt(1) / a) ** dt(1 / 2.4) - b


def resolve(src, dst, tone="spline", gamut="perceptual", tricubic=False):
    """colormap_ref.resolve plus what the diagnostics read: how the tone curve is evaluated (a
    table, or the closed forms of `clip` and `linear`: colorspace.c:1824-1849) and the two
    LMS -> RGB matrices of the gamut plot"""
    r = cr.resolve(src, dst, tone=tone.encode(), gamut=gamut.encode())
    lib = cr._cpu()
    tp, gp = r["tone"], r["gamut"]
    r["tone_kind"] = tone if tone in ("clip", "linear") else "lut"
    r["tricubic"] = tricubic
    r["lms2src"] = R.m3(lib.pl_ipt_lms2rgb(C.byref(gp.input_gamut)))
    r["lms2dst"] = R.m3(lib.pl_ipt_lms2rgb(C.byref(gp.output_gamut)))
    norm = lambda pq: lib.pl_hdr_rescale(R.HDR_PQ, R.HDR_NORM, pq)  # noqa: E731
    r["range"] = dict(in_min=tp.input_min, in_max=tp.input_max, in_avg=tp.input_avg,
                      out_min=tp.output_min, out_max=tp.output_max,
                      rgb_in_min=norm(tp.input_min), rgb_in_max=norm(tp.input_max),
                      g_min=gp.min_luma, g_max=gp.max_luma,
                      g_rgb_min=norm(gp.min_luma), g_rgb_max=norm(gp.max_luma),
                      exposure=tp.constants.exposure)
    return r


def plot_pos(w, h, rect, dt):
    """rect_pos (:1409-1422) at the pixel centres of a w x h output rect; y runs upwards"""
    x0, y0, x1, y1 = [np.float32(v) for v in rect]
    if not x0 and not x1:
        x1 = np.float32(1)
    if not y0 and not y1:
        y1 = np.float32(1)
    ax0, ax1 = -x0 / (x1 - x0), (np.float32(1) - x0) / (x1 - x0)
    ay0, ay1 = -y1 / (y0 - y1), (np.float32(1) - y1) / (y0 - y1)
    mx = (dt(1) / dt(w)) * (np.arange(w).astype(dt) + dt(0.5))
    my = (dt(1) / dt(h)) * (np.arange(h).astype(dt) + dt(0.5))
    px = mix(dt(ax0), dt(ax1), mx)[None, :] + np.zeros((h, 1), dt)
    py = mix(dt(ay0), dt(ay1), my)[:, None] + np.zeros((1, w), dt)
    return px, py


def run(img, r, show_clipping=False, visualize_lut=False, rect=(0, 0, 1, 1), hue=0.0, theta=0.0,
        prelinearized=False, dt=np.float64):
    """-> dict(out (h, w, 3) delinearised, cls (h, w) pixel class, bits / margin (h, w): the
    decisions taken and their smallest margin, raised: {source: (h, w) bool} per clip source)"""
    dt = np.dtype(dt).type
    h, w = img.shape[:2]
    K = r["range"]
    kw = r["kw"]
    need_tone, need_gamut = r["need_tone"], r["need_gamut"]
    assert need_tone or need_gamut, "matrix-only path: the diagnostics do nothing"
    dec = Decisions((h, w))
    raised = {}

    rgb = img[..., :3].astype(dt)
    if not prelinearized:
        rgb = pq_eotf(rgb, dt) * dt(c64.K10)
    lms = mat3(kw["rgb2lms"], rgb, dt)
    ipt = mat3(c64.LMS2IPT, pq_oetf(dt(c64.K203) * lms, dt), dt)
    I, P, T = ipt[..., 0], ipt[..., 1], ipt[..., 2]
    i_orig = I

    clip_hi = clip_lo = np.zeros((h, w), bool)
    if show_clipping:
        hi = dt(np.float32(K["rgb_in_max"]) + np.float32(EPS))
        lo = dt(np.float32(K["rgb_in_min"]) - np.float32(EPS))
        ihi = dt(np.float32(K["in_max"]) + np.float32(EPS))
        ilo = dt(np.float32(K["in_min"]) - np.float32(EPS))
        # (`clip_hi = clip_hi || ..`: a test behind a flag that is already set is not taken;
        # raised[] has every source's own outcome all the same, for the tests' census)
        raised.update(hi_rgb=rgb.max(-1) > hi, lo_rgb=rgb.min(-1) < lo, hi_I=I > ihi, lo_I=I < ilo)
        clip_hi = dec.take(raised["hi_rgb"], np.abs(rgb.max(-1) - hi))
        clip_lo = dec.take(raised["lo_rgb"], np.abs(rgb.min(-1) - lo))
        clip_hi = clip_hi | dec.take(raised["hi_I"], np.abs(I - ihi), ~clip_hi)
        clip_lo = clip_lo | dec.take(raised["lo_I"], np.abs(I - ilo), ~clip_lo)

    if r["tone_kind"] == "clip":
        curve = lambda x: np.clip(x, dt(np.float32(K["in_min"])), dt(np.float32(K["in_max"])))  # noqa: E731
    elif r["tone_kind"] == "linear":
        f32 = np.float32
        gain, scale = f32(K["exposure"]), f32(K["in_max"]) - f32(K["in_min"])
        a, b = dt(gain / scale), dt(-gain / scale * f32(K["in_min"]))
        c, d = dt(f32(K["out_max"]) - f32(K["out_min"])), dt(f32(K["out_min"]))
        curve = lambda x: c * np.clip(a * x + b, dt(0), dt(1)) + d  # noqa: E731
    else:
        tp = kw.get("tone_p", (0, 0))
        curve = lambda x: lut1d(kw["tone_lut"], dt(np.float32(tp[0])) * x + dt(np.float32(tp[1])), dt)  # noqa: E731
    if need_tone:
        I = curve(I)
        hull = lambda v: ((v - dt(6)) * v + dt(9)) * v   # noqa: E731
        k = np.minimum(i_orig / I, hull(I) / hull(i_orig))
        P, T = P * k, T * k

    in_rect = np.zeros((h, w), bool)
    if visualize_lut:
        px, py = plot_pos(w, h, rect, dt)
        lo_edge, hi_edge = np.minimum(px, py), np.maximum(px, py)
        in_rect = dec.take((lo_edge >= 0) & (hi_edge <= 1),
                           np.minimum(np.abs(lo_edge), np.abs(hi_edge - 1)))
    plot_gamut = visualize_lut and need_gamut
    plot_tone = visualize_lut and need_tone

    if need_gamut:
        size = kw["gamut_size"]
        fetch = lut3d_cubic if r["tricubic"] else lut3d
        k_atan = dt(np.float32(0.159155))
        idx = [dt(np.float32(kw["gamut_scale"])) * I + dt(np.float32(kw["gamut_offset"])),
               dt(2) * np.sqrt(P * P + T * T), k_atan * np.arctan2(T, P) + dt(0.5)]
        o = fetch(kw["gamut_lut"], size, idx, dt)
        half = dt(32768.0) / dt(65535.0)
        I, P, T = o[..., 0], o[..., 1] - half, o[..., 2] - half
        if show_clipping:
            # (2 |PT| is never negative in any arithmetic: it takes no part in the `< 0` test)
            low = np.minimum(idx[0], idx[2])
            high = np.maximum(np.maximum(idx[0], idx[1]), idx[2])
            raised.update(lo_idx=low < 0, hi_idx=high > 1)
            clip_lo = clip_lo | dec.take(raised["lo_idx"], np.abs(low), ~clip_lo)
            clip_hi = clip_hi | dec.take(raised["hi_idx"], np.abs(high - 1), ~clip_hi)
        if plot_gamut:
            f32 = np.float32
            pqmin, pqmax = dt(f32(K["g_min"])), dt(f32(K["g_max"]))
            rgbmin, rgbmax = dt(f32(K["g_rgb_min"])), dt(f32(K["g_rgb_max"]))
            hue_, theta_ = dt(f32(hue)), dt(f32(theta))
            sh, ch, st, ct = np.sin(hue_), np.cos(hue_), np.sin(theta_), np.cos(theta_)
            base = mix(dt(0.5), mix(pqmin, pqmax, dt(0.6)), st)
            # rot1 * rot2, then * dir = (pos.y - 1/2, pos.x - 1/2, 0)
            dx, dy = py - dt(0.5), px - dt(0.5)
            sI = base + (ct * dx + dt(0) * dy)
            sP = (-sh * st) * dx + ch * dy
            sT = (ch * st) * dx + sh * dy
            s_lms = pq_eotf(mat3(c64.IPT2LMS, np.stack([sI, sP, sT], -1), dt), dt) * dt(c64.K10)
            rgbsrc, rgbdst = mat3(r["lms2src"], s_lms, dt), mat3(r["lms2dst"], s_lms, dt)

            def inside(v):
                m = np.minimum(np.abs(v.max(-1) - rgbmax), np.abs(v.min(-1) - rgbmin))
                return dec.take((v.max(-1) < rgbmax) & (v.min(-1) > rgbmin), m, in_rect)
            insrc, indst = inside(rgbsrc), inside(rgbdst)
            sidx = [(sI - pqmin) / (pqmax - pqmin), dt(2) * np.sqrt(sP * sP + sT * sT),
                    k_atan * np.arctan2(sT, sP) + dt(0.5)]
            m = fetch(kw["gamut_lut"], size, sidx, dt)
            mI, mP, mT = m[..., 0], m[..., 1] - half, m[..., 2] - half
            mhue, mchroma = np.arctan2(mT, mP), np.sqrt(mP * mP + mT * mT)
            neither = ~insrc & ~indst
            oI = np.where(neither, I, np.where(insrc & ~indst, mI - dt(0.1),
                                               np.where(indst & ~insrc, mI + dt(0.1), mI)))
            oP, oT = np.where(neither, P, mP), np.where(neither, T, mT)
            live = in_rect & insrc
            f1 = fract(dt(50) * mI)
            on = dec.take(f1 < dt(0.1), fract_margin(f1, 0.1), live) & live
            kk = smoothstep(dt(0.1), dt(0), np.abs(st))
            n = np.sqrt(mchroma)
            oI = np.where(on, mix(oI, mix(mI, dt(0.3), dt(0.5)), kk), oI)
            oP = np.where(on, mix(oP, n * (mP / mchroma), kk), oP)
            oT = np.where(on, mix(oT, n * (mT / mchroma), kk), oT)
            f2 = fract(dt(10) * (mhue - hue_))
            on = dec.take(f2 < dt(0.1), fract_margin(f2, 0.1), live) & live
            kk = smoothstep(dt(0.3), dt(0), np.abs(ct))
            oI = np.where(on, mix(oI, mI - dt(0.05), kk), oI)
            oP = np.where(on, mix(oP, dt(1.2) * mP, kk), oP)
            oT = np.where(on, mix(oT, dt(1.2) * mT, kk), oT)
            f3 = fract(dt(100) * mchroma)
            on = dec.take(f3 < dt(0.1), fract_margin(f3, 0.1), live) & live
            oI = np.where(on, mix(oI, mI + dt(0.1), dt(0.5)), oI)
            oP = np.where(on, mix(oP, dt(0.4) * mP, dt(0.5)), oP)
            oT = np.where(on, mix(oT, dt(0.4) * mT, dt(0.5)), oT)
            I, P, T = np.where(in_rect, oI, I), np.where(in_rect, oP, P), np.where(in_rect, oT, T)

    lms_out = pq_eotf(mat3(c64.IPT2LMS, np.stack([I, P, T], -1), dt), dt) * dt(c64.K10)
    col = mat3(kw["lms2rgb"], lms_out, dt)

    if show_clipping:
        k23 = dt(2) / dt(3)
        k = col[..., 0] * k23 + col[..., 1] * k23 + col[..., 2] * k23
        inv = np.clip(k[..., None] - col, dt(0), dt(1))
        cmin, cmax = inv.min(-1, keepdims=True), inv.max(-1, keepdims=True)
        sat = smoothstep(cmin - dt(1e-6), cmax, inv)
        red = np.array([1, 0, 0], dt)
        marked_hi = mix(red, sat, smoothstep(dt(0), dt(0.3), cmax - cmin))
        marked_lo = mix(col, np.array([0, 0.3, 0.3], dt), dt(0.5))
        col = np.where(clip_hi[..., None], marked_hi, np.where(clip_lo[..., None], marked_lo, col))

    if plot_tone:
        f32 = np.float32
        xmin, xmax, xavg = dt(f32(K["in_min"])), dt(f32(K["in_max"])), dt(f32(K["in_avg"]))
        ymin, ymax = dt(f32(K["out_min"])), dt(f32(K["out_max"]))
        alpha = f32(0.8) * (f32(np.cos(f32(theta))) ** f32(5) if need_gamut else f32(1))
        alpha = np.full((h, w), dt(alpha))
        vv = curve(px)

        # (`clip` inside its domain returns its argument itself, in any arithmetic: vv against
        # pos.x is then no decision that rounding could turn)
        exact = r["tone_kind"] == "clip"

        def cmp(a, b, where, same=False):    # a < b
            return dec.take(a < b, np.inf if same else np.abs(a - b), where)
        live = in_rect
        def either(a, b, c, d, where):      # a < b || c < d
            first = cmp(a, b, where)
            return first | cmp(c, d, where & ~first)
        out_src = either(px, xmin, xmax, px, live)
        live = in_rect & ~out_src
        out_dst = either(py, ymin, ymax, py, live)
        also_src = either(py, xmin, xmax, py, live & out_dst)
        dom = live & ~out_dst
        diag = dec.take(np.abs(px - py) < dt(1e-3), np.abs(np.abs(px - py) - 1e-3), dom)
        under = cmp(py, vv, dom & ~diag)
        sel = dom & ~diag & under
        brighter = cmp(px, vv, sel, exact)
        brighter = brighter & cmp(px, py, sel & brighter)
        sel = dom & ~diag & ~under
        darker = cmp(vv, px, sel, exact)
        darker = darker & cmp(py, px, sel & darker)
        inverse = cmp(xmax, py, dom)
        black = cmp(py, xmin, dom & ~inverse)
        avg = (xavg > 0) & dec.take(np.abs(px - xavg) < dt(1e-3), np.abs(np.abs(px - xavg) - 1e-3),
                                    dom & bool(xavg > 0))
        viz = col.copy()

        def paint(where, rgb_):
            viz[where] = np.array(rgb_, dt)
        paint(live & out_dst & also_src, (0.1, 0.1, 0.5))
        paint(live & out_dst & ~also_src, (0.2, 0.05, 0.05))
        paint(dom & diag, (0.2, 0.2, 0.2))
        sel = dom & ~diag & under
        alpha = np.where(sel, alpha * dt(0.6), alpha)
        paint(sel, (0.05, 0.05, 0.05))
        viz[sel & brighter, 0], viz[sel & brighter, 1] = dt(0.5), dt(0.7)
        paint(dom & ~diag & ~under & darker, (0.0, 0.1, 0.2))
        sel = dom & inverse
        viz[sel] = mix(viz[sel], np.array([0.2, 0.5, 0.8], dt), dt(0.5))
        sel = dom & ~inverse & black
        viz[sel] = mix(viz[sel], np.array([0, 0, 0], dt), dt(0.3))
        paint(dom & avg, (0.5, 0.5, 0.5))
        col = np.where(in_rect[..., None], mix(col, viz, alpha[..., None]), col)

    _, dmin, dmax, _ = r["delin"]
    out = bt1886_inverse(col, dmin, dmax, dt)

    cls = np.full((h, w), UNMARKED)
    cls[clip_lo] = CLIP_LO
    cls[clip_hi] = CLIP_HI
    if plot_tone:
        cls[in_rect] = TONE_PLOT
    if plot_gamut:
        cls[in_rect] = GAMUT_PLOT
    return dict(out=out, cls=cls, bits=dec.bits, margin=dec.margin, raised=raised, in_rect=in_rect)


def compare(img, r, unorm=False, **kw):
    """Both runs -> (truth, keep, r32): the float64 result, the samples that are not set aside, and
    per pixel class the largest distance between the float32 and the float64 run over them. The
    two runs must have taken the same decisions on every sample kept. unorm: the target is a
    unorm texture, which holds 0 .. 1: both runs end in that clamp."""
    t = run(img, r, dt=np.float64, **kw)
    s = run(img, r, dt=np.float32, **kw)
    if unorm:
        t["out"], s["out"] = np.clip(t["out"], 0.0, 1.0), np.clip(s["out"], 0.0, 1.0)
    keep = t["margin"] >= MARGIN
    assert np.array_equal(t["bits"][keep], s["bits"][keep]), \
        "the float32 run takes another decision on a sample that is not set aside"
    dist = np.abs(s["out"].astype(np.float64) - t["out"]).max(-1)
    r32 = {c: float(dist[keep & (t["cls"] == c)].max()) for c in range(5)
           if (keep & (t["cls"] == c)).any()}
    return t, keep, r32


def tolerance(r32):
    """max(4 R32, one 16-bit code), per class"""
    return {c: max(4.0 * v, 1.0 / 65535.0) for c, v in r32.items()}


# ---- the inputs of tests/test_gpu_colormap_viz.py (and of the CPU check of their set-aside share) ----
def spaces(target="bt709"):
    import libplacebo_amd as pl
    return (cr.make_csp(pl.PRIM["bt2020"], pl.TRC["pq"], max_luma=1000.0),
            cr.make_csp(pl.PRIM[target], pl.TRC["bt1886"]))


def _rgb_of_ipt(ipt, r):
    """linear source RGB whose IPT (in front of the tone map) is `ipt`, in float64"""
    lmspq = ipt @ np.linalg.inv(c64.LMS2IPT).T
    lms = pq_eotf(lmspq, np.float64) / c64.K203
    return lms @ np.linalg.inv(np.array(r["kw"]["rgb2lms"], np.float64).reshape(3, 3)).T


def clip_frame(r, w=64, h=48, seed=3):
    """Linear-light BT.2020 (pl_color_map_args.prelinearized; 1.0 = 203 cd/m^2), in bands of rows.
    -> (frame, {band: (h, w) bool})"""
    rng = np.random.default_rng(seed)
    img = np.ones((h, w, 4), np.float32)
    grey = rng.uniform(0.05, 2.5, (h, w, 1))
    img[..., :3] = grey * (0.8 + 0.4 * rng.random((h, w, 3)))       # in range, mildly coloured
    band = {}

    def rows(name, a, b, cols=slice(None)):
        m = np.zeros((h, w), bool)
        m[a:b, cols] = True
        band[name] = m
        return m
    m = rows("4000 nits", 6, 12)
    img[m, :3] = (4000.0 / 203.0) * (0.85 + 0.15 * rng.random((m.sum(), 3)))
    m = rows("negative", 12, 18)
    img[m, :3] = rng.uniform(0.2, 1.5, (m.sum(), 3))
    img[m, 1] = -rng.uniform(0.01, 0.2, m.sum())
    m = rows("below black", 18, 19)
    img[m, :3] = -rng.uniform(0.005, 0.05, (m.sum(), 1))            # every component negative
    m = rows("black", 19, 20, slice(0, 8))
    img[m, :3] = 0.0
    m = rows("saturated", 24, 30)
    prim = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0]], np.float64)
    which = prim[np.arange(m.sum()) % 6]
    img[m, :3] = which * rng.uniform(0.5, 1.5, (m.sum(), 1)) + 0.002
    # hues at the two ends of atan's range: P < 0 and T a hair below / above zero, so that
    # (0.5 / pi) * atan(T, P) + 0.5 leaves [0, 1] by the rounding of 0.5 / pi as printed
    for name, row, cols, sign in (("hue -pi", 30, slice(0, 36), -1.0), ("hue +pi", 31, slice(0, 8), 1.0)):
        m = rows(name, row, row + 1, cols)
        n = m.sum()
        ipt = np.stack([rng.uniform(0.3, 0.5, n), -rng.uniform(0.05, 0.12, n), np.zeros(n)], -1)
        ipt[:, 2] = sign * 5e-7 * np.abs(ipt[:, 1])
        img[m, :3] = _rgb_of_ipt(ipt, r)
    return img, band


def picture(w, h, seed=7):
    """PQ-coded BT.2020 content (tests/test_gpu_color.py: hdr_test_frame), every code >= 0.1"""
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 4)).astype(np.float32)
    img[..., :3] *= np.linspace(0.15, 0.75, w, dtype=np.float32)[None, :, None]
    img[: h // 4, :, 1:3] *= 0.4
    img[h // 4: h // 2, :, 0] *= 0.4
    img[..., :3] = 0.1 + 0.9 * img[..., :3]
    img[..., 3] = 1.0
    return img


RECT_96x64 = (0.25, 0.125, 0.75, 0.875)
HUE_THETA = [(0.0, 0.0), (0.3, 0.8), (-1.2, float(np.float32(np.pi / 2 - 0.05)))]
