"""What the ICC tests hold the library to: LittleCMS 2 called through ctypes (profiles made on
the spot, the approximation profile and the 3D tables rebuilt from an object's public members)
and numpy models of the two ops. Nothing here comes from the library under test except what a
test passes in."""
import ctypes as C

import numpy as np

try:
    CMS = C.CDLL("liblcms2.so.2")
except OSError:
    CMS = None

TYPE_RGB_16 = (4 << 16) | (3 << 3) | 2
TYPE_RGBA_16 = (4 << 16) | (1 << 7) | (3 << 3) | 2
FLAGS_LUT = 0x2000 | 0x0040 | 0x0100    # black point compensation, no cache, no optimisation
KNEE = 16 << 8

D65 = (0.3127, 0.3290)
BT709 = ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))
BT2020 = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))


class XyY(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("Y", C.c_double)]


class XyYTriple(C.Structure):
    _fields_ = [("Red", XyY), ("Green", XyY), ("Blue", XyY)]


if CMS is not None:
    vp = C.c_void_p
    for name, res, args in (
        ("cmsCreate_sRGBProfile", vp, []),
        ("cmsCreateLab4Profile", vp, [vp]),
        ("cmsBuildGamma", vp, [vp, C.c_double]),
        ("cmsBuildParametricToneCurve", vp, [vp, C.c_int32, C.POINTER(C.c_double)]),
        ("cmsFreeToneCurve", None, [vp]),
        ("cmsCreateRGBProfile", vp, [C.POINTER(XyY), C.POINTER(XyYTriple), C.POINTER(vp)]),
        ("cmsSaveProfileToMem", C.c_int, [vp, vp, C.POINTER(C.c_uint32)]),
        ("cmsOpenProfileFromMem", vp, [vp, C.c_uint32]),
        ("cmsCloseProfile", C.c_int, [vp]),
        ("cmsSetHeaderRenderingIntent", None, [vp, C.c_uint32]),
        ("cmsSetProfileVersion", None, [vp, C.c_double]),
        ("cmsCreateTransform", vp, [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32]),
        ("cmsDoTransform", None, [vp, vp, vp, C.c_uint32]),
        ("cmsDeleteTransform", None, [vp]),
    ):
        f = getattr(CMS, name)
        f.restype, f.argtypes = res, args


def _save(h):
    n = C.c_uint32(0)
    assert CMS.cmsSaveProfileToMem(h, None, C.byref(n))
    buf = C.create_string_buffer(n.value)
    assert CMS.cmsSaveProfileToMem(h, buf, C.byref(n))
    CMS.cmsCloseProfile(h)
    return buf.raw[:n.value]


def _rgb_profile(white, prim, curve):
    wp = XyY(white[0], white[1], 1.0)
    tri = XyYTriple(*(XyY(x, y, 1.0) for x, y in prim))
    h = CMS.cmsCreateRGBProfile(C.byref(wp), C.byref(tri), (C.c_void_p * 3)(curve, curve, curve))
    CMS.cmsFreeToneCurve(curve)
    assert h
    return h


def srgb_profile():
    return _save(CMS.cmsCreate_sRGBProfile())


def gamma_profile(prim, gamma, white=D65):
    return _save(_rgb_profile(white, prim, CMS.cmsBuildGamma(None, gamma)))


def lab_profile():
    return _save(CMS.cmsCreateLab4Profile(None))


def approx_constants(gamma, min_luma, max_luma):
    """(a, b, scale) of Y = scale * (a X + b)^gamma, in float32 like the library"""
    f = np.float32
    b = np.power(f(min_luma) / f(max_luma), f(1.0) / f(gamma), dtype=np.float32)
    return f(1.0) - b, b, f(max_luma) / f(203.0)


def expected_lut(profile_bytes, prim_xy, white_xy, gamma, min_luma, max_luma, intent, size,
                 encode, force_bpc):
    """The table lcms gives for profile -> approximation (decode) or back, uint16
    [size_b][size_g][size_r][4]. prim_xy / white_xy: the containing primaries."""
    a, b, _ = approx_constants(gamma, min_luma, max_luma)
    pars = (C.c_double * 3)(float(np.float32(gamma)), float(a), float(b))
    approx = _rgb_profile(white_xy, prim_xy, CMS.cmsBuildParametricToneCurve(None, 2, pars))
    CMS.cmsSetHeaderRenderingIntent(approx, intent)
    CMS.cmsSetProfileVersion(approx, 2.2)
    buf = C.create_string_buffer(profile_bytes, len(profile_bytes))
    prof = CMS.cmsOpenProfileFromMem(buf, len(profile_bytes))
    assert prof
    src, dst = (approx, prof) if encode else (prof, approx)
    tf = CMS.cmsCreateTransform(src, TYPE_RGB_16, dst, TYPE_RGBA_16, intent, FLAGS_LUT)
    assert tf
    s_r, s_g, s_b = size
    grid = np.zeros((s_b, s_g, s_r, 3), np.uint16)
    grid[..., 0] = (np.arange(s_r) * 65535 // (s_r - 1))[None, None, :]
    grid[..., 1] = (np.arange(s_g) * 65535 // (s_g - 1))[None, :, None]
    grid[..., 2] = (np.arange(s_b) * 65535 // (s_b - 1))[:, None, None]
    out = np.zeros((s_b, s_g, s_r, 4), np.uint16)
    CMS.cmsDoTransform(tf, grid.ctypes.data, out.ctypes.data, s_r * s_g * s_b)
    CMS.cmsDeleteTransform(tf)
    CMS.cmsCloseProfile(prof)
    CMS.cmsCloseProfile(approx)
    if force_bpc:
        # below the knee the output is pulled towards the input's grey level, row by row
        g32 = grid.astype(np.int64)
        s = (2 * g32[..., 1] + g32[..., 2] + g32[..., 0]) >> 2
        fix = (g32[..., 1] < KNEE) & (s < KNEE)
        rgb = out[..., :3].astype(np.int64)
        fixed = (s[..., None] * rgb + (KNEE - s[..., None]) * s[..., None]) >> 12
        out[..., :3] = np.where(fix[..., None], fixed, rgb).astype(np.uint16)
    return out


# ---- the ops ------------------------------------------------------------------------------

def tetra_lookup(table, rgb, ftype):
    """Tetrahedral interpolation (the six-tetrahedron rule of the reference's lut.c:762-809) of
    `table` (uint16 [b][g][r][4]) at rgb in [0, 1] (clamped), in `ftype` arithmetic, summed in the
    order w0 t0 + w1 t1 + w2 t2 + w3 t3."""
    f = ftype
    size = np.array(table.shape[2::-1])                         # r, g, b
    pos = np.clip(rgb.astype(f), f(0), f(1)) * (size - 1).astype(f)
    base = np.floor(pos)
    fp = (pos - base).astype(f)
    v0 = base.astype(np.int64)
    v3 = np.ceil(pos).astype(np.int64)
    v1, v2 = v0.copy(), v3.copy()
    s = fp.copy()
    ge = lambda i, j: fp[..., i] >= fp[..., j]
    cxy, cyz, czx = ge(0, 1), ge(1, 2), ge(2, 0)
    conds = {(0, 1): cxy, (1, 0): ~cxy, (1, 2): cyz, (2, 1): ~cyz, (2, 0): czx, (0, 2): ~czx}
    for X, Y, Z in ((0, 1, 2), (0, 2, 1), (2, 0, 1), (2, 1, 0), (1, 2, 0), (1, 0, 2)):
        m = conds[(X, Y)] & conds[(Y, Z)]
        for k, src in enumerate((X, Y, Z)):
            s[..., k] = np.where(m, fp[..., src], s[..., k])
        v1[..., X] = np.where(m, v3[..., X], v1[..., X])
        v2[..., Z] = np.where(m, v0[..., Z], v2[..., Z])
    tex = lambda v: (table[v[..., 2], v[..., 1], v[..., 0], :3].astype(f) / f(65535))
    w = [f(1) - s[..., 0], s[..., 0] - s[..., 1], s[..., 1] - s[..., 2], s[..., 2]]
    t = [tex(v0), tex(v1), tex(v2), tex(v3)]
    acc = w[0][..., None] * t[0]
    for k in (1, 2, 3):
        acc = (acc + w[k][..., None] * t[k]).astype(f)
    return acc


def _pow(x, y, f):
    if f is np.float64:
        return np.power(x, y)
    # the kernel's pow: exp2(y * log2(x)) in single precision
    with np.errstate(divide="ignore"):
        return np.exp2((f(y) * np.log2(x.astype(f))).astype(f)).astype(f)


def decode_model(table, rgb, a, b, gamma, scale, ftype=np.float64):
    f = ftype
    x = tetra_lookup(table, rgb, f)
    x = (f(a) * x).astype(f) + f(b)
    return (f(scale) * _pow(x.astype(f), gamma, f)).astype(f)


def encode_model(table, rgb, a, b, gamma, scale, ftype=np.float64):
    """the op's constants are the float32 reciprocals the library records"""
    f, s = ftype, np.float32
    k = [s(1) / s(scale), s(1) / s(gamma), s(1) / s(a), s(b) / s(a)]
    x = (f(k[0]) * np.maximum(rgb.astype(f), f(0))).astype(f)
    x = (f(k[2]) * _pow(x, k[1], f)).astype(f) - f(k[3])
    return tetra_lookup(table, x.astype(f), f)
