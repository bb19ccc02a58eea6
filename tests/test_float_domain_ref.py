"""Non-finite and extreme texels stay local: the statement, its exclusion zones, and the oracle under it.

A float frame from a real pipeline carries Inf speculars, the odd NaN, values at the top of f16 and
signed (scRGB) data. A sampler reads a bounded neighbourhood of source texels per output pixel, so a
bad texel may change only the outputs that read it:

    out(B) == out(A), bit for bit, at every output pixel outside the exclusion zone of the bad texels

where B is A with six texels replaced (BAD_CODES at bad_positions). The zone of a bad texel is measured
in source texels from the output pixel's centre, (o + 0.5) * src / dst - 0.5:

    polar       a disc of radius `radius * max(1, src / dst) + 1`, `radius` from
                orc.filter_generate_polar (the + 1: the taps the reference calls "maybe skippable")
    separable   |d| < row_size / 2 + 1 along the filtered axis; across it |d| < 1.5: the pass reads its
                own row, and a bilinear fetch with a weight of exactly 0 (the LIN variants) its
                neighbour -- 0 x Inf is NaN there in the reference as well
    the simple samplers (bicubic, hermite, gaussian, oversample, bilinear, nearest)
                a square of half-width 3
    deband      a disc of radius `radius * iterations + 1` (iteration i reaches i * radius)

This file holds the geometries (GEOMETRIES: sampler, sizes, where the bad texels go, the zone) that
tests/test_gpu_float_domain.py runs the kernels on, and checks on the CPU, for every one of them,
  * that at least 85 % of the output pixels lie outside every zone (so the GPU statement compares the
    bulk of each frame), and
  * that the oracle itself obeys the statement with these zones: they are a property of the
    reference, not of the code under test.
"""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.usefixtures("built")

MIN_SHARE = 0.85

# +Inf, -Inf, NaN, +65504, -65504, a second (signalling, negative) NaN -- as f16 codes
BAD_CODES = np.array([0x7c00, 0xfc00, 0x7e00, 0x7bff, 0xfbff, 0xfd55], np.uint16)
FINITE_BAD = (3, 4)     # the two that are finite on purpose


def noise_f16(w, h, seed):
    """finite f16 noise in [0, 1), four components"""
    return np.random.default_rng(seed).random((h, w, 4), dtype=np.float32).astype(np.float16)


def bad_positions(w, h, seam=(63, 31), interior=None, edges=None):
    """(x, y) of the six bad texels, in the order of BAD_CODES: the source corner, the last column, the
    last row, a tile interior, and the two texels either side of a workgroup-tile seam (`seam`: the
    last column and row of the first tile). `edges`: the rows / columns of the last-column and last-row
    texels where the default (a third of the way along) is not wanted."""
    sx, sy = seam
    ey, ex = edges if edges is not None else (h // 3, w // 3)
    pos = [(0, 0), (w - 1, ey), (ex, h - 1), interior or (sx // 2, sy // 2), (sx, sy), (sx + 1, sy + 1)]
    assert all(0 <= x < w and 0 <= y < h for x, y in pos) and len(set(pos)) == 6, pos
    return pos


def poison(img, positions, which=range(6), alpha=False):
    """`img` (f16 or f32, h x w x 4) with the bad texels `which` written into RGB (and alpha)"""
    out = img.copy()
    for i in which:
        x, y = positions[i]
        if out.dtype == np.float16:
            # (the codes themselves: the signalling NaN stays one)
            out.view(np.uint16)[y, x, :4 if alpha else 3] = BAD_CODES[i]
        else:
            out[y, x, :4 if alpha else 3] = BAD_CODES.view(np.float16)[i].astype(out.dtype)
    return out


def centres(n_out, span, origin=0.0):
    """the output pixels' centres in source texel coordinates"""
    return origin + (np.arange(n_out) + 0.5) * (span / n_out) - 0.5


def compared(geo, which=range(6)):
    """(dh, dw) mask of the output pixels outside the zone of every bad texel in `which`"""
    x0, y0, x1, y1 = geo["rect"]
    cx, cy = centres(geo["dw"], x1 - x0, x0), centres(geo["dh"], y1 - y0, y0)
    keep = np.ones((geo["dh"], geo["dw"]), bool)
    zone = geo["zone"]
    for i in which:
        bx, by = geo["bad"][i]
        dx, dy = np.abs(cx - bx)[None, :], np.abs(cy - by)[:, None]
        if zone[0] == "disc":
            keep &= ~(np.hypot(dx, dy) < zone[1])
        else:
            keep &= ~((dx < zone[1]) & (dy < zone[2]))
    return keep


def same_bits(a, b):
    """elementwise: the same bit pattern (a NaN equals itself, -0 differs from +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.view(u) == b.view(u)


# ---- the oracle's form of each sampler ---------------------------------------------------------------
def polar_radius():
    return orc.filter_generate_polar(orc.ewa_lanczos())[1]


def oracle_polar(geo, img):
    x0, y0, x1, y1 = geo["rect"]
    inv = max(1.0, (x1 - x0) / geo["dw"])
    w, radius, rz = orc.filter_generate_polar(orc.ewa_lanczos(blur=inv if inv > 1.0 else 0.0))
    rect = None if geo["rect"] == (0, 0, geo["sw"], geo["sh"]) else geo["rect"]
    return orc.sample_polar(img.astype(np.float32), w, radius, rz, geo["dw"], geo["dh"], rect=rect,
                            gather_order=not radius < 6.0, mask=geo.get("mask", 0x7))


def bicubic(blur=0.0):
    f = orc.mitchell(blur)
    f.kparams[0], f.kparams[1] = 1.0, 0.0
    return f


ORTHO = {"lanczos": (orc.lanczos, False), "mitchell": (orc.mitchell, False), "bicubic": (bicubic, True)}


def ortho_rows(name, direction, new, sw, sh):
    """the weights of one separable pass as uploaded -> (rows, row_size, use_linear)"""
    ratio = float(np.float32(new / (sw if direction == 0 else sh)))
    inv_scale = float(np.float32(1.0 / ratio))
    rows, n, radius, rz = orc.filter_generate_ortho(ORTHO[name][0](blur=inv_scale if inv_scale > 1.0 else 0.0))
    use_linear = radius == rz
    assert use_linear == ORTHO[name][1], (name, radius, rz)
    return orc.ortho_lut_rows(rows, n, use_linear), n, use_linear


def oracle_ortho(geo, img):
    name, direction = geo["filter"], geo["dir"]
    new = geo["dw"] if direction == 0 else geo["dh"]
    rows, n, use_linear = ortho_rows(name, direction, new, geo["sw"], geo["sh"])
    return orc.sample_ortho(img.astype(np.float32), rows, n, direction, geo["dw"], geo["dh"],
                            use_linear=use_linear, mask=0xF)


def oracle_two_pass(geo, img):
    """the renderer's composition: the vertical pass into an rgba16hf intermediate, then the horizontal"""
    rows, n, _ = ortho_rows("lanczos", 1, geo["dh"], geo["sw"], geo["sh"])
    p1 = orc.op_quant_f16(orc.sample_ortho(img.astype(np.float32), rows, n, 1, geo["sw"], geo["dh"]))
    return orc.sample_ortho(p1, rows, n, 0, geo["dw"], geo["dh"])


SIMPLE = {"nearest": orc.S_NEAREST, "bilinear": orc.S_BILINEAR, "bicubic": orc.S_BICUBIC,
          "hermite": orc.S_HERMITE, "gaussian": orc.S_GAUSSIAN, "oversample": orc.S_OVERSAMPLE}


def oracle_simple(geo, img):
    return orc.sample_simple(img.astype(np.float32), SIMPLE[geo["kind"]], geo["dw"], geo["dh"])


def oracle_deband(geo, img, seed=2):
    return orc.deband(img.astype(np.float32), geo["dw"], geo["dh"], mask=0x7, frame_index=seed, **geo["params"])


def deband_source(w, h, seed):
    """noise of a few thousandths around mid grey: the debanding threshold accepts most averages"""
    rng = np.random.default_rng(seed)
    img = (0.5 + 0.004 * rng.random((h, w, 4), dtype=np.float32)).astype(np.float16)
    img[..., 3] = 1.0
    return img


# ---- the geometries -----------------------------------------------------------------------------------
def _geo(sampler, oracle, sw, sh, dw, dh, zone, rect=None, seed=21, source=noise_f16, **kw):
    bad_kw = {k: kw.pop(k) for k in ("seam", "interior", "edges") if k in kw}
    rect = rect or (0, 0, sw, sh)
    g = dict(sampler=sampler, oracle=oracle, sw=sw, sh=sh, dw=dw, dh=dh, zone=zone, rect=rect, seed=seed,
             source=source, **kw)
    g["bad"] = bad_positions(sw, sh, **bad_kw)
    return g


def _build():
    r = polar_radius()
    G = {}
    # polar 2x (k_polar_pp, k_polar_mx, k_polar_mxp): the workgroup tile is 8 * WTC = 64 source
    # columns by 32 source rows
    for sw, sh in ((96, 64), (130, 77)):
        G["polar-2x-%dx%d" % (sw, sh)] = _geo("polar", oracle_polar, sw, sh, 2 * sw, 2 * sh, ("disc", r + 1))
        G["polar-2x-alpha-%dx%d" % (sw, sh)] = _geo("polar", oracle_polar, sw, sh, 2 * sw, 2 * sh, ("disc", r + 1),
                                                    mask=0xF)
    # polar 3x, 4x, 3 : 2 (k_polar_mxr)
    for name, ratio in (("3x", 3), ("4x", 4), ("3:2", 1.5)):
        G["polar-%s-80x48" % name] = _geo("polar", oracle_polar, 80, 48, int(80 * ratio), int(48 * ratio),
                                          ("disc", r + 1), seam=(43, 23))
    # polar 2 : 1 (k_polar_mxd): a workgroup tile is 64 x 32 outputs = 128 x 64 source texels
    for dw, dh in ((128, 64), (200, 90)):
        G["polar-2:1-%dx%d" % (dw, dh)] = _geo("polar", oracle_polar, 2 * dw, 2 * dh, dw, dh,
                                               ("disc", 2 * r + 1), seam=(127, 63))
    # ... from a source rectangle that starts inside the plane at an odd offset: the bad texels are
    # placed on the rectangle's own corner, last column and last row (the texels beyond it are read
    # as they are: no clamp at the rectangle) and on the seam of its tiles
    x0, y0 = 7, 13
    g = _geo("polar", oracle_polar, 440, 220, 200, 90, ("disc", 2 * r + 1), rect=(x0, y0, x0 + 400, y0 + 180))
    g["bad"] = [(x0, y0), (x0 + 399, y0 + 60), (x0 + 133, y0 + 179), (x0 + 63, y0 + 31),
                (x0 + 127, y0 + 63), (x0 + 128, y0 + 64)]
    G["polar-2:1-crop-200x90"] = g
    # separable, 80 x 60, both axes, up and down
    for name in ORTHO:
        for direction, new in ((0, 160), (1, 120), (0, 37), (1, 29)):
            dw, dh = (new, 60) if direction == 0 else (80, new)
            n = ortho_rows(name, direction, new, 80, 60)[1]
            half = n / 2 + 1
            zone = ("rect", half, 1.5) if direction == 0 else ("rect", 1.5, half)
            G["ortho-%s-%s%d" % (name, "xy"[direction], new)] = _geo(
                "ortho", oracle_ortho, 80, 60, dw, dh, zone, filter=name, dir=direction, seam=(47, 31))
    n = ortho_rows("lanczos", 0, 128, 64, 48)[1]
    G["ortho-two-pass-64x48"] = _geo("two_pass", oracle_two_pass, 64, 48, 128, 96, ("rect", n / 2 + 1, n / 2 + 1),
                                     seam=(39, 23))
    # the simple samplers, 40 x 30 -> 100 x 75
    for kind in SIMPLE:
        G["simple-%s" % kind] = _geo("simple", oracle_simple, 40, 30, 100, 75, ("rect", 3.0, 3.0), kind=kind,
                                     seam=(23, 15))
    # deband. A zone of radius 17 (25) is a large part of a small frame: the edge texels sit next
    # to one corner and the interior ones next to each other so that the zones overlap, and the
    # second case takes a frame of twice the size -- six discs of radius 25 do not leave 85 % of
    # 128 x 96 pixels whatever their places (one interior disc alone is 16 % of it)
    G["deband-default-128x96"] = _geo("deband", oracle_deband, 128, 96, 128, 96, ("disc", 16.0 * 1 + 1),
                                      params=dict(), source=deband_source, seam=(63, 31), interior=(61, 30),
                                      edges=(92, 124))
    G["deband-it3-r8-256x192"] = _geo("deband", oracle_deband, 256, 192, 256, 192, ("disc", 8.0 * 3 + 1),
                                      params=dict(iterations=3, radius=8.0), source=deband_source,
                                      seam=(127, 63), interior=(125, 62), edges=(188, 252))
    return G


_GEOMETRIES = None


def geometries():
    global _GEOMETRIES
    if _GEOMETRIES is None:
        _GEOMETRIES = _build()
    return _GEOMETRIES


# (the names are listed here so that both files can parametrise over them before the oracle is built)
NAMES = (["polar-2x-96x64", "polar-2x-130x77", "polar-2x-alpha-96x64", "polar-2x-alpha-130x77"] +
         ["polar-%s-80x48" % r for r in ("3x", "4x", "3:2")] +
         ["polar-2:1-128x64", "polar-2:1-200x90", "polar-2:1-crop-200x90"] +
         ["ortho-%s-%s" % (f, d) for f in ("lanczos", "mitchell", "bicubic") for d in ("x160", "y120", "x37", "y29")] +
         ["ortho-two-pass-64x48"] +
         ["simple-%s" % k for k in ("nearest", "bilinear", "bicubic", "hermite", "gaussian", "oversample")] +
         ["deband-default-128x96", "deband-it3-r8-256x192"])


def frames(geo, alpha=None):
    """A, B (all six bad texels) and F (the two finite ones) of a geometry"""
    a = geo["source"](geo["sw"], geo["sh"], geo["seed"])
    alpha = geo.get("mask", 0x7) == 0xF if alpha is None else alpha
    return a, poison(a, geo["bad"], alpha=alpha), poison(a, geo["bad"], which=FINITE_BAD, alpha=alpha)


def test_the_names_are_the_geometries():
    assert sorted(NAMES) == sorted(geometries())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_obeys_the_zone_and_the_bulk_is_compared(name):
    geo = geometries()[name]
    keep = compared(geo)
    share = keep.mean()
    a, b, f = frames(geo)
    assert not np.isfinite(b.astype(np.float32)).all() and np.isfinite(f.astype(np.float32)).all()
    oa, ob, of = (geo["oracle"](geo, x) for x in (a, b, f))
    nch = 4 if geo.get("mask", 0x7) == 0xF or geo["sampler"] in ("ortho", "two_pass", "simple") else 3
    diff = ~same_bits(oa[..., :nch], ob[..., :nch]).all(axis=-1)
    diff_f = ~same_bits(oa[..., :nch], of[..., :nch]).all(axis=-1)
    print("%s: %.1f %% of %d x %d compared; the oracle changed %d pixels inside the zones, %d outside "
          "(finite texels only: %d, %d)" % (name, 100 * share, geo["dw"], geo["dh"], (diff & ~keep).sum(),
                                            (diff & keep).sum(), (diff_f & ~compared(geo, FINITE_BAD)).sum(),
                                            (diff_f & compared(geo, FINITE_BAD)).sum()))
    assert share >= MIN_SHARE, share
    assert np.isfinite(oa[..., :nch]).all()
    assert not (diff & keep).any(), np.argwhere(diff & keep)[:8]
    assert not (diff_f & compared(geo, FINITE_BAD)).any()
    # the zones are not vacuous: the bad texels do change the oracle's frame
    assert (diff & ~keep).sum() > 0
