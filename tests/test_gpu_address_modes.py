"""Every sampler that reads many taps per pixel, under PL_TEX_ADDRESS_REPEAT / MIRROR and with source
rects that reach outside the texture, against the CPU oracle (whose own wrapping has a second
opinion in tests/test_second_opinion.py: the periods written out).

These are the kernels whose addressing at the borders is hand-written: the separable ones (k_ortho:
plh_wrap per tap; k_ortho_fast: clamp or ONE reflection, shared-window loads, six plane formats
assembled from bytes), the polar ones (an LDS tile staged through plh_wrap), the four-tap family and
debanding. Bars as for clamped addressing: bit-exact where the path has no transcendental
(test_gpu_ortho_deband.py, test_gpu_sampling.py), gaussian within one code of 16 bits, debanding
>= 99.9 % identical pixels and the rest within threshold + grain.

Every separable case also reads the launcher's trace and asserts WHICH kernel ran: repeat on k_ortho,
clamp on k_ortho_fast, mirror on k_ortho_fast exactly where plh_ortho_one_reflection
(tests/test_ortho_mirror_guard.py) says one reflection reaches every tap -- a fall-back would
otherwise pass without touching the code the case is about."""
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util
from test_gpu_metric import bicubic, lowpass_feature_map
from test_gpu_ortho_deband import banded
from test_gpu_sampling import KINDS, polar_oracle, polar_pipeline, run_simple

pytestmark = pytest.mark.gpu

F = np.float32
CLAMP, REPEAT, MIRROR = pl.ADDRESS_CLAMP, pl.ADDRESS_REPEAT, pl.ADDRESS_MIRROR
MODE_NAMES = {CLAMP: "clamp", REPEAT: "repeat", MIRROR: "mirror"}


def ends(kind, n, which):
    """one axis (which: 0 = x, 1 = y) of the rect kinds of an n-texel axis"""
    return {"inside": ((3.25, n - 3.25), (1.5, n - 2.5))[which],
            "slight": ((-4.0, n + 5.0), (-3.0, n + 2.0))[which],
            "far": (-0.85 * n, 1.85 * n),                   # inside the window the old guard allowed
            "periods": ((-2.5 * n, 3.25 * n), (-2.25 * n, 3.5 * n))[which]}[kind]


def rect2(kind, w, h, flip=False):
    (x0, x1), (y0, y1) = ends(kind, w, 0), ends(kind, h, 1)
    return (x1, y1, x0, y0) if flip else (x0, y0, x1, y1)


def modes_for(kind):
    # (clamp wherever the rect leaves the texture: not covered for these samplers either)
    return (REPEAT, MIRROR) if kind == "inside" else (REPEAT, MIRROR, CLAMP)


def random_tex(fmt, w, h, seed):
    dt, nc = pl._FMT_DTYPES[fmt]
    rng = np.random.default_rng(seed)
    if np.issubdtype(dt, np.integer):
        return rng.integers(0, np.iinfo(dt).max + 1, (h, w, nc)).astype(dt)
    return rng.random((h, w, nc)).astype(dt)


# ---- separable ---------------------------------------------------------------------------------

def spline64(blur=0.0):
    return orc.OrcFilter(kernel=orc.K["spline64"], window=orc.K["none"], kradius=4.0, wradius=1.0,
                         resizable=0, radius=4.0, blur=blur)


# name: (the oracle's filter, ratio, taps -- a downscale's depend on the rounded output size --, linear trick)
SEP = {
    "mitchell": (orc.mitchell, 2.0, 4, False),
    "lanczos": (orc.lanczos, 2.0, 6, False),
    "spline64": (spline64, 2.0, 8, False),
    "lanczos_down": (orc.lanczos, 0.5, (12, 14), False),    # the run-time NT = 16 variant
    "bilinear": (orc.triangle, 2.0, 2, True),
    "bicubic_down": (bicubic, 0.5, (8, 10), True),          # the low-pass's configuration
}


def sep_rect(kind, flip, w, h, d):
    """the rect kind along the filtered axis; across it the same kind where its ends are whole texels
    (the other axis is copied 1 : 1), else the whole texture"""
    n_al, n_ac = (h, w) if d else (w, h)
    al = ends(kind, n_al, d)
    ac = ends(kind, n_ac, 1 - d) if kind == "slight" else (0.0, float(n_ac))
    (x0, x1), (y0, y1) = (ac, al) if d else (al, ac)
    return (x1, y1, x0, y0) if flip else (x0, y0, x1, y1)


def one_reflection(w, h, n, rect, d):
    fn = pl.lib().plh_test_ortho_one_reflection
    sx, sy = F(1.0 / w), F(1.0 / h)         # sh_bind (shaders.c)
    rect = util.bound_rect(rect)
    x0, y0, x1, y1 = sx * F(rect[0]), sy * F(rect[1]), sx * F(rect[2]), sy * F(rect[3])
    pos = np.array([x0, y0, x1, y0, x0, y1, x1, y1], F)
    return bool(fn(h if d else w, w if d else h, n, pos.ctypes.data_as(C.POINTER(C.c_float)), d))


def sep_filter(name, rect, d):
    """-> the output size, the ratio as setup_src has it, the weight rows as uploaded, the tap count"""
    mk, ratio, taps, lin = SEP[name]
    # (setup_src: the rect's size in float32; float ratio = out / |src|)
    al = float(abs(F(rect[3]) - F(rect[1])) if d else abs(F(rect[2]) - F(rect[0])))
    ac = abs(rect[2] - rect[0]) if d else abs(rect[3] - rect[1])
    assert ac == int(ac)
    new = max(1, int(round(al * ratio)))
    r = float(F(new / al))
    inv = float(F(1.0 / r))
    rows, n, radius, rz = orc.filter_generate_ortho(mk(blur=inv if inv > 1.0 else 0.0))
    assert n in (taps if isinstance(taps, tuple) else (taps,)) and (radius == rz) == lin, (n, radius, rz)
    return ((int(ac), new) if d else (new, int(ac))), r, orc.ortho_lut_rows(rows, n, lin), n


def separable_reference(src, sfmt, name, d, rect, mode, dfmt, antiring=0.0):
    """-> the oracle's frame as `dfmt` stores it, the tap count, the output size"""
    lin = SEP[name][3]
    nc = src.shape[2]
    (ow, oh), r, rows, n = sep_filter(name, rect, d)
    use_ar = antiring > 0 and r > 1 and not lin
    ref = orc.sample_ortho(orc.tex_decode(src, sfmt), rows, n, d, ow, oh, rect=util.bound_rect(rect), use_linear=lin,
                           use_ar=use_ar, antiring=antiring, mask=(1 << nc) - 1, address_mode=mode)
    if dfmt.endswith("32f"):
        ref = ref[..., :pl._FMT_DTYPES[dfmt][1]]
    else:
        ref = orc.tex_decode(orc.tex_encode(ref, dfmt), dfmt)
    return ref, n, ow, oh


def check_separable(gpu, capfd, src, sfmt, name, d, rect, mode, dfmt=None, antiring=0.0):
    """one pass on the GPU, with k_ortho_fast allowed and without, against ONE oracle frame; and the
    kernel that took each launch"""
    h, w, nc = src.shape
    dfmt = dfmt or {1: "r32f", 2: "rg32f", 4: "rgba32f"}[nc]
    ref, n, ow, oh = separable_reference(src, sfmt, name, d, rect, mode, dfmt, antiring)
    cfg = pl.filter_config(name.split("_")[0])
    for fast in ("1", "0"):
        t = gpu.tex_create(w, h, sfmt, src)
        dst = gpu.tex_create(ow, oh, dfmt)
        lut = pl.ShaderObj()
        with util.kernel_trace(capfd, PL_HIP_ORTHO_FAST=fast) as kernels:
            sh = gpu.begin()
            assert sh.sample_ortho(t, cfg, lut, antiring=antiring, rect=rect, new_w=ow, new_h=oh,
                                   components=nc, address_mode=mode), gpu.messages[-3:]
            assert sh.finish(dst), gpu.messages[-3:]
            got = dst.download()
        t.destroy(); dst.destroy(); lut.destroy()
        what = (name, sfmt, (w, h), d, rect, MODE_NAMES[mode], "PL_HIP_ORTHO_FAST=" + fast, kernels)
        if mode == REPEAT or fast == "0":
            want = "k_ortho"
        elif mode == CLAMP:
            want = "k_ortho_fast"
        else:
            want = "k_ortho_fast" if one_reflection(w, h, n, rect, d) else "k_ortho"
        assert kernels == [want], (want,) + what
        assert got.shape == ref.shape, (got.shape, ref.shape)
        assert np.array_equal(got, ref), what + (float(np.abs(got.astype(F) - ref).max()),
                                                 int((got != ref).any(axis=2).sum()))


ALL_RECTS = [(k, f) for k in ("inside", "slight", "far", "periods") for f in (False, True)]
SOME_RECTS = [("inside", False), ("slight", True), ("far", False), ("periods", True)]


def sep_cases():
    out = []
    for name in ("mitchell", "lanczos", "spline64", "lanczos_down", "bilinear"):
        for kind, flip in (ALL_RECTS if name in ("mitchell", "lanczos") else SOME_RECTS):
            for mode in modes_for(kind):
                for d in (0, 1):
                    out.append(("rgba16", (40, 24), name, kind, flip, mode, d))
    # below 2 * row_size on one axis or both: mirror must fall to k_ortho, clamp stays
    for name in ("lanczos", "spline64"):
        for kind in ("inside", "slight", "far"):
            for mode in modes_for(kind):
                for d in (0, 1):
                    out.append(("rgba16", (13, 9), name, kind, False, mode, d))
    # planes: odd widths, so that rows end inside a 16-byte piece
    for fmt in ("r8", "rg8", "r16", "rg16", "r16hf", "rg16hf"):
        for kind, flip in (("inside", False), ("slight", True), ("far", False)):
            for mode in modes_for(kind):
                for d in (0, 1):
                    out.append((fmt, (37, 21), "lanczos", kind, flip, mode, d))
    for kind, flip in (("inside", False), ("slight", False), ("far", True)):
        for mode in modes_for(kind):
            for d in (0, 1):
                out.append(("r16hf", (37, 21), "bicubic_down", kind, flip, mode, d))
                out.append(("r8", (37, 21), "mitchell", kind, flip, mode, d))
                out.append(("rg16", (37, 21), "spline64", kind, flip, mode, d))
    return out


def sep_id(c):
    fmt, (w, h), name, kind, flip, mode, d = c
    return "%s-%dx%d-%s-%s%s-%s-%s" % (fmt, w, h, name, kind, "-flipped" if flip else "", MODE_NAMES[mode], "hv"[d])


@pytest.mark.parametrize("case", sep_cases(), ids=sep_id)
def test_separable(gpu, capfd, case):
    fmt, (w, h), name, kind, flip, mode, d = case
    src = random_tex(fmt, w, h, seed=w + 3 * d)
    check_separable(gpu, capfd, src, fmt, name, d, sep_rect(kind, flip, w, h, d), mode)


def test_mirror_keeps_the_fast_kernel_where_one_reflection_reaches():
    """(no GPU needed, but it is about the cases above) Which of them the fast kernel keeps under
    mirror: rects inside or slightly outside a texture of two windows or more, the low-pass's
    configuration among them -- and, of the far-outside ones the old rule admitted, only those whose
    taps one reflection still reaches (four taps on 40 texels; not six or eight on 24 or 21)."""
    kept = set()
    for fmt, size, name, kind, flip, mode, d in sep_cases():
        rect = sep_rect(kind, flip, *size, d)
        if mode == MIRROR and one_reflection(*size, sep_filter(name, rect, d)[3], rect, d):
            kept.add((size, name, kind, d))
    for d in (0, 1):
        assert ((40, 24), "lanczos", "inside", d) in kept and ((40, 24), "lanczos", "slight", d) in kept
        assert ((37, 21), "bicubic_down", "inside", d) in kept
    assert ((40, 24), "mitchell", "far", 0) in kept
    assert ((40, 24), "lanczos", "far", 1) not in kept and ((37, 21), "lanczos", "far", 1) not in kept
    assert ((40, 24), "spline64", "far", 1) not in kept
    assert not any(k[2] == "periods" for k in kept)
    assert not any(k[0] == (13, 9) and k[1] == "spline64" for k in kept)


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("mode", [REPEAT, MIRROR])
def test_separable_half_float_target_and_antiringing(gpu, capfd, d, mode):
    src = util.chirp_rgba16(40, 24)
    check_separable(gpu, capfd, src, "rgba16", "lanczos", d, sep_rect("slight", False, 40, 24, d), mode,
                    dfmt="rgba16hf")
    check_separable(gpu, capfd, src, "rgba16", "lanczos", d, sep_rect("slight", True, 40, 24, d), mode,
                    antiring=0.8)
    check_separable(gpu, capfd, src, "rgba16", "mitchell", d, sep_rect("far", False, 40, 24, d), mode,
                    antiring=0.8)


# ---- the contrast-recovery low-pass, on its own ---------------------------------------------------

@pytest.mark.parametrize("size", [((40, 24), (20, 12)), ((257, 131), (73, 37))])
def test_mirrored_lowpass_two_passes(gpu, capfd, size):
    """get_feature_map's two passes (renderer.c:2089-2154) recorded by hand: bicubic, MIRROR, a
    vertical pass of an r16hf plane into an r16hf intermediate, then the horizontal one -- against the
    oracle's (test_gpu_metric.py: lowpass_feature_map), bit for bit, on k_ortho_fast and on k_ortho.
    (The fused kernel is reachable through the renderer only;
    test_gpu_contrast_recovery.py::test_fused_lowpass_equals_the_two_passes ties it to these two.)"""
    (w, h), (mw, mh) = size
    plane = random_tex("r16hf", w, h, seed=31)
    ref = lowpass_feature_map(orc.tex_decode(plane, "r16hf"), mw, mh)[..., :1]
    cfg = pl.filter_config("bicubic")
    for fast in ("1", "0"):
        t = gpu.tex_create(w, h, "r16hf", plane)
        mid = gpu.tex_create(w, mh, "r16hf")
        dst = gpu.tex_create(mw, mh, "r16hf")
        lut_v, lut_h = pl.ShaderObj(), pl.ShaderObj()
        with util.kernel_trace(capfd, PL_HIP_ORTHO_FAST=fast) as kernels:
            a = gpu.begin()
            assert a.sample_ortho(t, cfg, lut_v, new_w=w, new_h=mh, components=1, address_mode=MIRROR)
            assert a.finish(mid), gpu.messages[-3:]
            b = gpu.begin()
            assert b.sample_ortho(mid, cfg, lut_h, new_w=mw, new_h=mh, components=1, address_mode=MIRROR)
            assert b.finish(dst), gpu.messages[-3:]
            got = dst.download()
        for o in (t, mid, dst, lut_v, lut_h):
            o.destroy()
        assert kernels == ["k_ortho_fast" if fast == "1" else "k_ortho"] * 2, kernels
        assert np.array_equal(got.astype(F), ref), (fast, util.diff_stats(got.view(np.uint16), ref.astype(np.float16).view(np.uint16)))


def test_the_renderers_lowpass_stays_on_the_fast_kernels(gpu, capfd):
    """a high_quality render of an HDR frame: the contrast-recovery low-pass (mirrored, pos within
    [0, 1]) is still one launch of k_lowpass2 -- and with the fused kernel switched off, its two
    passes, the only separable passes of that frame, run on k_ortho_fast. Same frame either way."""
    from test_gpu_fullsize import hdr_frame16
    from test_gpu_transfer_render import render
    outs = []
    for fused, want in (("1", ["k_lowpass2"]), ("0", ["k_ortho_fast"] * 2)):
        out, kernels = render(gpu, capfd, hdr_frame16(96, 64), "rgba16", pl.color_space("bt2020", "pq", max_luma=1000.0),
                              96, 64, "rgba16", pl.color_space("bt709", "bt1886"),
                              pl.render_params("high_quality", peak_detect_params=pl.peak_detect_params(percentile=99.995)),
                              PL_HIP_LOWPASS_FUSED=fused)
        assert [k for k in kernels if k.startswith(("k_ortho", "k_lowpass"))] == want, kernels
        outs.append(out)
    assert outs[0][..., :3].std() > 1000
    assert np.array_equal(outs[0], outs[1])


# ---- polar -------------------------------------------------------------------------------------

POLAR = [
    # source, rect kind, flipped, ratio, components
    ((48, 32), None, False, 2.0, 3), ((48, 32), None, False, 2.0, 4),
    ((48, 32), None, False, 0.5, 3),                    # (the downscale: gather order)
    ((48, 32), "slight", False, 2.0, 3), ((48, 32), "slight", True, 2.0, 4),
    ((48, 32), "periods", False, 0.5, 3), ((24, 16), "periods", True, 2.0, 3),
]


def polar_geometry(size, kind, flip, ratio):
    w, h = size
    rect = rect2(kind, w, h, flip) if kind else None
    rw, rh = (abs(rect[2] - rect[0]), abs(rect[3] - rect[1])) if rect else (w, h)
    assert (rw * ratio) == int(rw * ratio) and (rh * ratio) == int(rh * ratio)      # the ratio is exact
    return rect, int(rw * ratio), int(rh * ratio), orc.ewa_lanczos(blur=2.0 if ratio < 1 else 0.0)


# (the whole texture, clamped: test_gpu_sampling.py)
POLAR_CASES = [(c, m) for c in POLAR for m in (REPEAT, MIRROR, CLAMP) if c[1] or m != CLAMP]


@pytest.mark.parametrize("case,mode", POLAR_CASES, ids=lambda v: MODE_NAMES[v] if isinstance(v, int) else
                         "%dx%d-%s%s-x%g-c%d" % (v[0] + (v[1] or "whole", "-flipped" if v[2] else "") + v[3:]))
def test_polar(gpu, capfd, case, mode):
    size, kind, flip, ratio, comps = case
    rect, dw, dh, f = polar_geometry(size, kind, flip, ratio)
    src = util.random_rgba16(*size, seed=11)
    ref = polar_oracle(src, dw, dh, f, comps=comps, rect=rect and util.bound_rect(rect), address_mode=mode)
    got = polar_pipeline(gpu, src, dw, dh, comps=comps, rect=rect, address_mode=mode)
    util.assert_polar_equal(got, ref, what=(case, MODE_NAMES[mode]))
    if mode == CLAMP:
        return
    # the matrix-pipe kernels assume clamped addressing (polar_tables.c): with them switched on such
    # a pass must still go to the sequential-fma kernels -- and so match bit for bit
    with util.kernel_trace(capfd, PL_HIP_POLAR_MFMA="1") as kernels:
        got = polar_pipeline(gpu, src, dw, dh, comps=comps, rect=rect, address_mode=mode)
    polar = [k for k in kernels if k.startswith("k_polar")]
    assert polar and not any(k.startswith("k_polar_mx") for k in polar), kernels
    assert np.array_equal(got, ref), (case, MODE_NAMES[mode], kernels, util.diff_stats(got, ref))


@pytest.mark.parametrize("ratio", [2.0, 0.5])
@pytest.mark.parametrize("mode", [REPEAT, MIRROR], ids=MODE_NAMES.get)
def test_polar_one_component_half_float_plane(gpu, mode, ratio):
    w, h = 48, 32
    plane = random_tex("r16hf", w, h, seed=12)
    dw, dh = int(w * ratio), int(h * ratio)
    lut, radius, rz = orc.filter_generate_polar(orc.ewa_lanczos(blur=2.0 if ratio < 1 else 0.0))
    ref = orc.sample_polar(orc.tex_decode(plane, "r16hf"), lut, radius, rz, dw, dh, mask=0x1,
                           gather_order=not radius < 6.0, address_mode=mode)[..., :1]
    t = gpu.tex_create(w, h, "r16hf", plane)
    dst = gpu.tex_create(dw, dh, "r32f")
    obj = pl.ShaderObj()
    sh = gpu.begin()
    assert sh.sample_polar(t, pl.filter_config("ewa_lanczos"), obj, new_w=dw, new_h=dh, components=1,
                           address_mode=mode), gpu.messages[-3:]
    assert sh.finish(dst), gpu.messages[-3:]
    got = dst.download()
    for o in (t, dst, obj):
        o.destroy()
    util.assert_polar_equal(got, ref, what=(MODE_NAMES[mode], ratio))


# ---- the four-tap family and nearest -------------------------------------------------------------

SIMPLE_RECTS = [None, ("slight", False), ("slight", True), ("far", False), ("periods", False), ("periods", True)]
_simple_src = util.random_rgba16(33, 21, seed=54)
_simple_tex = None


@pytest.mark.parametrize("kind", list(KINDS) + ["gaussian"])
@pytest.mark.parametrize("out", [(70, 45), (16, 10)])
@pytest.mark.parametrize("mode", [REPEAT, MIRROR, CLAMP], ids=MODE_NAMES.get)
def test_simple_samplers(gpu, kind, out, mode):
    global _simple_tex
    if _simple_tex is None:
        _simple_tex = orc.tex_decode(_simple_src, "rgba16")
    dw, dh = out
    for r in SIMPLE_RECTS[1 if mode == CLAMP else 0:]:     # (the whole texture, clamped: test_gpu_sampling.py)
        rect = rect2(r[0], 33, 21, r[1]) if r else None
        got = run_simple(gpu, kind, _simple_src, "rgba16", dw, dh, rect=rect, address_mode=mode)
        ref = orc.tex_encode(orc.sample_simple(_simple_tex, KINDS.get(kind, orc.S_GAUSSIAN), dw, dh,
                                               rect=rect and util.bound_rect(rect), address_mode=mode,
                                               size=rect and util.rect_size(rect)), "rgba16")
        mx, n = util.diff_stats(got, ref)
        # gaussian: exp() is the native v_exp_f32 on the GPU, libm in the oracle (test_gaussian_within_1lsb)
        assert mx <= (1 if kind == "gaussian" else 0), (kind, out, MODE_NAMES[mode], r, mx, n)


# ---- debanding -----------------------------------------------------------------------------------

BIG = dict(iterations=2, radius=20.0)
DEBAND_CASES = [(BIG, False, REPEAT), (BIG, False, MIRROR), ({}, False, REPEAT), ({}, False, MIRROR),
                (BIG, True, REPEAT), (BIG, True, MIRROR), (BIG, True, CLAMP)]


@pytest.mark.parametrize("kw,outside,mode", DEBAND_CASES,
                         ids=["%s-%s%s" % ("r20x2" if k else "defaults", MODE_NAMES[m], "-outside" if o else "")
                              for k, o, m in DEBAND_CASES])
def test_deband(gpu, capfd, kw, outside, mode):
    """the statement of test_gpu_ortho_deband.py::test_deband_vs_oracle; a radius large enough that
    most border pixels take wrapped taps"""
    w, h = 64, 48
    img = banded(w, h)
    rect = rect2("slight", w, h) if outside else None
    ow, oh = (w + 9, h + 5) if outside else (w, h)
    t = gpu.tex_create(w, h, "rgba16", img)
    d = gpu.tex_create(ow, oh, "rgba32f")
    gpu.reset_frame()
    with util.kernel_trace(capfd) as kernels:
        sh = gpu.begin()
        src_kw = dict(rect=rect, new_w=ow, new_h=oh) if outside else {}
        assert sh.deband(t, address_mode=mode, **kw, **src_kw), gpu.messages[-3:]
        seed = int(sh.listing().split("seed=")[1].split(")")[0])
        assert sh.finish(d), gpu.messages[-3:]
        got = d.download()
    t.destroy(); d.destroy()
    assert kernels == ["k_deband"], kernels
    ref = orc.deband(orc.tex_decode(img, "rgba16"), ow, oh, mask=0xf, frame_index=seed,
                     rect=rect and util.bound_rect(rect), address_mode=mode, **kw)
    same = np.all(got == ref, axis=2).mean()
    print("deband %s %s outside=%s: %.5f of the pixels identical, max |diff| %.3g" %
          (MODE_NAMES[mode], kw, outside, same, np.abs(got - ref).max()))
    assert same >= 0.999, same
    assert np.abs(got - ref).max() <= (3.0 + 4.0) / 1000 + 1e-6
