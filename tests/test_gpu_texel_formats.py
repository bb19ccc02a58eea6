"""The emulated texture formats (bgra8, rgb10a2, bgr10a2) on the GPU: transfers through `ptr` and
through a pl_buf at shapes that take both kernel paths (16-byte groups and per-texel), the row
tail and more than one workgroup; exactness of the conversion as seen through blits; the format
order; the renderer with such textures as sources and as targets; pl_hip_wrap's refusal.
The reference for the arithmetic is tests/test_texel_formats.py's (Python integers)."""
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl
import libplacebo_amd._capi as capi
from test_texel_formats import ref_pack, ref_unpack

pytestmark = pytest.mark.gpu

FMTS = ["bgra8", "rgb10a2", "bgr10a2"]
STORAGE = {"bgra8": "rgba8", "rgb10a2": "rgba16", "bgr10a2": "rgba16"}


class BufParams(C.Structure):  # struct pl_buf_params
    _fields_ = [("size", C.c_size_t), ("host_writable", C.c_bool), ("host_readable", C.c_bool),
                ("host_mapped", C.c_bool), ("uniform", C.c_bool), ("storable", C.c_bool),
                ("drawable", C.c_bool), ("memory_type", C.c_int), ("format", C.c_void_p),
                ("export_handle", C.c_int), ("import_handle", C.c_int),
                ("shared_mem", capi.SharedMem), ("initial_data", C.c_void_p),
                ("user_data", C.c_void_p), ("debug_tag", C.c_char_p)]


@pytest.fixture(scope="module")
def L(gpu):
    lib = pl.lib()
    P = C.POINTER
    lib.pl_buf_create.restype = C.c_void_p
    lib.pl_buf_create.argtypes = [P(capi.Gpu), P(BufParams)]
    lib.pl_buf_destroy.restype = None
    lib.pl_buf_destroy.argtypes = [P(capi.Gpu), P(C.c_void_p)]
    lib.pl_buf_write.restype = None
    lib.pl_buf_write.argtypes = [P(capi.Gpu), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.pl_buf_read.restype = C.c_bool
    lib.pl_buf_read.argtypes = [P(capi.Gpu), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    return lib


class Buf:
    def __init__(self, L, gpu, data):
        self.L, self.gpu = L, gpu
        data = np.ascontiguousarray(data, np.uint8)
        bp = BufParams(size=data.size, host_writable=True, host_readable=True,
                       initial_data=data.ctypes.data)
        self.ptr = C.c_void_p(L.pl_buf_create(gpu.gpu, C.byref(bp)))
        assert self.ptr, gpu.messages[-3:]
        self.size = data.size

    def read(self):
        out = np.empty(self.size, np.uint8)
        assert self.L.pl_buf_read(self.gpu.gpu, self.ptr, 0, out.ctypes.data, self.size)
        return out

    def destroy(self):
        self.L.pl_buf_destroy(self.gpu.gpu, C.byref(self.ptr))


def words(rng, h, w):
    """random texels in host layout: one uint32 per texel"""
    return rng.integers(0, 1 << 32, (max(h, 1), w), dtype=np.uint64).astype(np.uint32)


def transfer(gpu, tex, upload, rc=None, ptr=None, buf=None, buf_offset=0, row_pitch=0, timer=None,
             callback=None):
    xp = capi.TexTransferParams(tex=tex.ptr, row_pitch=row_pitch, timer=timer, callback=callback,
                                buf=buf.ptr if buf else None, buf_offset=buf_offset,
                                ptr=ptr.ctypes.data if ptr is not None else None)
    if rc:
        xp.rc = capi.Rect3d(rc[0], rc[1], 0, rc[2], rc[3], 1)
    fn = pl.lib().pl_tex_upload if upload else pl.lib().pl_tex_download
    return fn(gpu.gpu, C.byref(xp))


def download_words(gpu, tex):
    out = np.zeros((max(tex.h, 1), tex.w), np.uint32)
    assert transfer(gpu, tex, False, ptr=out), gpu.messages[-3:]
    return out


# (w, h, rc or None): 37x5 and 1027x3 (odd widths: a row tail; 1027 = more than one workgroup
# across), 1D 16 (only whole groups) and 1 (only a tail), and a rect that starts off the 16-byte
# grid of the storage
SHAPES = [(37, 5, None), (1027, 3, None), (16, 0, None), (1, 0, None), (37, 5, (3, 1, 30, 4))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{'rc' if s[2] else ''}")
@pytest.mark.parametrize("fmt", FMTS)
def test_round_trip_through_ptr(gpu, fmt, shape):
    w, h, rc = shape
    rng = np.random.default_rng(w * 7 + h)
    tex = gpu.tex_create(w, h, fmt)
    try:
        full = words(rng, h, w)
        assert transfer(gpu, tex, True, ptr=full), gpu.messages[-3:]
        assert np.array_equal(download_words(gpu, tex), full)
        x0, y0, x1, y1 = rc or (0, 0, w, max(h, 1))
        rw, rh = x1 - x0, y1 - y0
        for extra in (0, 1):        # tight rows (16-byte path where w allows), rows + 4 bytes
            part = words(rng, rh, rw + extra)
            pitch = 4 * (rw + extra)
            assert transfer(gpu, tex, True, rc=rc, ptr=part, row_pitch=pitch), gpu.messages[-3:]
            full[y0:y1, x0:x1] = part[:, :rw]
            assert np.array_equal(download_words(gpu, tex), full)       # outside rc: untouched
            back = np.full((rh, rw + extra), 0xdeadbeef, np.uint32)
            assert transfer(gpu, tex, False, rc=rc, ptr=back, row_pitch=pitch), gpu.messages[-3:]
            assert np.array_equal(back[:, :rw], part[:, :rw])
            assert np.all(back[:, rw:] == 0xdeadbeef)                   # the padding: untouched
    finally:
        tex.destroy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{'rc' if s[2] else ''}")
@pytest.mark.parametrize("fmt", FMTS)
def test_round_trip_through_buffer(gpu, L, fmt, shape):
    w, h, rc = shape
    rng = np.random.default_rng(w * 11 + h)
    tex = gpu.tex_create(w, h, fmt)
    x0, y0, x1, y1 = rc or (0, 0, w, max(h, 1))
    rw, rh = x1 - x0, y1 - y0
    full = words(rng, h, w)
    assert transfer(gpu, tex, True, ptr=full), gpu.messages[-3:]
    bufs = []
    try:
        for offset, extra in ((0, 0), (4, 0), (16, 0), (16, 1), (4, 1)):
            pitch = 4 * (rw + extra)
            span = (rh - 1) * pitch + 4 * rw
            src = rng.integers(0, 256, offset + span + 20, dtype=np.uint8)
            up = Buf(L, gpu, src)
            down = Buf(L, gpu, np.full(src.size, 0x5a, np.uint8))
            bufs += [up, down]
            assert transfer(gpu, tex, True, rc=rc, buf=up, buf_offset=offset, row_pitch=pitch)
            rows = [src[offset + y * pitch:offset + y * pitch + 4 * rw].view(np.uint32)
                    for y in range(rh)]
            full[y0:y1, x0:x1] = np.stack(rows)
            assert np.array_equal(download_words(gpu, tex), full)
            assert transfer(gpu, tex, False, rc=rc, buf=down, buf_offset=offset, row_pitch=pitch)
            want = np.full(src.size, 0x5a, np.uint8)
            for y in range(rh):
                a = offset + y * pitch
                want[a:a + 4 * rw] = src[a:a + 4 * rw]
            assert np.array_equal(down.read(), want)    # byte for byte, the rest untouched
            assert np.array_equal(up.read(), src)
    finally:
        for b in bufs:
            b.destroy()
        tex.destroy()


@pytest.mark.parametrize("fmt", FMTS)
def test_initial_data_timer_callback_and_unaligned_offset(gpu, L, fmt):
    rng = np.random.default_rng(21)
    a = words(rng, 5, 37)
    dt, nc = pl._FMT_DTYPES[fmt]
    tex = gpu.tex_create(37, 5, fmt, a.view(dt).reshape(5, 37, nc))
    assert np.array_equal(download_words(gpu, tex), a)
    assert np.array_equal(tex.download().reshape(5, -1).view(np.uint32), a)    # the Python helper

    timer = gpu.timer()
    called = []
    cb = C.CFUNCTYPE(None, C.c_void_p)(lambda priv: called.append(priv))
    b = words(rng, 5, 37)
    assert transfer(gpu, tex, True, ptr=b, timer=timer, callback=C.cast(cb, C.c_void_p))
    assert called == [None]
    out = np.zeros_like(b)
    assert transfer(gpu, tex, False, ptr=out, timer=timer, callback=C.cast(cb, C.c_void_p))
    assert len(called) == 2 and np.array_equal(out, b)
    gpu.finish()
    assert gpu.timer_query(timer) > 0 and gpu.timer_query(timer) > 0
    pl.lib().pl_timer_destroy(gpu.gpu, C.byref(timer))

    # texel_align = 4 covers the buffer offset and the row pitch: refused, nothing written
    buf = Buf(L, gpu, np.zeros(37 * 5 * 4 + 8, np.uint8))
    assert not transfer(gpu, tex, False, buf=buf, buf_offset=2)
    assert not transfer(gpu, tex, False, buf=buf, row_pitch=37 * 4 + 2)
    assert not buf.read().any()
    buf.destroy()
    tex.destroy()


@pytest.fixture(scope="module")
def every_code():
    """1024 x 4 words: every colour code (a different one in every field) x every alpha code"""
    c = np.arange(1024, dtype=np.uint32)[None, :]
    a = np.arange(4, dtype=np.uint32)[:, None]
    return (c | ((1023 - c) << 10) | ((c ^ 0x155) << 20) | (a << 30)).astype(np.uint32)


@pytest.mark.parametrize("fmt", ["rgb10a2", "bgr10a2"])
def test_unpack_is_exact(gpu, fmt, every_code):
    src = gpu.tex_create(1024, 4, fmt, every_code)
    dst = gpu.tex_create(1024, 4, "rgba16")
    dst.blit_from(src)
    assert np.array_equal(dst.download(), ref_unpack(fmt, every_code))
    src.destroy()
    dst.destroy()


@pytest.mark.parametrize("fmt", ["rgb10a2", "bgr10a2"])
@pytest.mark.parametrize("size", [(37, 5), (1027, 3)])
def test_pack_is_exact(gpu, fmt, size):
    w, h = size
    texels = np.random.default_rng(w).integers(0, 65536, (h, w, 4)).astype(np.uint16)
    texels[0, :4] = [[0, 65535, 32767, 32768], [32, 33, 10922, 10923], [65503, 65502, 54612, 54613],
                     [65535, 0, 1, 65534]]
    src = gpu.tex_create(w, h, "rgba16", texels)
    dst = gpu.tex_create(w, h, fmt)
    dst.blit_from(src)
    assert np.array_equal(dst.download()[..., 0], ref_pack(fmt, texels))
    src.destroy()
    dst.destroy()


@pytest.mark.parametrize("size", [(37, 5), (1027, 3)])
def test_bgra8_blits_permute_the_bytes(gpu, size):
    w, h = size
    b = np.random.default_rng(h).integers(0, 256, (h, w, 4)).astype(np.uint8)
    for a_fmt, b_fmt in (("bgra8", "rgba8"), ("rgba8", "bgra8")):
        src = gpu.tex_create(w, h, a_fmt, b)
        dst = gpu.tex_create(w, h, b_fmt)
        dst.blit_from(src)
        assert np.array_equal(dst.download(), b[..., [2, 1, 0, 3]])
        src.destroy()
        dst.destroy()


# ---- format order ---------------------------------------------------------------------------

# pl_find_fmt's answers before these formats existed: the suffix by (type, min depth, host bits)
# for a capability every format has; UNORM = 1, FLOAT = 5. Anything not listed: no format.
SUFFIX = {
    (1, 0, 0): "8", (1, 0, 8): "8", (1, 0, 16): "16",
    (1, 8, 0): "8", (1, 8, 8): "8", (1, 8, 16): "16",
    (1, 10, 0): "16", (1, 10, 16): "16", (1, 16, 0): "16", (1, 16, 16): "16",
    (5, 0, 0): "16hf", (5, 0, 16): "16hf", (5, 0, 32): "32f",
    (5, 8, 0): "16hf", (5, 8, 16): "16hf", (5, 8, 32): "32f",
    (5, 10, 0): "16hf", (5, 10, 16): "16hf", (5, 10, 32): "32f",
    (5, 16, 0): "16hf", (5, 16, 16): "16hf", (5, 16, 32): "32f",
    (5, 32, 0): "32f", (5, 32, 32): "32f",
}
PREFIX = {1: "r", 2: "rg", 4: "rgba"}
CAP_VERTEX, CAP_TEXEL_UNIFORM, CAP_TEXEL_STORAGE = 1 << 6, 1 << 7, 1 << 8


def parent_answer(typ, comps, depth, host_bits, cap):
    if comps not in PREFIX or cap in (CAP_TEXEL_UNIFORM, CAP_TEXEL_STORAGE):
        return None
    if cap == CAP_VERTEX:       # only the 32-bit float formats are vertex formats
        return PREFIX[comps] + "32f" if typ == 5 and host_bits in (0, 32) else None
    suffix = SUFFIX.get((typ, depth, host_bits))
    return PREFIX[comps] + suffix if suffix else None


def test_format_order_and_queries(gpu):
    g = gpu.gpu.contents
    names = [g.formats[i].contents.name.decode() for i in range(g.num_formats)]
    assert names[:12] == ["r8", "rg8", "rgba8", "r16", "r16hf", "rg16", "rg16hf", "rgba16",
                          "rgba16hf", "r32f", "rg32f", "rgba32f"]
    assert names[12:] == ["bgra8", "rgb10a2", "bgr10a2"]
    assert [g.formats[i].contents.emulated for i in range(g.num_formats)] == [False] * 12 + [True] * 3

    lib = pl.lib()
    for typ in range(0, 6):
        for comps in range(1, 5):
            for depth in (0, 8, 10, 16, 32):
                for host_bits in (0, 8, 16, 32):
                    for bit in range(11):
                        f = lib.pl_find_fmt(gpu.gpu, typ, comps, depth, host_bits, 1 << bit)
                        got = f.contents.name.decode() if f else None
                        assert not (f and f.contents.emulated)
                        assert got == parent_answer(typ, comps, depth, host_bits, 1 << bit), \
                            (typ, comps, depth, host_bits, bit, got)
    # (the reference's own test)
    assert lib.pl_find_fmt(gpu.gpu, 1, 4, 0, 0, 1 << 5).contents.name == b"rgba8"

    def find(bits, cmap):
        d = capi.PlaneData(type=pl.FMT_UNORM, width=8, height=8, pixel_stride=4)
        for c, b in enumerate(bits):
            d.component_size[c] = b
            d.component_map[c] = cmap[c]
        m = (C.c_int * 4)()
        f = lib.pl_plane_find_fmt(gpu.gpu, m, C.byref(d))
        return (f.contents.name.decode() if f else None), list(m)

    assert find([10, 10, 10], [2, 1, 0]) == ("rgb10a2", [2, 1, 0, -1])        # x2rgb10
    assert find([10, 10, 10, 2], [0, 1, 2, 3]) == ("rgb10a2", [0, 1, 2, 3])
    assert find([8, 8, 8, 8], [2, 1, 0, 3]) == ("rgba8", [2, 1, 0, 3])        # as before


def test_wrap_refuses_emulated_formats(gpu):
    backing = gpu.tex_create(16, 4, "rgba16")
    ptr, pitch = backing.device_ptr()
    for fmt in FMTS:
        before = len(gpu.messages)
        wp = capi.HipWrapParams(ptr=ptr, width=16, height=4, row_pitch=pitch, format=gpu.fmt(fmt))
        assert not pl.lib().pl_hip_wrap(gpu.gpu, C.byref(wp))
        new = gpu.messages[before:]
        assert any(level == 2 and "emulated" in msg for level, msg in new), new   # PL_LOG_ERR
    # pl_hip_tex_ptr of an emulated texture: the storage (rgba16: 8 bytes a texel)
    t = gpu.tex_create(100, 4, "rgb10a2")
    assert t.device_ptr()[0] and t.device_ptr()[1] >= 800
    t.destroy()
    backing.destroy()


# ---- renderer -------------------------------------------------------------------------------

PRESETS = ["fast", "default"]


def render_to(gpu, rr, image, fmt, w=48, h=20, params=None, bits=None):
    dst = gpu.tex_create(w, h, fmt)
    target = pl.frame(dst)
    if bits:
        target.repr = pl.color_repr("rgb", "full", sample_depth=bits, color_depth=bits)
    assert rr.render(image, target, params), gpu.messages[-4:]
    out = dst.download()
    dst.destroy()
    return out


@pytest.mark.parametrize("preset", PRESETS)
def test_source_twins(gpu, preset):
    """a packed source plane renders exactly as the ordered plane holding its unpacked values"""
    rng = np.random.default_rng(31)
    x2rgb10 = words(rng, 10, 24) & np.uint32(0x3fffffff)
    rr = pl.Renderer(gpu)
    params = pl.render_params(preset)
    texs = []

    def rendered(tex, mapping):
        texs.append(tex)
        return render_to(gpu, rr, pl.frame(tex, components=len(mapping), mapping=mapping),
                         "rgba16", params=params)

    # (a) pl_upload_plane finds rgb10a2 for x2rgb10 words; (b) rgba16 with the formula's values
    plane, t = pl.upload_plane(gpu, pl.plane_data(x2rgb10, [10, 10, 10], [2, 1, 0], pixel_stride=4))
    assert t.fmt_name == "rgb10a2" and list(plane.component_mapping) == [2, 1, 0, -1]
    a = rendered(t, [2, 1, 0])
    b = rendered(gpu.tex_create(24, 10, "rgba16", ref_unpack("rgb10a2", x2rgb10)), [2, 1, 0])
    assert np.array_equal(a, b)
    # the same words as a bgr10a2 plane: host component c is sampled as channel sample_order[c]
    c = rendered(gpu.tex_create(24, 10, "bgr10a2", x2rgb10), [2, 1, 0])
    d = rendered(gpu.tex_create(24, 10, "rgba16", ref_unpack("bgr10a2", x2rgb10)), [0, 1, 2])
    assert np.array_equal(c, d) and np.array_equal(c, a)

    by = rng.integers(0, 256, (10, 24, 4)).astype(np.uint8)
    e = rendered(gpu.tex_create(24, 10, "bgra8", by), [2, 1, 0, 3])
    f = rendered(gpu.tex_create(24, 10, "rgba8", by[..., [2, 1, 0, 3]]), [0, 1, 2, 3])
    assert np.array_equal(e, f)
    assert a.std() > 1000 and e.std() > 1000    # (pictures, not blanks)
    for t in texs:
        t.destroy()
    rr.destroy()


@pytest.mark.parametrize("preset", PRESETS)
def test_target_twins(gpu, preset):
    rng = np.random.default_rng(32)
    src = gpu.tex_create(24, 10, "rgba16", rng.integers(0, 65536, (10, 24, 4)).astype(np.uint16))
    image = pl.frame(src)
    rr = pl.Renderer(gpu)
    dithered = pl.render_params(preset) if preset == "default" else pl.render_params(
        preset, dither_params=capi.DitherParams.in_dll(pl.lib(), "pl_dither_default_params"))
    plain = pl.render_params(preset, dither_params=None)

    exact = render_to(gpu, rr, image, "rgba32f", params=plain).astype(np.float64)
    v = np.clip(exact[..., :3], 0.0, 1.0) * 1023       # (unorm storage clamps)
    for fmt in ("rgb10a2", "bgr10a2"):
        order = [0, 1, 2] if fmt == "rgb10a2" else [2, 1, 0]
        for params in (dithered, plain):
            packed = render_to(gpu, rr, image, fmt, params=params)[..., 0]
            twin = render_to(gpu, rr, image, "rgba16", params=params, bits=10)
            assert np.array_equal(packed, ref_pack(fmt, twin))
            # the target side does not consult sample_order: field i of the word is component i
            codes = np.stack([(packed >> np.uint32(10 * i)) & np.uint32(1023) for i in order],
                             axis=-1).astype(np.float64)
            err = np.abs(codes - v).max()
            print(f"{fmt} {preset} {'dithered' if params is dithered else 'plain'}: "
                  f"max |code - x * 1023| = {err:.6f}")
            if params is dithered:
                assert np.all((codes == np.floor(v)) | (codes == np.ceil(v)))
            else:
                # rounding to 16 bits, then to 10: half a 10-bit step plus half a 16-bit step,
                # plus 1e-3 codes for the float32 evaluation of x
                assert err <= 0.5 + 0.5 * 1023 / 65535 + 1e-3
        assert len(np.unique(codes)) > 100

    for params in (dithered, plain):
        b = render_to(gpu, rr, image, "bgra8", params=params)
        r = render_to(gpu, rr, image, "rgba8", params=params)
        assert np.array_equal(b, r[..., [2, 1, 0, 3]]) and r.std() > 10
    src.destroy()
    rr.destroy()
