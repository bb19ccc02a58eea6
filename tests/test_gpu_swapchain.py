"""The headless swapchain (swapchain.h, hip_swapchain.h) on the GPU: what the reference's render
loop sees (frames, hint, resize, latency) and what the consumer sees (order, contents, host copies,
reuse hazards). Frames are 70 x 46: no row is a multiple of the 256-byte transfer pitch. Every
blocking call carries a timeout of 2 s at most; nothing here sleeps."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

W, H = 70, 46
SEC = 1_000_000_000
TIMEOUT = 2 * SEC
ERR, WARN, DEBUG = 2, 3, 5


def tex_addr(ptr):
    return C.cast(ptr, C.c_void_p).value


def clear_frame(gpu, swframe, rgba):
    pl.lib().pl_tex_clear(gpu.gpu, swframe.fbo, (C.c_float * 4)(*rgba))


def produce(gpu, sw, rgba):
    """one cleared frame through start / submit / swap; the fbo's address"""
    f = sw.start_frame()
    assert f is not None, gpu.messages[-3:]
    clear_frame(gpu, f, rgba)
    assert sw.submit_frame()
    sw.swap_buffers()
    return tex_addr(f.fbo)


def take(sw):
    p = sw.acquire(TIMEOUT)
    assert p is not None, "acquire timed out"
    return p


def struct_bytes(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


def inferred(csp):
    out = capi.ColorSpace()
    C.memmove(C.byref(out), C.byref(csp), C.sizeof(out))
    pl.lib().pl_color_space_infer(C.byref(out))
    return out


@pytest.fixture(scope="module")
def gradient():
    return util.chirp_rgba16(W, H)


def render_into(gpu, image, target):
    """pl_render_image with the default preset (which dithers to the target's depth) on a
    renderer of its own, blue noise from the same seed"""
    rr = pl.Renderer(gpu)
    util.srand(1)
    ok = rr.render(image, target, pl.render_params("default"))
    errors = rr.errors()
    gpu.finish()
    rr.destroy()
    assert ok and errors == 0, gpu.messages[-4:]


# ---- 1. parity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16", "rgb10a2", "rgba16hf"])
def test_render_into_a_swapchain_frame_equals_render_into_a_texture(gpu, gradient, fmt):
    """same kernels, same parameters: byte-identical"""
    src = gpu.tex_create(W, H, "rgba16", gradient)
    image = pl.frame(src, components=3)
    sw = pl.Swapchain(gpu, W, H, fmt=fmt)
    f = sw.start_frame()
    assert f is not None and not f.flipped
    fbo = f.fbo.contents.params
    assert (fbo.w, fbo.h, fbo.format.contents.name.decode()) == (W, H, fmt)
    assert fbo.renderable and fbo.blit_dst
    depth = fbo.format.contents.component_depth[0]
    assert (f.color_repr.bits.sample_depth, f.color_repr.bits.color_depth) == (depth, depth)
    assert (f.color_repr.sys, f.color_repr.levels) == (pl.SYS["rgb"], pl.LEVELS["full"])

    target = sw.target(f)
    assert target.num_planes == 1 and tex_addr(target.planes[0].texture) == tex_addr(f.fbo)
    assert target.planes[0].components == 4 and not target.planes[0].flipped
    assert list(target.planes[0].component_mapping) == [0, 1, 2, 3]
    assert (target.crop.x0, target.crop.y0, target.crop.x1, target.crop.y1) == (0, 0, W, H)
    assert struct_bytes(target.color) == struct_bytes(f.color_space)
    render_into(gpu, image, target)
    assert sw.submit_frame()
    sw.swap_buffers()
    p = take(sw)
    assert tex_addr(p.tex) == tex_addr(f.fbo)
    got = sw.texture(p.tex).download()
    sw.release(p.tex)

    plain = gpu.tex_create(W, H, fmt)
    render_into(gpu, image, pl.frame(plain, repr_=f.color_repr, color=f.color_space))
    ref = plain.download()
    assert got.tobytes() == ref.tobytes()
    assert len(np.unique(got.view(np.uint8))) > 16     # (an image, not a blank)
    sw.destroy(); plain.destroy(); src.destroy()


def test_frame_from_swapchain_caps_components_without_alpha(gpu):
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8", alpha="none")
    f = sw.start_frame()
    assert f.color_repr.alpha == pl.ALPHA["none"]
    assert sw.target(f).planes[0].components == 3
    assert sw.submit_frame()
    sw.destroy()


# ---- 2. ring order -----------------------------------------------------------------------------
COLOURS = [(1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 1, 1), (1, 1, 0, 1), (0, 1, 1, 0)]


def test_five_frames_through_three_images_arrive_in_order(gpu):
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8", num_images=3)
    assert sw.latency() == 2
    seen = []
    for i, rgba in enumerate(COLOURS):
        fbo = produce(gpu, sw, rgba)
        p = take(sw)
        assert p.seq == i and tex_addr(p.tex) == fbo and p.ready_event
        assert not p.host_ptr and p.host_pitch == 0
        got = sw.texture(p.tex).download()
        assert np.array_equal(got, np.broadcast_to(np.array(rgba, np.uint8) * 255, (H, W, 4))), i
        seen.append(fbo)
        sw.release(p.tex)
    assert len(set(seen)) == 3 and seen[3:] == seen[:2], seen
    assert sw.acquire(0) is None
    sw.destroy()


def test_presented_images_queue_up_oldest_first(gpu):
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8", num_images=3, latency=1)
    assert sw.latency() == 1
    for rgba in COLOURS[:3]:
        produce(gpu, sw, rgba)
    for i, rgba in enumerate(COLOURS[:3]):
        p = sw.acquire(0)       # latency 1: swap_buffers has waited for each of them
        assert p is not None and p.seq == i
        assert tuple(sw.texture(p.tex).download()[H // 2, W // 2]) == tuple(255 * c for c in rgba)
        sw.release(p.tex)
    sw.destroy()


# ---- 3. exhaustion -----------------------------------------------------------------------------
def test_start_frame_refuses_without_blocking_when_nothing_is_free(built):
    with pl.HipGpu(0, log_level=DEBUG) as g:
        sw = pl.Swapchain(g, W, H, fmt="rgba8", num_images=3)
        for rgba in COLOURS[:3]:
            produce(g, sw, rgba)        # (swap_buffers returns with the consumer idle)
        n = len(g.messages)
        t0 = time.monotonic()
        assert sw.start_frame() is None
        assert time.monotonic() - t0 < 1.0
        said = [m for lev, m in g.messages[n:] if "pl_swapchain_start_frame" in m]
        assert len(said) == 1 and g.messages[n:][0][0] == DEBUG, g.messages[n:]
        p = take(sw)
        assert sw.start_frame() is None     # held is not free either
        sw.release(p.tex)
        f = sw.start_frame()
        assert f is not None and tex_addr(f.fbo) == tex_addr(p.tex)
        assert sw.submit_frame()
        sw.swap_buffers()
        sw.destroy()


def test_no_size_no_frame(gpu):
    sw = pl.Swapchain(gpu, 0, 0, fmt="rgba8")
    assert sw.resize() == (True, 0, 0)
    assert sw.start_frame() is None
    assert sw.resize(W, H) == (True, W, H)
    produce(gpu, sw, COLOURS[0])
    p = take(sw)
    assert (p.tex.contents.params.w, p.tex.contents.params.h) == (W, H)
    sw.release(p.tex)
    sw.destroy()


# ---- 4. host readback --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba8", "rgba16", "rgb10a2"])
def test_host_copy_equals_a_download(gpu, gradient, fmt):
    src = gpu.tex_create(W, H, "rgba16", gradient)
    image = pl.frame(src, components=3)
    sw = pl.Swapchain(gpu, W, H, fmt=fmt, host_readback=True)
    slots = {}
    for i in range(5):
        f = sw.start_frame()
        assert f is not None
        if i % 2:
            clear_frame(gpu, f, COLOURS[i])
        else:
            render_into(gpu, image, sw.target(f))
        assert sw.submit_frame()
        sw.swap_buffers()
        p = take(sw)
        texel = p.tex.contents.params.format.contents.texel_size
        assert p.host_ptr and p.host_pitch >= W * texel and p.host_pitch % texel == 0
        host = sw.host_image(p)
        ref = sw.texture(p.tex).download()
        assert host.dtype == ref.dtype and host.tobytes() == ref.tobytes(), i
        if not i:
            assert len(np.unique(host.view(np.uint8))) > 16
        assert slots.setdefault(tex_addr(p.tex), p.host_ptr) == p.host_ptr
        sw.release(p.tex)
    assert len(slots) == 3 and len(set(slots.values())) == 3
    sw.destroy(); src.destroy()


# ---- 5. colour-space hint ----------------------------------------------------------------------
def pq_ramp():
    """a horizontal PQ ramp from 0 to the code of 1000 cd/m^2, as rgba16"""
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 32, 3424 / 4096, 2413 / 128, 2392 / 128
    y = (1000 / 10000) ** m1
    top = ((c1 + c2 * y) / (1 + c3 * y)) ** m2
    ramp = np.rint(np.linspace(0, top, W) * 65535).astype(np.uint16)
    img = np.empty((H, W, 4), np.uint16)
    img[..., :3] = ramp[None, :, None]
    img[..., 3] = 65535
    return img


def test_hint_selects_colour_space_metadata_and_format(gpu):
    hint = pl.color_space("bt2020", "pq", max_luma=1000.0)
    want = inferred(hint)
    assert want.hdr.max_luma == 1000.0 and want.hdr.min_luma > 0    # (infer fills the rest)
    srgb = inferred(capi.ColorSpace.in_dll(pl.lib(), "pl_color_space_srgb"))
    ramp = pq_ramp()
    src = gpu.tex_create(W, H, "rgba16", ramp)
    image = pl.frame(src, components=3, color=want)
    fast = pl.render_params("fast")
    rr = pl.Renderer(gpu)

    sw = pl.Swapchain(gpu, W, H)
    f = sw.start_frame()    # no hint yet: sRGB on rgba8
    assert f.fbo.contents.params.format.contents.name == b"rgba8"
    assert struct_bytes(f.color_space) == struct_bytes(srgb)
    assert sw.submit_frame()
    sw.release(take(sw).tex)

    sw.colorspace_hint(hint)
    f = sw.start_frame()
    assert (f.color_space.primaries, f.color_space.transfer) == (pl.PRIM["bt2020"], pl.TRC["pq"])
    assert f.color_space.hdr.max_luma == 1000.0
    assert struct_bytes(f.color_space) == struct_bytes(want)
    assert f.fbo.contents.params.format.contents.name == b"rgb10a2"
    assert (f.color_repr.bits.sample_depth, f.color_repr.bits.color_depth) == (10, 10)
    assert rr.render(image, sw.target(f), fast) and rr.errors() == 0
    assert sw.submit_frame()
    p = take(sw)
    assert struct_bytes(p.color_space) == struct_bytes(want) and p.color_repr.bits.color_depth == 10
    word = sw.texture(p.tex).download()[..., 0]
    sw.release(p.tex)
    # Source and target colour spaces are equal, the size is 1:1 and the fast preset does not
    # dither: the PQ codes pass through, rounded once to 10 bits (half a code), with one more code
    # allowed for the rounding of the 16-bit code to the float the pass computes in.
    passed = np.stack([(word >> s) & 1023 for s in (0, 10, 20)], -1).astype(np.float64)
    d = np.abs(passed - ramp[..., :3] * (1023 / 65535)).max()
    print(f"PQ hint: max |10-bit code - source| = {d:.3f}")
    assert d <= 1.5

    sw.colorspace_hint(None)
    f = sw.start_frame()
    assert struct_bytes(f.color_space) == struct_bytes(srgb)
    assert f.fbo.contents.params.format.contents.name == b"rgba8"
    assert (f.color_repr.bits.sample_depth, f.color_repr.bits.color_depth) == (8, 8)
    assert rr.render(image, sw.target(f), fast) and rr.errors() == 0
    assert sw.submit_frame()
    p = take(sw)
    mapped = sw.texture(p.tex).download()
    sw.release(p.tex)

    plain = gpu.tex_create(W, H, "rgba8")
    assert rr.render(image, pl.frame(plain, repr_=f.color_repr, color=f.color_space), fast)
    assert mapped.tobytes() == plain.download().tobytes()
    # tone-mapped, not passed through: the 8-bit sRGB picture is not the PQ codes cut to 8 bits
    assert np.abs(mapped[..., :3].astype(int) - (ramp[..., :3] >> 8)).max() > 8
    assert mapped[0, 0, 0] < mapped[0, W // 2, 0] < mapped[0, W - 1, 0]
    # ... and below 1.0: a pixel well above SDR white (203 cd/m^2), which clipping would put at
    # 255, keeps room under the 1000 cd/m^2 peak
    col = W * 9 // 10
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 32, 3424 / 4096, 2413 / 128, 2392 / 128
    e = (ramp[0, col, 0] / 65535) ** (1 / m2)
    nits = 10000 * (max(e - c1, 0) / (c2 - c3 * e)) ** (1 / m1)
    print(f"sRGB hint: {nits:.0f} cd/m^2 -> {mapped[0, col, 0]}, peak -> {mapped[0, W - 1, 0]}")
    assert 400 < nits < 1000 and mapped[0, col, 0] < 255
    rr.destroy(); sw.destroy(); plain.destroy(); src.destroy()


def test_bare_hdr_hint_gets_hdr10_metadata(gpu):
    """swapchain.h's defaults come before the inference: an HDR transfer without metadata carries
    pl_hdr_metadata_hdr10, metadata without a transfer means PQ"""
    hdr10 = capi.HdrMetadata.in_dll(pl.lib(), "pl_hdr_metadata_hdr10")
    sw = pl.Swapchain(gpu, W, H)
    sw.colorspace_hint(pl.color_space("bt2020", "pq"))
    f = sw.start_frame()
    want = capi.ColorSpace(primaries=pl.PRIM["bt2020"], transfer=pl.TRC["pq"], hdr=hdr10)
    assert hdr10.max_luma > 0 and f.color_space.hdr.max_luma == hdr10.max_luma
    assert struct_bytes(f.color_space) == struct_bytes(inferred(want))
    assert sw.submit_frame()
    sw.release(take(sw).tex)

    only_metadata = capi.ColorSpace()
    only_metadata.hdr.max_luma = 600.0
    sw.colorspace_hint(only_metadata)
    f = sw.start_frame()
    assert f.color_space.transfer == pl.TRC["pq"] and f.color_space.hdr.max_luma == 600.0
    want = capi.ColorSpace(transfer=pl.TRC["pq"])
    want.hdr.max_luma = 600.0
    assert struct_bytes(f.color_space) == struct_bytes(inferred(want))
    assert f.fbo.contents.params.format.contents.name == b"rgb10a2"
    assert sw.submit_frame()
    sw.destroy()


def test_format_follows_the_hint_only_once_nothing_is_presented_or_held(gpu):
    sw = pl.Swapchain(gpu, W, H)
    produce(gpu, sw, COLOURS[0])
    sw.colorspace_hint(pl.color_space("bt2020", "hlg"))
    f = sw.start_frame()    # one image is presented: the ring stays rgba8, the colour space moves
    assert f.fbo.contents.params.format.contents.name == b"rgba8"
    assert f.color_space.transfer == pl.TRC["hlg"] and f.color_repr.bits.color_depth == 8
    assert sw.submit_frame()
    for _ in range(2):
        sw.release(take(sw).tex)
    f = sw.start_frame()
    assert f.fbo.contents.params.format.contents.name == b"rgb10a2"
    assert sw.submit_frame()
    sw.destroy()


# ---- 6. resize ---------------------------------------------------------------------------------
def test_resize_is_lazy_and_clamped(gpu):
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8")
    assert sw.resize() == (True, W, H)
    produce(gpu, sw, COLOURS[0])
    held = take(sw)
    assert sw.resize(33, 17) == (True, 33, 17)
    assert (held.tex.contents.params.w, held.tex.contents.params.h) == (W, H)
    assert np.array_equal(sw.texture(held.tex).download()[0, 0], [255, 0, 0, 255])
    for i in range(2):
        produce(gpu, sw, COLOURS[1 + i])
        p = take(sw)
        assert (p.tex.contents.params.w, p.tex.contents.params.h) == (33, 17)
        assert sw.texture(p.tex).download().shape == (17, 33, 4)
        sw.release(p.tex)
    assert (held.tex.contents.params.w, held.tex.contents.params.h) == (W, H)
    sw.release(held.tex)
    for i in range(3):      # every slot has come round: none keeps the old size
        produce(gpu, sw, COLOURS[i])
        p = take(sw)
        assert (p.tex.contents.params.w, p.tex.contents.params.h) == (33, 17)
        sw.release(p.tex)
    limit = gpu.gpu.contents.limits.max_tex_2d_dim
    assert sw.resize(limit + 1000, 10) == (True, limit, 10)
    assert sw.resize(W, H) == (True, W, H)
    sw.destroy()


# ---- 7. consumer stream ------------------------------------------------------------------------
class BusyConsumer:
    """a HIP stream of the consumer's own that is busy for a while (16 x 256 MiB of copies) and
    then copies an image's storage out; everything it allocated goes in close()"""
    BIG = 256 << 20

    def __init__(self):
        self.hip = util.hip_runtime()
        self.stream, self.mem = C.c_void_p(), []
        self.ok(self.hip.hipStreamCreate(C.byref(self.stream)))

    @staticmethod
    def ok(rc):
        assert rc == 0, rc

    def alloc(self, size):
        ptr = C.c_void_p()
        self.ok(self.hip.hipMalloc(C.byref(ptr), C.c_size_t(size)))
        self.mem.append(ptr)
        return ptr

    def copy_out_later(self, tex):
        ptr, pitch = tex.device_ptr()
        self.size, self.pitch = pitch * tex.h, pitch
        big_a, big_b, self.copy = self.alloc(self.BIG), self.alloc(self.BIG), self.alloc(self.size)
        for _ in range(16):
            self.ok(self.hip.hipMemcpyAsync(big_b, big_a, C.c_size_t(self.BIG), 3, self.stream))
        self.ok(self.hip.hipMemcpyAsync(self.copy, C.c_void_p(ptr), C.c_size_t(self.size), 3,
                                        self.stream))

    def copied(self, w, h):
        """what the copy read: h rows of w rgba8 texels"""
        self.ok(self.hip.hipStreamSynchronize(self.stream))
        out = np.empty((h, self.pitch), np.uint8)
        self.ok(self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.copy,
                                   C.c_size_t(self.size), 2))
        return out[:, :w * 4]

    def close(self):
        self.hip.hipStreamSynchronize(self.stream)
        for ptr in self.mem:
            self.hip.hipFree(ptr)
        self.hip.hipStreamDestroy(self.stream)


@pytest.mark.parametrize("resize", [False, True], ids=["same-size", "resized"])
def test_release_with_a_stream_keeps_the_image_until_the_consumers_copy_has_read_it(gpu, resize):
    """the next frame goes into the released slot -- rendered into the same image, or (after a
    resize) into a new one for which the old one is freed: either way the consumer's copy, queued
    before the release, reads what was there"""
    consumer = BusyConsumer()
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8", num_images=2)
    try:
        produce(gpu, sw, COLOURS[0])
        produce(gpu, sw, COLOURS[1])
        a, b = take(sw), take(sw)       # b stays held: the next frame can only go into a's slot
        old = tex_addr(a.tex)
        before = sw.texture(a.tex).download()
        consumer.copy_out_later(sw.texture(a.tex))
        sw.release(a.tex, consumer.stream)

        size = (33, 17) if resize else (W, H)
        if resize:
            assert sw.resize(*size) == (True, *size)
        f = sw.start_frame()
        assert f is not None
        assert (f.fbo.contents.params.w, f.fbo.contents.params.h) == size
        if not resize:
            assert tex_addr(f.fbo) == old
        clear_frame(gpu, f, COLOURS[2])
        assert sw.submit_frame()
        sw.swap_buffers()
        c = take(sw)
        assert tex_addr(c.tex) == tex_addr(f.fbo)
        assert np.array_equal(sw.texture(c.tex).download()[0, 0], [0, 0, 255, 255])

        assert consumer.copied(W, H).tobytes() == before.tobytes()
        sw.release(c.tex)
        sw.release(b.tex)
    finally:
        consumer.close()
        sw.destroy()


# ---- 8. two threads ----------------------------------------------------------------------------
def test_producer_and_consumer_threads(gpu):
    frames = 32
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8", host_readback=True)
    got, problems, stop = [], [], threading.Event()

    def consumer():
        try:
            while len(got) < frames and not stop.is_set():
                p = sw.acquire(TIMEOUT)
                if p is None:
                    problems.append("acquire timed out")
                    return
                got.append((p.seq, int(sw.host_image(p)[H - 1, W - 1, 0])))
                sw.release(p.tex)
        except Exception as e:  # noqa: BLE001
            problems.append(repr(e))

    t = threading.Thread(target=consumer, daemon=True)
    t.start()
    try:
        for i in range(frames):
            deadline = time.monotonic() + 2
            f = sw.start_frame()
            while f is None and t.is_alive() and time.monotonic() < deadline:
                f = sw.start_frame()    # (never blocks: the consumer gets the time)
            assert f is not None, (i, problems)
            clear_frame(gpu, f, (i / 255, 0, 0, 1))
            assert sw.submit_frame()
            sw.swap_buffers()
        t.join(timeout=2)
        assert not t.is_alive() and not problems, problems
        assert got == [(i, i) for i in range(frames)]
    finally:
        stop.set()
        t.join(timeout=2)   # (its acquire returns within its own 2 s; the swapchain outlives it)
        if not t.is_alive():
            sw.destroy()


# ---- 9. misuse ---------------------------------------------------------------------------------
def test_misuse_is_reported_and_survived(gpu):
    sw = pl.Swapchain(gpu, W, H, fmt="rgba8")
    other = gpu.tex_create(W, H, "rgba8")
    fbo = produce(gpu, sw, COLOURS[0])
    n = len(gpu.messages)
    sw.release(other.ptr)                   # not of this swapchain
    assert [lev for lev, _ in gpu.messages[n:]] == [ERR], gpu.messages[n:]
    sw.release(C.cast(C.c_void_p(fbo), C.POINTER(capi.Tex)))    # presented, not held
    assert [lev for lev, _ in gpu.messages[n:]] == [ERR, ERR]
    p = take(sw)
    sw.release(p.tex)
    sw.release(p.tex)                       # released already
    assert [lev for lev, _ in gpu.messages[n:]] == [ERR, ERR, ERR]
    assert all("pl_hip_swapchain_release" in m for _, m in gpu.messages[n:])

    produce(gpu, sw, COLOURS[1])
    assert take(sw) is not None             # ... and never released
    n = len(gpu.messages)
    sw.destroy()
    said = gpu.messages[n:]
    assert [lev for lev, _ in said] == [WARN] and "held" in said[0][1], said
    other.destroy()
