"""Asynchronous frame I/O: buffers imported from host pointers (PL_HANDLE_HOST_PTR), completion
polled per buffer, deferred transfer callbacks.

(a) the import contract, after the reference's pl_test_host_ptr (src/tests/gpu_tests.c:1797-1835);
(b) imported buffer -> texture -> imported buffer for plain and emulated formats, on both
    instances of the conversion kernels, with a sub-rectangle, a padded pitch and an offset: the
    bytes inside the rect arrive, every byte outside it stays as it was;
(c) none of this drains the stream (plh_test_stream_syncs), while `ptr` transfers do;
(d) callbacks: in order, once each, not before the data is in place, re-entrant, 80 pending;
(e) a buffer destroyed with its transfer pending;
(f) frames that enter through pl_upload_plane(.buf) and leave through an imported buffer are
    bit-identical to the same frames through `ptr` transfers, async_measure on and off."""
import ctypes as C
import mmap

import numpy as np
import pytest

import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi

pytestmark = pytest.mark.gpu

PAGE = mmap.PAGESIZE
ERR, WARN = 2, 3


def aligned(nbytes, fill=None):
    """a page-aligned uint8 array (a view that keeps its allocation alive)"""
    raw = np.empty(nbytes + PAGE, np.uint8)
    off = -raw.ctypes.data % PAGE
    a = raw[off:off + nbytes]
    assert a.ctypes.data % PAGE == 0
    if fill is not None:
        a[:] = fill
    return a


def errors(gpu):
    return sum(1 for lvl, _ in gpu.messages if lvl == ERR)


def refused(gpu, make):
    """`make()` returns nothing and the library said why"""
    before = errors(gpu)
    got = make()
    assert not got, "accepted"
    assert errors(gpu) > before, "refused without a message"


# ---- (a) ---------------------------------------------------------------------------------------
def test_import_contract(gpu):
    g = gpu.gpu.contents
    assert g.limits.callbacks is True
    assert g.limits.align_host_ptr == PAGE
    assert g.limits.max_mapped_size == 0        # (buffers the backend allocates)
    assert g.import_caps.buf == capi.HANDLE_HOST_PTR
    assert g.import_caps.tex == 0 and g.import_caps.sync == 0
    assert (g.export_caps.tex, g.export_caps.buf, g.export_caps.sync) == (0, 0, 0)

    # the reference's pl_test_host_ptr: a 64 KiB slice at 2 KiB in a page-aligned 2 MiB block
    # (its constants: size = 2 << 20, offset = 2 << 10, slice = 2 << 16)
    size, offset, slice_ = 2 << 20, 2 << 10, 2 << 16
    block = aligned(size)
    block[:] = np.arange(size, dtype=np.uint32).astype(np.uint8)
    warned = lambda: sum(1 for lvl, m in gpu.messages if lvl == WARN and "not page-aligned" in m)
    w0 = warned()
    buf = gpu.buf_import(block, offset=offset, size=slice_, host_mapped=True)
    assert buf, gpu.messages[-3:]
    assert buf.data == block.ctypes.data + offset
    got = np.ctypeslib.as_array(C.cast(buf.data, C.POINTER(C.c_uint8)), (slice_,))
    assert np.array_equal(got, block[offset:offset + slice_])
    assert buf.device_ptr()
    assert buf.poll(0) is False                 # never used: not busy
    assert warned() == w0                       # aligned: nothing to round
    buf.destroy()

    # what is refused, each with a message; nothing stays registered (see the import below)
    refused(gpu, lambda: gpu.buf_import(block, size=4096, uniform=True))
    refused(gpu, lambda: gpu.buf_import(block, size=4096, storable=True))
    refused(gpu, lambda: gpu.buf_import(block, offset=size - 100, size=200))
    refused(gpu, lambda: gpu.buf_import(block, size=4096, handle=capi.HANDLE_FD))
    refused(gpu, lambda: gpu.buf_import(block, size=4096,
                                        handle=capi.HANDLE_FD | capi.HANDLE_HOST_PTR))
    refused(gpu, lambda: gpu.buf_create(capi.BufParams(size=4096, export_handle=capi.HANDLE_FD)))
    refused(gpu, lambda: gpu.buf_create(capi.BufParams(size=4096,
                                                       export_handle=capi.HANDLE_HOST_PTR)))
    refused(gpu, lambda: gpu.buf_create(capi.BufParams(size=64, host_mapped=True)))
    tp = capi.TexParams(w=16, h=16, format=gpu.fmt("rgba8"), sampleable=True, host_writable=True,
                        import_handle=capi.HANDLE_HOST_PTR)
    tp.shared_mem.handle = block.ctypes.data
    tp.shared_mem.size = size
    refused(gpu, lambda: pl.lib().pl_tex_create(gpu.gpu, C.byref(tp)))
    tp.import_handle, tp.export_handle = 0, capi.HANDLE_FD
    refused(gpu, lambda: pl.lib().pl_tex_create(gpu.gpu, C.byref(tp)))

    # a pointer at +24 imports: rounded to pages, with ONE warning per process
    odd = block[24:24 + 3 * PAGE]
    buf = gpu.buf_import(odd, host_readable=True, host_writable=True)
    assert buf, gpu.messages[-3:]
    assert buf.data == block.ctypes.data + 24 and buf.size == 3 * PAGE
    assert warned() == w0 + 1
    buf.destroy()
    buf = gpu.buf_import(block[40:40 + PAGE])
    assert buf, gpu.messages[-3:]
    assert warned() == w0 + 1
    buf.destroy()
    del block                                   # the caller's memory, freed by the caller


# ---- (b) ---------------------------------------------------------------------------------------
TEXEL_SIZE = {"r8": 1, "rg16": 4, "rgba16": 8, "rgba32f": 16, "bgra8": 4, "rgb10a2": 4, "bgr10a2": 4}
SHAPES = [("r8", 13, 8), ("rg16", 16, 8), ("rgba16", 16, 8), ("rgba32f", 16, 8),
          ("bgra8", 5, 8), ("bgra8", 64, 8), ("rgb10a2", 5, 8), ("rgb10a2", 64, 8),
          ("bgr10a2", 5, 8), ("bgr10a2", 64, 8)]


def layout(mode, fmt, w, h):
    """(rect, row_pitch, buf_offset) of one round trip"""
    tsz = TEXEL_SIZE[fmt]
    if mode == "aligned":       # bases and pitches multiples of 16: the kernels' 16-byte instance
        return (0, 0, w, h), -(-w * tsz // 16) * 16, 0
    if mode == "offset4":       # tight rows 4 bytes into the buffer: the per-texel instance
        return (0, 0, w, h), w * tsz, 4
    rect = (1, 2, w - 1, h - 1)  # "subrect": padded pitch, offset
    return rect, (rect[2] - rect[0] + 3) * tsz, 4 * tsz


@pytest.fixture(scope="module")
def io_bufs(gpu):
    """one imported source and one imported destination block, shared by the round trips"""
    src, dst = aligned(64 << 10), aligned(64 << 10)
    src[:] = np.random.default_rng(7).integers(0, 256, src.size, dtype=np.uint8)
    bs = gpu.buf_import(src, host_writable=True)
    bd = gpu.buf_import(dst, host_readable=True)
    assert bs and bd, gpu.messages[-3:]
    yield src, dst, bs, bd
    bs.destroy()
    bd.destroy()


def expected(src, rect, pitch, offset, tsz):
    want = np.full(src.size, 0xA5, np.uint8)
    row = (rect[2] - rect[0]) * tsz
    for r in range(rect[3] - rect[1]):
        a = offset + r * pitch
        want[a:a + row] = src[a:a + row]
    return want


@pytest.mark.parametrize("mode", ["aligned", "offset4", "subrect"])
@pytest.mark.parametrize("fmt,w,h", SHAPES)
def test_round_trip(gpu, io_bufs, fmt, w, h, mode):
    src, dst, bs, bd = io_bufs
    rect, pitch, offset = layout(mode, fmt, w, h)
    tex = gpu.tex_create(w, h, fmt)
    dst[:] = 0xA5
    assert tex.upload_from(bs, rect=rect, row_pitch=pitch, buf_offset=offset), gpu.messages[-3:]
    assert tex.download_to(bd, rect=rect, row_pitch=pitch, buf_offset=offset), gpu.messages[-3:]
    assert bd.poll(pl.POLL_FOREVER) is False
    want = expected(src, rect, pitch, offset, TEXEL_SIZE[fmt])
    bad = np.flatnonzero(dst != want)
    assert bad.size == 0, (fmt, mode, bad[:8], dst[bad[:8]], want[bad[:8]])
    assert bs.poll(0) is False                  # its upload was queued before the download
    tex.destroy()


# ---- (c) ---------------------------------------------------------------------------------------
def test_no_drains(gpu, io_bufs):
    src, dst, bs, bd = io_bufs
    w, h = 16, 8
    tex = gpu.tex_create(w, h, "rgba16")
    ran = []
    before = gpu.stream_syncs()
    for i in range(8):
        dst[:] = 0xA5
        assert tex.upload_from(bs, buf_offset=256 * i, callback=lambda i=i: ran.append(("ul", i)))
        assert tex.download_to(bd, callback=lambda i=i: ran.append(("dl", i)))
        bd.poll(0)
        assert bd.poll(pl.POLL_FOREVER) is False
        assert np.array_equal(dst[:w * h * 8], src[256 * i:256 * i + w * h * 8])
    gpu.flush()
    assert gpu.stream_syncs() == before, "an imported-buffer round trip drained the stream"
    gpu.finish()                                # (whatever callback was still waiting for its fence)
    assert ran == [(k, i) for i in range(8) for k in ("ul", "dl")]

    # the same through `ptr` without callbacks: each transfer has to drain
    before = gpu.stream_syncs()
    for i in range(8):
        img = src[256 * i:256 * i + w * h * 8].view(np.uint16).reshape(h, w, 4)
        tex.upload(img)
        assert np.array_equal(tex.download(), img)
    assert gpu.stream_syncs() - before >= 16
    tex.destroy()


# ---- (d) ---------------------------------------------------------------------------------------
def test_callbacks(gpu, io_bufs):
    src, dst, bs, bd = io_bufs
    w, h = 16, 4
    nbytes = w * h * 8                          # 512 bytes per transfer: 80 fit the 64 KiB block
    tex = gpu.tex_create(w, h, "rgba16")
    dst[:] = 0xA5
    assert tex.upload_from(bs)

    # 80 pending downloads, more than the queue holds: each callback looks at its own bytes
    order, intact = [], []

    def done(i):
        order.append(i)
        intact.append(bool(np.array_equal(dst[i * nbytes:(i + 1) * nbytes], src[:nbytes])))

    for i in range(80):
        assert tex.download_to(bd, buf_offset=i * nbytes, callback=lambda i=i: done(i))
    gpu.finish()
    assert order == list(range(80)), order      # FIFO, each exactly once, all after pl_gpu_finish
    assert all(intact), [i for i, ok in enumerate(intact) if not ok]
    assert not gpu._callbacks                   # every C callback has run

    # a `ptr` transfer is complete on return, as ever, and so is its callback -- behind the one
    # queued before it
    out = np.zeros((h, w, 4), np.uint16)
    seen = []
    xp = capi.TexTransferParams(tex=tex.ptr, ptr=out.ctypes.data)
    xp.callback = C.cast(gpu.transfer_callback(
        lambda: seen.append(bool(np.array_equal(out.view(np.uint8).ravel(), src[:nbytes])))),
        C.c_void_p)
    assert tex.download_to(bd, callback=lambda: seen.append("buf"))
    assert pl.lib().pl_tex_download(gpu.gpu, C.byref(xp))
    assert seen == ["buf", True]

    # a callback that destroys its buffer and starts another transfer
    mem_x, mem_y = aligned(PAGE, 0xA5), aligned(PAGE, 0xA5)
    bx = gpu.buf_import(mem_x, host_readable=True)
    by = gpu.buf_import(mem_y, host_readable=True)
    assert bx and by
    log = []

    def first():
        log.append(("first", bool(np.array_equal(mem_x[:nbytes], src[:nbytes]))))
        bx.destroy()
        ok = tex.download_to(by, callback=lambda: log.append(
            ("second", bool(np.array_equal(mem_y[:nbytes], src[:nbytes])))))
        log.append(("started", bool(ok)))

    assert tex.download_to(bx, callback=first)
    gpu.finish()
    assert log == [("first", True), ("started", True), ("second", True)], log
    assert bx.ptr is None
    by.destroy()
    tex.destroy()


# ---- (e) ---------------------------------------------------------------------------------------
def test_destroy_with_a_transfer_pending(gpu):
    w, h = 64, 64
    img = util.chirp_rgba16(w, h)
    tex = gpu.tex_create(w, h, "rgba16", img)
    mem = aligned(w * h * 8, 0xA5)
    buf = gpu.buf_import(mem, host_readable=True)
    assert buf
    before = gpu.stream_syncs()
    assert tex.download_to(buf)
    buf.destroy()                               # waits for its own transfer, and only for that
    assert gpu.stream_syncs() == before
    assert np.array_equal(mem.view(np.uint16).reshape(h, w, 4), img)
    del mem                                     # the block is the caller's to free
    tex.destroy()


# ---- buffer operations on an import; the copy stream --------------------------------------------
def test_buffer_operations_on_imports(gpu):
    """pl_buf_write / pl_buf_read (fence wait + memcpy), initial_data, pl_buf_copy through the
    device alias (import -> ordinary buffer -> import), and a poll with a finite timeout"""
    L = pl.lib()
    n = 8192
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    mem_a, mem_b = aligned(n, 0xA5), aligned(n, 0xA5)
    a = gpu.buf_import(mem_a, host_readable=True, host_writable=True,
                       initial_data=data.ctypes.data)
    b = gpu.buf_import(mem_b, host_readable=True, host_writable=True)
    mid = gpu.buf_create(capi.BufParams(size=n, host_readable=True, host_writable=True))
    assert a and b and mid, gpu.messages[-3:]
    assert np.array_equal(mem_a, data)                  # initial_data lands in the caller's memory

    patch = rng.integers(0, 256, 512, dtype=np.uint8)
    L.pl_buf_write(gpu.gpu, a.ptr, 1024, patch.ctypes.data, patch.size)
    data[1024:1536] = patch
    assert np.array_equal(mem_a, data)
    back = np.zeros(n, np.uint8)
    assert L.pl_buf_read(gpu.gpu, a.ptr, 0, back.ctypes.data, n)
    assert np.array_equal(back, data)

    before = gpu.stream_syncs()
    L.pl_buf_copy(gpu.gpu, mid.ptr, 0, a.ptr, 0, n)             # import -> device
    L.pl_buf_copy(gpu.gpu, b.ptr, 256, mid.ptr, 256, n - 512)   # device -> import, inside it
    busy = b.poll(2_000_000_000)                        # finite: asks and yields, at most 2 s
    assert busy is False and a.poll(0) is False
    assert gpu.stream_syncs() == before
    want = np.full(n, 0xA5, np.uint8)
    want[256:n - 256] = data[256:n - 256]
    assert np.array_equal(mem_b, want)
    assert L.pl_buf_read(gpu.gpu, mid.ptr, 0, back.ctypes.data, n) and np.array_equal(back, data)
    assert not L.pl_gpu_is_failed(gpu.gpu)
    for x in (a, b, mid):
        x.destroy()


def test_download_beside_the_next_write(gpu):
    """A download into an imported buffer runs beside what is queued next. What is queued next
    here overwrites the texture, and then reads the buffer: the download must have seen the old
    picture, the upload out of the buffer the downloaded one. 8 MB a transfer, so that "beside"
    is long enough to go wrong."""
    w = h = 1024
    nbytes = w * h * 8
    rng = np.random.default_rng(5)
    old = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
    new = rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
    mem_new, mem_1, mem_2 = aligned(nbytes), aligned(nbytes, 0xA5), aligned(nbytes, 0xA5)
    mem_new[:] = new.view(np.uint8).ravel()
    b_new = gpu.buf_import(mem_new, host_writable=True)
    b1 = gpu.buf_import(mem_1, host_readable=True, host_writable=True)
    b2 = gpu.buf_import(mem_2, host_readable=True)
    assert b_new and b1 and b2, gpu.messages[-3:]
    tex = gpu.tex_create(w, h, "rgba16", old)
    other = gpu.tex_create(w, h, "rgba16")
    before = gpu.stream_syncs()
    for _ in range(3):
        assert tex.download_to(b1)              # the old picture ...
        assert tex.upload_from(b_new)           # ... overwritten at once
        assert other.upload_from(b1)            # the buffer read back behind its download
        assert other.download_to(b2)
        black = (C.c_float * 4)(0, 0, 0, 0)
        pl.lib().pl_tex_clear(gpu.gpu, other.ptr, black)    # ... and `other` overwritten too
        assert b2.poll(pl.POLL_FOREVER) is False and b1.poll(pl.POLL_FOREVER) is False
        assert np.array_equal(mem_1.view(np.uint16).reshape(h, w, 4), old)
        assert np.array_equal(mem_2.view(np.uint16).reshape(h, w, 4), old)
        assert tex.download_to(b1)
        assert b1.poll(pl.POLL_FOREVER) is False
        assert np.array_equal(mem_1.view(np.uint16).reshape(h, w, 4), new)
        mem_1[:] = 0xA5
        mem_2[:] = 0xA5
        tex.upload(old)                        # (a `ptr` upload: waits for the stream)
    assert gpu.stream_syncs() - before == 3     # the three `ptr` uploads, nothing else
    for x in (b_new, b1, b2, tex, other):
        x.destroy()


def test_frame_loop_tool_runs(gpu):
    """tests/c/bench_io, two frames a leg: both legs run, the ring leg without a drain, every
    callback delivered, and both legs download the same picture"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "c", "build", "bench_io")
    assert os.path.exists(exe), "tests/c/build/bench_io missing: run build()"
    r = subprocess.run([exe, "2", "1", "both"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: ln for ln in r.stdout.splitlines() if ln.strip()}
    assert "sync" in lines and "ms/frame" in lines["sync"], r.stdout
    assert "drains/frame 0.000 " in lines["ring"] and "callbacks 2 + 2 of 2" in lines["ring"], r.stdout
    _, c_sync, c_ring = lines["check"].split()
    assert c_sync == c_ring != "0" * 16, r.stdout


# ---- (f) ---------------------------------------------------------------------------------------
W, H = 64, 48


def yuv420p():
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:H, 0:W]
    luma = (16 + (x * 3 + y * 2) % 220).astype(np.uint8)
    cb = rng.integers(16, 241, (H // 2, W // 2), dtype=np.uint8)
    cr = rng.integers(16, 241, (H // 2, W // 2), dtype=np.uint8)
    return [luma, cb, cr]


def hdr10_rgba16():
    from test_gpu_color import hdr_test_frame
    return (hdr_test_frame(W, H) * 65535 + 0.5).astype(np.uint16)


def plane_in_buf(buf, offset, w, h, comp_bits, comp_map):
    d = capi.PlaneData(type=pl.FMT_UNORM, width=w, height=h,
                       buf=C.cast(buf.ptr, C.c_void_p), buf_offset=offset)
    for c, bits in enumerate(comp_bits):
        d.component_size[c] = bits
        d.component_map[c] = comp_map[c]
    d.pixel_stride = sum(comp_bits) // 8
    return d


def render_frame(g, kind, through_bufs):
    """one frame in, rendered to rgba16 64 x 48, out -- all through `ptr`, or all through
    imported buffers"""
    if kind == "yuv420p":
        planes = [(p, [8], [i]) for i, p in enumerate(yuv420p())]
        repr_, color = pl.color_repr("bt709", "limited"), pl.color_space("bt709", "bt1886")
        params = pl.render_params("default", dither_params=None)
    else:
        planes = [(hdr10_rgba16(), [16, 16, 16, 16], [0, 1, 2, 3])]
        repr_, color = pl.color_repr("rgb", "full"), pl.color_space("bt2020", "pq", max_luma=1000.0)
        params = pl.render_params("default", dither_params=None)

    texs, frame = [], capi.Frame(num_planes=len(planes), repr=repr_, color=color)
    bufs = []
    if through_bufs:
        mem = aligned(64 << 10)
        sbuf = g.buf_import(mem, host_writable=True)
        assert sbuf, g.messages[-3:]
        bufs.append(sbuf)
    offset = 0
    for i, (arr, bits, cmap) in enumerate(planes):
        if through_bufs:
            raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
            mem[offset:offset + raw.size] = raw
            data = plane_in_buf(sbuf, offset, arr.shape[1], arr.shape[0], bits, cmap)
            offset += -(-raw.size // 256) * 256
        else:
            data = pl.plane_data(arr.reshape(arr.shape[0], arr.shape[1], -1), bits, cmap)
        plane, tex = pl.upload_plane(g, data)
        C.memmove(C.byref(frame.planes[i]), C.byref(plane), C.sizeof(capi.Plane))
        texs.append(tex)

    dst = g.tex_create(W, H, "rgba16")
    target = pl.frame(dst, color=pl.color_space("bt709", "bt1886"))
    rr = pl.Renderer(g)
    assert rr.render(frame, target, params), g.messages[-4:]
    assert rr.errors() == 0
    if through_bufs:
        out_mem = aligned(W * H * 8, 0xA5)
        obuf = g.buf_import(out_mem, host_readable=True)
        assert obuf and dst.download_to(obuf)
        assert obuf.poll(pl.POLL_FOREVER) is False
        got = out_mem.view(np.uint16).reshape(H, W, 4).copy()
        bufs.append(obuf)
    else:
        got = dst.download()
    rr.destroy()
    for t in texs + [dst]:
        t.destroy()
    for b in bufs:
        b.destroy()
    return got


@pytest.mark.parametrize("async_measure", [False, True])
@pytest.mark.parametrize("kind", ["yuv420p", "hdr10"])
def test_through_the_renderer(built, kind, async_measure):
    with pl.HipGpu(0, async_measure=async_measure) as g:
        want = render_frame(g, kind, False)
        got = render_frame(g, kind, True)
    assert want.std() > 0                       # a picture, not a constant
    assert np.array_equal(got, want), util.diff_stats(got, want)
