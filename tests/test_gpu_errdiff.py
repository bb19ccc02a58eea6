"""Error diffusion (pl_shader_error_diffusion) on the GPU against the oracle: integer error
transport + a handful of exactly rounded float ops -> bit-exact. (The oracle itself is held to a
raster-order restatement of the shader, without shear, ring or packed word, in
tests/test_second_opinion.py. The renderer's use of the stage: tests/test_gpu_errdiff_render.py.)"""
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util

pytestmark = pytest.mark.gpu

KERNELS = ["simple", "false-fs", "sierra-lite", "floyd-steinberg", "atkinson",
           "jarvis-judice-ninke", "stucki", "burkes", "sierra-2", "sierra-3"]


def kernel_of(name):
    k = pl.lib().pl_find_error_diffusion_kernel(name.encode())
    assert k, name
    k = k.contents
    return k.shift, k.divisor, [[k.pattern[y][x] for x in range(5)] for y in range(3)]


def diffuse(gpu, data, src_fmt, dst_fmt, depth, name):
    """`data` (the host layout of src_fmt) through k_errdiff into a dst_fmt texture -> what was
    stored, and what the oracle says should have been: (got, want)"""
    h, w = data.shape[:2]
    src = gpu.tex_create(w, h, src_fmt, data)
    dst = gpu.tex_create(w, h, dst_fmt)
    try:
        sh = gpu.begin()
        assert sh.error_diffusion(src, dst, depth, name), gpu.messages[-3:]
        assert sh.compute(), gpu.messages[-3:]
        got = dst.download()
    finally:
        src.destroy(); dst.destroy()
    ref = orc.error_diffusion(orc.tex_decode(data, src_fmt), depth, *kernel_of(name))
    return got, orc.tex_encode(ref, dst_fmt)


def same(got, want, what=None):
    """bit for bit (floats compared as their words)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    if got.dtype.kind == "f":
        got, want = (a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) for a in (got, want))
    assert np.array_equal(got, want), (what, util.diff_stats(got, want))


def float_image(w, h, fmt, lo=0.0, hi=1.0, seed=1):
    """random values in [lo, hi] in the host layout of a float format"""
    dt, nc = pl._FMT_DTYPES[fmt]
    return (lo + (hi - lo) * np.random.default_rng(seed).random((h, w, nc))).astype(dt)


@pytest.mark.parametrize("name", KERNELS)
def test_error_diffusion_bit_exact(gpu, name):
    w, h, depth = 96, 70, 4
    img = util.chirp_rgba16(w, h)
    src = gpu.tex_create(w, h, "rgba16", img)
    dst = gpu.tex_create(w, h, "rgba16")
    sh = gpu.begin()
    assert sh.error_diffusion(src, dst, depth, name), gpu.messages[-3:]
    assert sh.compute(), gpu.messages[-3:]
    got = dst.download()
    shift, divisor, pattern = kernel_of(name)
    ref = orc.error_diffusion(orc.tex_decode(img, "rgba16"), depth, shift, divisor, pattern)
    ref16 = orc.tex_encode(ref, "rgba16")
    assert np.array_equal(got, ref16), util.diff_stats(got, ref16)
    # it is a dither: every value is a multiple of 1/15, mean is preserved
    q = orc.tex_decode(got, "rgba16")[..., :3] * 15
    assert np.abs(q - np.round(q)).max() < 1e-3
    assert abs(q.mean() / 15 - orc.tex_decode(img, "rgba16")[..., :3].mean()) < 2e-3
    src.destroy(); dst.destroy()


@pytest.mark.parametrize("h", [1100, 2160])
def test_error_diffusion_tall_frames_multi_step(gpu, h):
    """height > 1024: several sequential steps per sheared column; 2160 rows needs > 64 KiB of
    LDS with a 3-row kernel (the case the reference downgrades to ordered dither)."""
    w, depth = 48, 8
    img = util.random_rgba16(w, h, seed=h)
    src = gpu.tex_create(w, h, "rgba16", img)
    dst = gpu.tex_create(w, h, "rgba16")
    sh = gpu.begin()
    assert sh.error_diffusion(src, dst, depth, "sierra-3"), gpu.messages[-3:]
    assert sh.compute(), gpu.messages[-3:]
    got = dst.download()
    shift, divisor, pattern = kernel_of("sierra-3")
    ref = orc.tex_encode(orc.error_diffusion(orc.tex_decode(img, "rgba16"), depth, shift, divisor,
                                             pattern), "rgba16")
    assert np.array_equal(got, ref), util.diff_stats(got, ref)
    src.destroy(); dst.destroy()


def test_error_diffusion_shmem_req(gpu):
    k = pl.lib().pl_find_error_diffusion_kernel(b"sierra-lite")
    shift, divisor, pattern = kernel_of("sierra-lite")
    cols = 1 + max(dx - 2 + dy * shift for dy in range(3) for dx in range(5) if pattern[dy][dx])
    assert pl.lib().pl_error_diffusion_shmem_req(k, 1080) == (1080 + 2) * cols * 4


# What shapes the launch: block_size = min(1024, height), down to a one-lane workgroup for a single
# row; widths narrower than a pattern's reach to the left (the guard "dx < 0 && x < -dx") and to the
# right; heights at and just over the 1024 lanes of the workgroup, where a sheared column takes more
# than one step and the last step of the frame is a partial one. (width, height)
EDGE_SIZES = [(1, 1), (1, 9), (2, 3), (3, 1), (4, 2), (64, 1), (5, 2), (7, 3),
              (5, 1023), (5, 1024), (5, 1025), (3, 2049)]


@pytest.mark.parametrize("name", KERNELS)
def test_block_size_and_border_edges(gpu, name):
    for i, (w, h) in enumerate(EDGE_SIZES):
        got, want = diffuse(gpu, util.random_rgba16(w, h, seed=100 + i), "rgba16", "rgba16", 8, name)
        same(got, want, (w, h))


@pytest.mark.parametrize("name", ["floyd-steinberg", "stucki"])      # two rows, three rows
@pytest.mark.parametrize("depth", [1, 2, 6, 8, 10, 12, 16])
def test_depths(gpu, name, depth):
    img = util.random_rgba16(33, 17, seed=depth)
    got, want = diffuse(gpu, img, "rgba16", "rgba16", depth, name)
    same(got, want)
    # on the depth's grid, as far as the container's own rounding (half a code of 16 bits) lets
    # a level be told; the shallow depths use every level
    quant = (1 << depth) - 1
    q = orc.tex_decode(got, "rgba16")[..., :3].astype(np.float64) * quant
    assert np.abs(q - np.rint(q)).max() <= 0.5 * quant / 65535 + 1e-4
    if depth <= 6:
        assert len(np.unique(np.rint(q))) == 1 << depth


@pytest.mark.parametrize("name", ["sierra-lite", "floyd-steinberg", "stucki"])   # one of each shift
@pytest.mark.parametrize("src_fmt,dst_fmt", [("rgba16hf", "rgba16hf"), ("rg16hf", "rg16hf"),
                                             ("r16hf", "r16hf"), ("rgba32f", "rgba32f"),
                                             ("rgba16", "rgba8"), ("rgba8", "rgba8")])
def test_formats(gpu, name, src_fmt, dst_fmt):
    """The half-float formats are the renderer's intermediates (four / two / one component): the
    components a format lacks read as 0, 0, 1, are diffused like any other value (0 stays 0) and
    only the format's own components are stored. Alpha is carried, never diffused."""
    w, h, depth = 37, 21, 6
    dt, nc = pl._FMT_DTYPES[src_fmt]
    if dt in (np.float16, np.float32):
        img = float_image(w, h, src_fmt, seed=nc)
    else:
        img = np.random.default_rng(nc).integers(0, np.iinfo(dt).max + 1, (h, w, nc)).astype(dt)
    got, want = diffuse(gpu, img, src_fmt, dst_fmt, depth, name)
    same(got, want)
    back = orc.tex_decode(got, dst_fmt)
    if nc == 4:
        # a non-constant alpha, untouched (through the destination's own rounding)
        assert len(np.unique(img[..., 3])) > 16
        alpha = orc.tex_encode(orc.tex_decode(img, src_fmt), dst_fmt)[..., 3]
        assert np.array_equal(got[..., 3], alpha)
    else:
        assert np.all(back[..., nc:3] == 0) and np.all(back[..., 3] == 1)
    # every stored value is a level of the depth, to the destination's own rounding of a value in
    # [0, 1]: half an ulp of a half float (2^-11 relative), half a code of 8 bits, half an ulp of fp32
    quant = (1 << depth) - 1
    rounding = 2.0 ** -11 if dst_fmt.endswith("hf") else 0.5 / 255 if dst_fmt == "rgba8" else 2.0 ** -24
    q = back[..., :min(nc, 3)].astype(np.float64) * quant
    assert np.abs(q - np.rint(q)).max() <= quant * rounding * 1.01


@pytest.mark.parametrize("dst_fmt", ["rgba16hf", "rgba16"])
def test_out_of_range_sources(gpu, dst_fmt):
    """A float source outside [0, 1]: the shader clamps nothing, so a float destination receives
    levels below 0 and above 1; a unorm destination clamps in its store, and only there."""
    img = float_image(41, 23, "rgba16hf", lo=-0.25, hi=1.5, seed=3)
    got, want = diffuse(gpu, img, "rgba16hf", dst_fmt, 5, "burkes")
    same(got, want)
    if dst_fmt == "rgba16hf":
        assert got[..., :3].min() < -0.2 and got[..., :3].max() > 1.4
    else:
        assert (got[..., :3] == 0).mean() > 0.1 and (got[..., :3] == 65535).mean() > 0.2


def tallest_that_fits(kernel_name, limit):
    """the tallest frame whose error ring (pl_error_diffusion_shmem_req) fits `limit` bytes"""
    k = pl.lib().pl_find_error_diffusion_kernel(kernel_name.encode())
    req = lambda h: pl.lib().pl_error_diffusion_shmem_req(k, h)
    row = req(2) - req(1)
    h = (limit - req(0)) // row
    assert req(h) <= limit < req(h + 1)
    return h, req(h)


@pytest.mark.parametrize("name", ["stucki", "jarvis-judice-ninke"])
def test_largest_ring_the_device_holds(gpu, name):
    """The ring of a nine-column kernel at the tallest height that fits the 160 KiB of LDS: 36
    bytes per row, two rows of padding -> 4549 rows, four bytes short of the limit. One row more
    is refused when the shader is recorded (pl_shader_error_diffusion returns false, the shader is
    failed), not when it is launched."""
    limit = gpu.gpu.contents.glsl.max_shmem_size
    assert limit == 160 * 1024
    h, need = tallest_that_fits(name, limit)
    assert (h, need) == (4549, (4549 + 2) * 36) and need == 163836
    got, want = diffuse(gpu, util.random_rgba16(8, h, seed=h), "rgba16", "rgba16", 8, name)
    same(got, want)

    src = gpu.tex_create(8, h + 1, "rgba16")
    dst = gpu.tex_create(8, h + 1, "rgba16")
    sh = gpu.begin()
    n = len(gpu.messages)
    assert not sh.error_diffusion(src, dst, 8, name)
    assert sh.failed()
    assert any("insufficient" in m for _, m in gpu.messages[n:]), gpu.messages[n:]
    sh.abort()
    src.destroy(); dst.destroy()
