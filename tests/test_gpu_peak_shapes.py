"""The measuring kernel (k_peak_tiles), pinned word for word and bit for bit.

k_peak_tiles decides what is uniform over a launch -- the clamp in front of the PQ curve, the
PLANE_MAP's component count, the cutoff, the histogram -- once, outside its per-pixel code. None of
that may move a word of the 816-word measurement buffer or a bit of the rgba16hf intermediate.

Every case is measured by k_peak_tiles (the default) and by k_pass_peak (PL_HIP_PEAK_FAST=0: the op
interpreter) in the same build, and compared with what the library recorded BEFORE that change
(tests/golden/peak_shapes/; `python tests/test_gpu_peak_shapes.py` regenerates the fixtures with
whatever library is built: run on that earlier commit it reproduces them byte for byte).

Sizes     16x16 (one tile), 97x61 and 99x59 (odd: the lane whose second texel lies beyond the row,
          partial tiles on both edges), 160x90 (whole tiles across, a partial last row of tiles).
          At 97x61 the launcher takes k_pass_peak itself: the measuring kernels want the pass to
          cover its source exactly, and fp32(1 / 97) * 97 is not 1 (nor fp32(1 / 61) * 61); 99x59
          is the odd size that reaches k_peak_tiles. The trace says which kernel ran.
Sources   c3 / c4     an rgba16 PQ plane sampled with 3 and with 4 components, by hand: sample ->
                      detect_peak -> the intermediate (ops: PEAK_DETECT)
          f16         an rgba16hf linear source (values up to 4), the same way
          plane3      the renderer's own measuring pass of a 3-component rgba16 plane (ops: the
                      identity PLANE_MAP of 3 components, PEAK_DETECT: alpha is the neutral 1);
                      in front of a 2x EWA upscale. The renderer consumes its own buffer: what is
                      compared is the peak and the average it derives from the 816 words (fp32 bits,
                      pl_renderer_get_hdr_metadata) and the frame tone-mapped with them (recorded
                      as its SHA-256), which also stands for the intermediate
Settings  histogram on / off (percentile 99.995 / 100) x cutoff default / 0
Frames    the HDR test frame; `black`: every pixel under the cutoff (codes 0..63), c3 only
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import libplacebo_amd as pl
import util
from libplacebo_amd import _capi as capi
from test_gpu_color import _read_device
from test_gpu_fullsize import hdr_frame16, inferred

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peak_shapes")
SIZES = [(16, 16), (97, 61), (99, 59), (160, 90)]
SOURCES = ["c3", "c4", "f16", "plane3"]
# name -> (percentile, black_cutoff)
SETTINGS = {"hist_cut": (99.995, 1.0), "hist_nocut": (99.995, 0.0),
            "nohist_cut": (100.0, 1.0), "nohist_nocut": (100.0, 0.0)}
HDR = dict(primaries="bt2020", transfer="pq", max_luma=1000.0)


def covers_exactly(n):
    """shaders.c: sh_bind -- the far corner's texture coordinate is fp32(1 / n) * n"""
    return np.float32(1.0 / n) * np.float32(n) == np.float32(1.0)


def black_frame(w, h):
    # (14 bits of PQ x the cutoff's smoothstep come out as 0 below code 83, the bare value above code 4)
    img = np.random.default_rng(3).integers(0, 64, (h, w, 4)).astype(np.uint16)
    img[..., 3] = 65535
    return img


def source_image(source, w, h, black=False):
    img = black_frame(w, h) if black else hdr_frame16(w, h)
    if not black:
        # a dark corner around the cutoff (PQ 0.01 = code 655): its smoothstep, partly black tiles
        rng = np.random.default_rng(5)
        img[: (h + 2) // 3, : (w + 2) // 3, :3] = rng.integers(0, 1400, ((h + 2) // 3, (w + 2) // 3, 3))
    if source == "c4":
        img[..., 3] = rng.integers(0, 65536, (h, w))    # (an alpha that is decoded, not the neutral 1)
    if source == "f16":
        img = (img.astype(np.float32) / 65535.0 * 4.0).astype(np.float16)
    return img


def peak_words(state):
    size_ = C.c_size_t()
    pl.lib().pl_hip_peak_buffer.restype = C.c_void_p
    ptr = pl.lib().pl_hip_peak_buffer(state, C.byref(size_))
    assert ptr and size_.value == 816 * 4
    return _read_device(ptr, size_.value).copy()


def measure(gpu, source, img, setting):
    """-> (the 816 words, the intermediate's f16 codes); plane3: (peak and average, the frame)"""
    h, w = img.shape[:2]
    percentile, cutoff = SETTINGS[setting]
    pp = pl.peak_detect_params(percentile=percentile, black_cutoff=cutoff)
    if source == "plane3":
        rr = pl.Renderer(gpu)
        src = gpu.tex_create(w, h, "rgba16", img)
        dst = gpu.tex_create(2 * w, 2 * h, "rgba16")
        assert rr.render(pl.frame(src, components=3, color=pl.color_space(**HDR)),
                         pl.frame(dst, color=pl.color_space("bt709", "bt1886")),
                         pl.render_params("default", upscaler=pl.filter_config("ewa_lanczos"),
                                          peak_detect_params=pp)), gpu.messages[-4:]
        assert rr.errors() == 0
        meta = capi.HdrMetadata()
        assert pl.lib().pl_renderer_get_hdr_metadata(rr.rr, C.byref(meta))
        buf = np.array([meta.max_pq_y, meta.avg_pq_y], np.float32).view(np.uint32)
        out = dst.download()
        rr.destroy(); src.destroy(); dst.destroy()
        return buf, out
    fmt, trc = ("rgba16hf", "linear") if source == "f16" else ("rgba16", "pq")
    csp, _ = inferred(pl.color_space("bt2020", trc, max_luma=1000.0), pl.color_space("bt709", "bt1886"))
    src = gpu.tex_create(w, h, fmt, img)
    fbo = gpu.tex_create(w, h, "rgba16hf")
    state = pl.ShaderObj()
    a = gpu.begin()
    assert a.sample("direct", src, components=4 if source == "c4" else 3)
    assert pl.lib().pl_shader_detect_peak(a.sh, csp, C.byref(state.slot), C.byref(pp))
    assert a.finish(fbo), gpu.messages[-3:]
    buf = peak_words(state.slot)
    out = fbo.download().view(np.uint16).copy()
    state.destroy(); fbo.destroy(); src.destroy()
    return buf, out


def measure_env(gpu, source, img, setting, env):
    keys = ("PL_HIP_PEAK_FAST", "PL_HIP_PEAK_TILES", "PL_HIP_PASS_TRACE", "PL_HIP_POLAR_MFMA")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ["PL_HIP_POLAR_MFMA"] = "0"   # (plane3's upscale: the sequential-fma kernel, as in the suite)
    os.environ.update(env)
    try:
        return measure(gpu, source, img, setting)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def stored(source, out):
    """what the fixtures hold of `out`: the intermediate itself, the SHA-256 of plane3's frame"""
    if source != "plane3":
        return out
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(out).tobytes()).digest(), np.uint8)


def out_key(key, source, setting):
    # (the intermediate does not depend on the settings: recorded once)
    return "%s/%s/out" % (key, setting) if source == "plane3" else "%s/out" % key


def golden(w, h):
    return np.load(os.path.join(GOLDEN, "%dx%d.npz" % (w, h)))


def check(gpu, capfd, want, key, source, img):
    h, w = img.shape[:2]
    for setting in sorted(SETTINGS):
        capfd.readouterr()
        buf_t, out_t = measure_env(gpu, source, img, setting, {"PL_HIP_PASS_TRACE": "1"})
        kernels = [l.split()[-1] for l in capfd.readouterr().err.splitlines() if l.startswith("[plh] kernel k_p")]
        tiles = covers_exactly(w) and covers_exactly(h)
        assert ("k_peak_tiles" if tiles else "k_pass_peak") in kernels, kernels
        buf_g, out_g = measure_env(gpu, source, img, setting, {"PL_HIP_PEAK_FAST": "0"})
        if source != "plane3":
            assert buf_g[0:12].sum() == (-(-w // 16)) * (-(-h // 16))
        # (a) the interpreter of the same build
        assert np.array_equal(buf_t, buf_g), (setting, np.nonzero(buf_t != buf_g))
        assert np.array_equal(out_t, out_g), (setting, util.diff_stats(out_t, out_g))
        # (b) the recorded words and codes
        assert np.array_equal(buf_t, want["%s/%s/buf" % (key, setting)]), setting
        assert np.array_equal(stored(source, out_t), want[out_key(key, source, setting)]), setting


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("source", SOURCES)
def test_measurement_is_the_recorded_one(gpu, capfd, size, source):
    w, h = size
    want = golden(w, h)
    if source != "plane3":
        assert want["%s/out" % source].any()
        assert want["%s/hist_cut/buf" % source][24:36].sum() > 0
    check(gpu, capfd, want, source, source, source_image(source, w, h))


@pytest.mark.parametrize("size", SIZES)
def test_black_frame(gpu, capfd, size):
    """every pixel under the cutoff: with it no tile is lit and nothing is summed; without it the
    tiles count again"""
    w, h = size
    want = golden(w, h)
    cut, nocut = want["black/hist_cut/buf"], want["black/hist_nocut/buf"]
    assert cut[12:24].sum() == 0 and cut[24:48].sum() == 0 and cut[48:].sum() == 0
    assert nocut[12:24].sum() == nocut[0:12].sum() and nocut[36:48].max() > 0
    check(gpu, capfd, want, "black", "c3", source_image("c3", w, h, black=True))


def test_codes_whose_quotient_is_next_to_a_half(gpu):
    """65455 / 65535 and 65519 / 65535 lie so close to the middle between two f16 numbers that the
    decode's last fma, fused with the conversion into one rounding, lands on the other one. The
    intermediate holds f16(fp32 quotient): both kernels, every channel, either pixel of a lane.
    (Not in the recorded fixtures: the library they were recorded from fused the first channel.)"""
    img = np.random.default_rng(11).choice(np.array([65455, 65519, 65454, 65520], np.uint16), (16, 32, 4))
    want = (img.astype(np.float64) / 65535.0).astype(np.float32).astype(np.float16).view(np.uint16)
    for env in ({}, {"PL_HIP_PEAK_FAST": "0"}):
        _, out = measure_env(gpu, "c4", img, "hist_cut", env)
        assert np.array_equal(out, want), (env, np.argwhere(out != want)[:4])


def main():
    """measure every case with the library that is built; write the fixtures (or, with a directory
    as argument, write them there: to compare against the committed ones)"""
    out_dir = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    with pl.HipGpu(0) as gpu:
        for w, h in SIZES:
            rec = {}
            for key, source, black in [(s, s, False) for s in SOURCES] + [("black", "c3", True)]:
                img = source_image(source, w, h, black)
                for setting in sorted(SETTINGS):
                    buf, out = measure_env(gpu, source, img, setting, {})
                    rec["%s/%s/buf" % (key, setting)] = buf
                    k = out_key(key, source, setting)
                    assert np.array_equal(rec.setdefault(k, stored(source, out)), stored(source, out)), k
            path = os.path.join(out_dir, "%dx%d.npz" % (w, h))
            np.savez_compressed(path, **rec)
            digest = hashlib.sha256(b"".join(rec[k].tobytes() for k in sorted(rec))).hexdigest()
            print("%-12s %3d arrays, %7d bytes, sha256 of the arrays %s" % (os.path.basename(path), len(rec),
                                                                          os.path.getsize(path), digest))


if __name__ == "__main__":
    main()
