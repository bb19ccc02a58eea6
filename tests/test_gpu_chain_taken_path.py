"""The colour-map chain's frames, pinned bit for bit against recorded frames.

The device functions of the HDR10 -> SDR chain (cmfast.hiph, pqseg.hiph, transfer.hiph, devmath.hiph)
have had instructions removed that their arithmetic does not need: the square root's handling of
tiny arguments, a `+ 0` in front of the target curve, the floor / convert pairs of the table indices,
the copies behind the cubics. None of that may move a bit of any frame.

The fixtures under tests/golden/chain_taken_path/ were rendered by the library as it stood BEFORE
those edits (`python tests/test_gpu_chain_taken_path.py` regenerates them with whatever library
is built: run on that earlier commit it reproduces them byte for byte). Every frame is stored whole,
16 bits per sample, as a compressed .npz.

Frames (all HDR10 -> bt709, blue-noise dither to 10 bit unless said otherwise):
  metric_*        the metric's frame (EWA-Lanczos 2x + map chain, k_polar_mx's shape instances):
                  160x90 -> 320x180 (whole wave tiles and a partial last tile row) and
                  97x61 -> 194x122 (odd: every guard), BT.1886; the odd size also for gamma 2.2 and
                  sRGB (instances 8, 9, 10)
  chirp           the benchmark's chirp scaled by 0.75, without the highlights hdr_frame16 adds
  grey            R = G = B ramps: P and T next to 0, the square root at tiny arguments, atan2(0, 0)
  dark            exact 0 and codes below PQ 1/64: the EOTF's fine tier, +-0 into the target curve
  beyond_*        an rgba16hf source with values up to 1.6: all three closed-form fall-backs run
  mxr             96x54 -> 288x162 (k_polar_mxr, 3x: the generic chain)
  pass_chain      320x180 1:1 tone map into a 16-bit target (k_pass_chain)
"""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import libplacebo_amd as pl
import util
from test_gpu_fullsize import hdr_frame16
from test_gpu_metric import HDR, metric_params, ten_bit

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_taken_path")


def chirp_frame(w, h):
    return np.rint(util.chirp_rgba16(w, h).astype(np.float32) * np.float32(0.75)).astype(np.uint16)


def grey_frame(w, h):
    """rows of grey ramps, each over another range of codes (the full range, the dark end, the
    fine tier) and in another direction"""
    img = np.empty((h, w, 4), np.uint16)
    tops = (49152, 65535, 8192, 1024, 256)
    for y in range(h):
        top = tops[y % len(tops)]
        ramp = np.rint(np.linspace(0, top, w)).astype(np.uint16)
        img[y, :, :3] = (ramp if y & 1 else ramp[::-1])[:, None]
    img[..., 3] = 65535
    return img


def dark_frame(w, h):
    """a third exact black, the rest codes below PQ 1/64 (code 1024), a few brighter texels so that
    the measured peak is not the floor"""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 1024, (h, w, 4)).astype(np.uint16)
    img[rng.random((h, w)) < 1.0 / 3.0, :3] = 0
    img[: h // 4, : w // 4, :3] = 0
    img[h // 2, ::7, :3] = 30000
    img[..., 3] = 65535
    return img


def beyond_frame(w, h):
    """(the frame of test_gpu_chain_shape.py::test_values_beyond_the_cubics)"""
    f16 = hdr_frame16(w, h).astype(np.float32) / 65535.0
    f16[:, : w // 2, :3] *= 1.6 / max(float(f16[..., :3].max()), 1e-3)
    f16 = f16.astype(np.float16)
    assert float(f16[..., :3].max()) > 1.5
    return f16


# name -> (source, scale, transfer, source format, dithered 10-bit target)
CASES = {
    "metric_160x90_bt1886": (lambda: hdr_frame16(160, 90), 2, "bt1886", "rgba16", True),
    "metric_97x61_bt1886": (lambda: hdr_frame16(97, 61), 2, "bt1886", "rgba16", True),
    "metric_97x61_gamma22": (lambda: hdr_frame16(97, 61), 2, "gamma22", "rgba16", True),
    "metric_97x61_srgb": (lambda: hdr_frame16(97, 61), 2, "srgb", "rgba16", True),
    "chirp_160x90": (lambda: chirp_frame(160, 90), 2, "bt1886", "rgba16", True),
    "grey_97x61": (lambda: grey_frame(97, 61), 2, "bt1886", "rgba16", True),
    "dark_97x61": (lambda: dark_frame(97, 61), 2, "bt1886", "rgba16", True),
    "beyond_97x61_bt1886": (lambda: beyond_frame(97, 61), 2, "bt1886", "rgba16hf", True),
    "beyond_97x61_gamma22": (lambda: beyond_frame(97, 61), 2, "gamma22", "rgba16hf", True),
    "beyond_97x61_srgb": (lambda: beyond_frame(97, 61), 2, "srgb", "rgba16hf", True),
    "mxr_96x54": (lambda: hdr_frame16(96, 54), 3, "bt1886", "rgba16", True),
    "pass_chain_320x180": (lambda: hdr_frame16(320, 180), 1, "bt1886", "rgba16", False),
}


def render(gpu, name):
    make, scale, transfer, fmt, dither = CASES[name]
    img = make()
    h, w = img.shape[:2]
    if scale == 1:
        params = pl.render_params("default", peak_detect_params=pl.peak_detect_params(percentile=99.995))
    else:
        params = metric_params(True)
    env = {"PL_HIP_POLAR_MFMA": "1"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rr = pl.Renderer(gpu)
        src = gpu.tex_create(w, h, fmt, img)
        dst = gpu.tex_create(scale * w, scale * h, "rgba16")
        util.srand(1)
        assert rr.render(pl.frame(src, components=3, color=pl.color_space(**HDR)),
                         pl.frame(dst, color=pl.color_space("bt709", transfer),
                                  repr_=ten_bit() if dither else None),
                         params), gpu.messages[-4:]
        assert rr.errors() == 0
        out = dst.download()
        rr.destroy(); src.destroy(); dst.destroy()
        return out
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_is_the_recorded_one(gpu, name):
    want = np.load(os.path.join(GOLDEN, name + ".npz"))["frame"]
    got = render(gpu, name)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert want[..., :3].std() > 100
    assert np.array_equal(got, want), util.diff_stats(got, want)


def main():
    """render every frame with the library that is built; write the fixtures (or, with a directory
    as argument, write them there: to compare against the committed ones)"""
    import hashlib
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(out, exist_ok=True)
    with pl.HipGpu(0) as gpu:
        for name in sorted(CASES):
            frame = render(gpu, name)
            np.savez_compressed(os.path.join(out, name + ".npz"), frame=frame)
            print("%-24s %s %s sha256 %s" % (name, frame.shape, frame.dtype,
                                             hashlib.sha256(frame.tobytes()).hexdigest()))


if __name__ == "__main__":
    main()
