"""The chain epilogue of k_polar_mx, walked one row phase at a time, pinned bit for bit.

k_polar_mx's CHAIN branch (k_polar_mx.hiph) used to contract both row phases of a wave tile and then
walk the lane's row pairs {0, 2}, {1, 3}, {4, 6}, {5, 7}; it now contracts ONE phase, maps its pairs
{0, 2}, {4, 6}, then the other phase's {1, 3}, {5, 7}. Every pixel must see the same sums, the same
dither cell and the same store guard: only the order of the stores may change. A wrong row, dither
row or guard shows in these frames.

The fixtures under tests/golden/chain_row_phase/ were rendered by the library as it stood BEFORE that
change (`python tests/test_gpu_chain_row_phase.py` regenerates them with whatever library is built:
run on that earlier commit it reproduces them byte for byte). Every frame is stored whole, 16 bits
per sample, as a compressed .npz.

Frames (all HDR10 -> bt709 through pl_render_image: EWA-Lanczos 2x, tone + gamut map, blue-noise
dither to 10 bit; BT.1886 unless said otherwise):
  plain_80x45, plain_97x61   -> 160x90 and 194x122: heights that end inside a lane's eight rows and
                             inside a wave tile (90 = 64 + 3 * 8 + 2, 122 = 64 + 32 + 3 * 8 + 2); both
                             also with PL_HIP_CHAIN_SHAPE=0, the generic CHAIN instance, against the
                             same fixtures
  offset_80x45               the target rectangle 3 columns and 5 rows inside a larger target
  crop_97x61                 the source rectangle (2, 3) .. (66, 46): 128x86 pixels, it starts off the
                             tile grid of the plane and ends inside a lane's eight rows
  vflip_80x45                a vertically flipped target (dir_y = -1)
  yramp_80x45                rows that are a ramp in Y, constant along a row: any permutation of rows
                             is visible
  gamma22_80x45, srgb_80x45  the other two target curves that have a shape instance

The launcher's trace line (PL_HIP_PASS_TRACE) must say which instance of the chain took the launch: a
frame that fell back to another kernel fails the test."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import libplacebo_amd as pl
import util
from test_gpu_chain_shape import SHAPE_OF
from test_gpu_fullsize import hdr_frame16
from test_gpu_metric import HDR, metric_params, ten_bit

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_row_phase")


def yramp_frame(w, h):
    """PQ codes that rise from row to row (each channel at its own rate) and do not change along a row"""
    img = np.empty((h, w, 4), np.uint16)
    y = np.arange(h, dtype=np.float64)[:, None]
    img[..., 0] = np.rint(3000 + y * (42000.0 / h))
    img[..., 1] = np.rint(9000 + y * (30000.0 / h))
    img[..., 2] = np.rint(40000 - y * (33000.0 / h))
    img[..., 3] = 65535
    return img


# name -> source, transfer, and (as functions of the source size) the source rectangle, the target's
# size and the target rectangle (None: the whole plane / twice the source / the whole target)
CASES = {
    "plain_80x45": dict(make=lambda: hdr_frame16(80, 45)),
    "plain_97x61": dict(make=lambda: hdr_frame16(97, 61)),
    "offset_80x45": dict(make=lambda: hdr_frame16(80, 45), target=(160 + 7, 90 + 9),
                         target_crop=(3.0, 5.0, 163.0, 95.0)),
    "crop_97x61": dict(make=lambda: hdr_frame16(97, 61), crop=(2.0, 3.0, 66.0, 46.0), target=(128, 86)),
    "vflip_80x45": dict(make=lambda: hdr_frame16(80, 45), target_crop=(0.0, 90.0, 160.0, 0.0)),
    "yramp_80x45": dict(make=lambda: yramp_frame(80, 45)),
    "gamma22_80x45": dict(make=lambda: hdr_frame16(80, 45), transfer="gamma22"),
    "srgb_80x45": dict(make=lambda: hdr_frame16(80, 45), transfer="srgb"),
}
GENERIC_TOO = ["plain_80x45", "plain_97x61"]


def render(gpu, name, env=None):
    case = CASES[name]
    img = case["make"]()
    h, w = img.shape[:2]
    dw, dh = case.get("target", (2 * w, 2 * h))
    env = {"PL_HIP_POLAR_MFMA": "1", "PL_HIP_PASS_TRACE": "1", **(env or {})}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rr = pl.Renderer(gpu)
        src = gpu.tex_create(w, h, "rgba16", img)
        # (a target the frame does not cover keeps what it is created with)
        dst = gpu.tex_create(dw, dh, "rgba16", np.full((dh, dw, 4), 0x1234, np.uint16))
        util.srand(1)
        assert rr.render(pl.frame(src, components=3, color=pl.color_space(**HDR), crop=case.get("crop")),
                         pl.frame(dst, color=pl.color_space("bt709", case.get("transfer", "bt1886")),
                                  repr_=ten_bit(), crop=case.get("target_crop")),
                         metric_params(True)), gpu.messages[-4:]
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


def check(gpu, capfd, name, env, want_line):
    want = np.load(os.path.join(GOLDEN, name + ".npz"))["frame"]
    capfd.readouterr()
    got = render(gpu, name, env)
    lines = [l for l in capfd.readouterr().err.splitlines() if "k_polar_mx chain" in l]
    assert lines, "the chain epilogue of k_polar_mx did not run"
    assert all(l.endswith(want_line) for l in lines), (want_line, lines)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert want[..., :3].std() > 100
    assert np.array_equal(got, want), util.diff_stats(got, want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_frame_is_the_recorded_one(gpu, capfd, name):
    shape = SHAPE_OF[CASES[name].get("transfer", "bt1886")]
    check(gpu, capfd, name, None, "shape %d, specialised instance" % shape)


@pytest.mark.parametrize("name", GENERIC_TOO)
def test_generic_chain_instance_renders_the_same_frame(gpu, capfd, name):
    check(gpu, capfd, name, {"PL_HIP_CHAIN_SHAPE": "0"}, "shape 0, generic instance")


def test_yramp_rows_are_all_different():
    """(what makes a permutation of rows visible: no two source rows of the ramp are alike)"""
    img = yramp_frame(80, 45)
    assert len({row.tobytes() for row in img}) == 45
    assert all((row == row[0]).all() for row in img)


def main():
    """render every frame with the library that is built; write the fixtures (or, with a directory
    as argument, write them there: to compare against the committed ones). The launcher's trace
    lines go to stderr beside the list."""
    import hashlib
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(out, exist_ok=True)
    with pl.HipGpu(0) as gpu:
        for name in sorted(CASES):
            frame = render(gpu, name)
            np.savez_compressed(os.path.join(out, name + ".npz"), frame=frame)
            print("%-16s %s %s sha256 %s" % (name, frame.shape, frame.dtype,
                                             hashlib.sha256(frame.tobytes()).hexdigest()), flush=True)


if __name__ == "__main__":
    main()
