#!/usr/bin/env python3
"""Time a 4K rgba16 SDR frame rendered 1:1 onto a target that carries an sRGB ICC profile
(profiles/icc_frame.md).

  tools/icc_frame.py --mode none|map|icc|icc17|icc129 [--frames N]     one mode, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d <dir> -- python tools/icc_frame.py --mode icc
  tools/icc_frame.py --compare [--frames N] [--rounds R]           host clock around N frames ending
        in a device synchronise, the modes alternating, R rounds

none: no profile (sRGB onto sRGB: nothing to map, the frame is a copy). map: no profile, onto a
BT.2020 / BT.1886 target: the plain colour-map pass (linearise, gamut 3D-LUT, delinearise). icc: the table size pl_icc_open infers for the profile. icc17 / icc129: 17^3 / 129^3.
The profile is lcms2's own sRGB profile (liblcms2.so.2 through ctypes)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libplacebo_amd as pl  # noqa: E402

W, H = 3840, 2160
SIZES = {"icc": (0, 0, 0), "icc17": (17,) * 3, "icc129": (129,) * 3}


def srgb_profile():
    cms = C.CDLL("liblcms2.so.2")
    cms.cmsCreate_sRGBProfile.restype = C.c_void_p
    cms.cmsSaveProfileToMem.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    h = cms.cmsCreate_sRGBProfile()
    n = C.c_uint32(0)
    cms.cmsSaveProfileToMem(h, None, C.byref(n))
    buf = C.create_string_buffer(n.value)
    cms.cmsSaveProfileToMem(h, buf, C.byref(n))
    return buf.raw[:n.value]


class Setup:
    def __init__(self, g, modes):
        rng = np.random.default_rng(1)
        img = rng.integers(0, 65536, (H, W, 4), dtype=np.uint16)
        self.g = g
        self.src = g.tex_create(W, H, "rgba16", img)
        self.dst = g.tex_create(W, H, "rgba16")
        self.rr = {m: pl.Renderer(g) for m in modes}
        data = srgb_profile()
        self.icc = {m: pl.Icc(data, size=SIZES[m]) for m in modes if m in SIZES}
        self.image = pl.frame(self.src, components=3, color=pl.color_space("bt709", "srgb"))
        self.params = pl.render_params("fast", dither_params=None)
        for m, icc in self.icc.items():
            p = icc.params
            print("%s: table %dx%dx%d (%.2f MB)" % (m, p.size_r, p.size_g, p.size_b,
                                                    p.size_r * p.size_g * p.size_b * 8 / 1e6))

    def frames(self, mode, n):
        color = pl.color_space("bt2020", "bt1886") if mode == "map" else pl.color_space("bt709", "srgb")
        target = pl.frame(self.dst, color=color, icc=self.icc.get(mode))
        for _ in range(n):
            assert self.rr[mode].render(self.image, target, self.params), self.g.messages[-3:]
        self.g.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["none", "map"] + list(SIZES))
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    modes = ["none", "map"] + list(SIZES) if a.compare else [a.mode]
    with pl.HipGpu(0) as g:
        s = Setup(g, modes)
        for m in modes:
            s.frames(m, 10)         # warm-up: code objects, the tables
        if not a.compare:
            s.frames(a.mode, a.frames)
            return
        best = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                t0 = time.perf_counter()
                s.frames(m, a.frames)
                best[m].append((time.perf_counter() - t0) / a.frames * 1e6)
        for m in modes:
            v = sorted(best[m])
            print("%-7s %8.1f us / frame (median of %d rounds of %d frames; min %.1f, max %.1f)" %
                  (m, v[len(v) // 2], a.rounds, a.frames, v[0], v[-1]))


if __name__ == "__main__":
    main()
