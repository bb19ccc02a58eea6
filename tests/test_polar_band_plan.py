"""The launch geometry of k_polar_band (csrc/hip/k_polar_band.hip): polar_band_plan, host
shader_sampling.c, through the plh_test_polar_band_plan hook -- no GPU.

The kernel never holds a tile's footprint whole. It walks the tap list in 2 * bound turns; turn t
covers the tap rows y0 = 1 - bound + t and y0 + 1 and reads, per lane, the "virtual" rows
v = (base row of the lane - lowest base row of the tile) + (tap row + bound - 1) out of a ring of
`ring_rows` rows (slot = v mod ring_rows). Before turn 0 the rows 0 .. span are staged
(span = ring_rows - 2), during turn t the row t + span + 1, with one barrier per turn. This file
restates that walk in Python and holds the plan to it over every ratio the reference renders:
every row and column a lane reads is in the ring, holds the row the lane means, and is not being
overwritten during the turn that reads it."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import libplacebo_amd as pl

LDS_LIMIT = 160 * 1024
SHAPES = ((32, 8), (32, 4), (32, 2), (32, 1), (16, 1))    # the output tiles, widest first
PHASES = (0.0, 0.25, 0.5, 0.999)    # where a tile's first output falls inside its source texel


def plan(fx, fy, bound, texel, limit=LDS_LIMIT):
    """fx, fy: downscale factors (source texels per output); the library's ratios are their inverses"""
    out = (C.c_int * 5)()
    if not pl.lib().plh_test_polar_band_plan(1.0 / fx, 1.0 / fy, bound, texel, limit, out):
        return None
    return tuple(out)


def bases(n, f, phase):
    """base texel floor(pos * size - 0.5) of the n outputs of a tile whose first output lies `phase`
    into its source texel"""
    i = np.arange(n, dtype=np.float64)
    return np.floor(phase + i * f).astype(np.int64)


@functools.lru_cache(maxsize=None)
def columns_fit(f, bound, n, ring_w):
    """every column base + x, x = 1 - bound .. bound, of every lane lies inside a ring row; `est`: the
    kernel's origin comes from the corner lanes, whose estimate may be one texel high (its slack)"""
    for phase in PHASES:
        b = bases(n, f, phase)
        for est in (0, 1):
            ox = min(b[0], b[-1]) + est - (bound - 1) - 1
            rel = b - ox
            # (the kernel clamps to this range so that padding lanes stay inside: it must not bite)
            if rel.min() < bound - 1 or rel.max() > ring_w - bound - 1:
                return False
            if rel.min() + 1 - bound < 0 or rel.max() + bound > ring_w - 1:
                return False
        # and one spare column on the high side
        if (b - b[0]).max() + bound + bound > ring_w - 2:
            return False
    return True


@functools.lru_cache(maxsize=None)
def rows_walk(f, bound, n, ring_rows):
    """the walk itself: ring[slot] = the virtual row it holds"""
    span = ring_rows - 2
    vmax = span + 2 * bound - 1
    for phase in PHASES:
        b = bases(n, f, phase)
        for est in (0, 1):
            rely = b - (min(b[0], b[-1]) + est - 1)
            if rely.min() < 0 or rely.max() > span - 1:
                return False
            ring = np.full(ring_rows, -1)
            for v in range(min(span + 1, vmax)):
                ring[v % ring_rows] = v
            seen = set()
            for turn in range(2 * bound):
                before = ring.copy()
                if turn + 1 < 2 * bound and turn + span + 1 < vmax:
                    ring[(turn + span + 1) % ring_rows] = turn + span + 1
                y0 = 1 - bound + turn
                for y in range(y0, min(y0 + 1, bound) + 1):
                    seen.add(y)
                    v = rely + (y + bound - 1)
                    slot = turn % ring_rows + (y - y0) + rely
                    slot = np.where(slot >= ring_rows, slot - ring_rows, slot)
                    if slot.min() < 0 or slot.max() >= ring_rows:
                        return False
                    # the row the lane means, before and after this turn's staging
                    if not (np.array_equal(before[slot], v) and np.array_equal(ring[slot], v)):
                        return False
            if seen != set(range(1 - bound, bound + 1)):
                return False
        # and one spare row on the high side
        if (b - b[0]).max() + 1 > span - 2:
            return False
    return True


def sweep(radius, top):
    n = int(round((top - 1.0) / 0.07)) + 1
    return [round(1.0 + 0.07 * i, 2) for i in range(n)]


@pytest.mark.parametrize("radius,top", [(3.2383154841662362, 9.88), (2.0, 16.0)])
@pytest.mark.parametrize("texel", [8, 16])
def test_plan_over_every_ratio(radius, top, texel):
    fs = sweep(radius, top)
    assert fs[0] == 1.0 and abs(fs[-1] - top) < 0.07
    checked = 0
    for fx in fs:
        for fy in fs:
            bound = math.ceil(radius * max(fx, fy))
            p = plan(fx, fy, bound, texel)
            assert (p is not None) == (bound <= 32), (fx, fy, bound, p)
            if p is None:
                continue
            ow, oh, rows, width, lds = p
            assert lds == 2048 + rows * width * texel and lds <= 163840, p
            assert (ow, oh) in SHAPES, p
            assert columns_fit(fx, bound, ow, width), (fx, fy, bound, p)
            assert rows_walk(fy, bound, oh, rows), (fx, fy, bound, p)
            checked += 1
    assert checked > 10000


def test_plan_stops_at_the_reference_cap():
    # 2 * bound - 1 gathers of a tap row in a 64-bit mask (sampling.c:671-674)
    assert plan(9.88, 9.88, 32, 16) is not None
    assert plan(10.0, 10.0, 33, 16) is None
    assert plan(2.0, 2.0, 0, 16) is None


def test_plan_narrows_the_tile():
    """a ring row holds the tile's whole width, so steep ratios narrow the tile: each shape is taken
    exactly when the wider ones do not fit"""
    taken = set()
    for f, bound in ((4.5, 15), (6.0, 20), (9.88, 32), (16.0, 32)):
        for texel in (8, 16):
            p = plan(f, f, bound, texel)
            sizes = [2048 + (math.ceil(w * f - 1e-5) + 2 * bound + 2) * (math.ceil(h * f - 1e-5) + 5) * texel
                     for w, h in SHAPES]
            first = next(i for i, sz in enumerate(sizes) if sz <= LDS_LIMIT)
            assert p[:2] == SHAPES[first] and p[4] == sizes[first], (f, bound, texel, p, sizes)
            taken.add(p[:2])
    assert (32, 8) in taken and (16, 1) in taken, taken
    # what the two real workloads of an ABR ladder get: 2160p -> 480p from rgba16, -> 360p from rgba16hf
    assert plan(4.5, 4.5, 15, 16)[:2] == (32, 8)
    assert plan(6.0, 6.0, 20, 8)[:2] == (32, 8)
