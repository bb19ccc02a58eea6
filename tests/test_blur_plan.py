"""The blurred border's pyramid as the planner lays it out (rp_plan_blur, shown by plh_test_plan):
the pass count, tap offset and level sizes of the reference's pass_blur (src/renderer.c:2345-2465),
restated in blur_ref.plan. CPU only."""
import ctypes as C
import re

import numpy as np
import pytest

import blur_ref
import libplacebo_amd as pl
from libplacebo_amd import _capi as capi
from test_render_plan import FakeTex, plan

RADII = [0, 0.1, 1, 2, 16, 64, 1000]
SIZES = [(1, 1), (1, 7), (3, 2), (1920, 800), (3839, 1601)]


@pytest.fixture(scope="module")
def L(built):
    lib = pl.lib()
    lib.plh_test_format.restype = C.POINTER(capi.Fmt)
    lib.plh_test_format.argtypes = [C.c_char_p]
    lib.plh_test_plan.restype = C.c_size_t
    return lib


def letterbox(L, w, h, **kw):
    """a w x h image 1 : 1 into the middle of a larger target"""
    s, d = FakeTex(L, w, h, "rgba16hf"), FakeTex(L, w + 4, h + 6, "rgba16hf")
    image = pl.frame(s, components=3)
    target = pl.frame(d, crop=(2, 3, 2 + w, 3 + h))
    image._keep, target._keep = s, d
    return image, target


def blur_line(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("blur:")]
    assert len(lines) <= 1, text
    return lines[0] if lines else None


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("radius", RADII)
def test_plan_follows_the_formula(L, radius, size):
    w, h = size
    image, target = letterbox(L, w, h)
    text = plan(L, image, target, pl.render_params("fast", border=3, blur_radius=radius))
    line = blur_line(text)
    assert line is not None, text
    m = re.match(r"blur: radius (\S+) passes (\d+) offset (\S+) levels((?: \d+x\d+)+)( \(no upscale\))?$",
                 line)
    assert m, line
    passes, offset, levels, up = blur_ref.plan(radius, w, h)
    assert int(m.group(2)) == passes, (line, passes)
    assert np.float32(float(m.group(3))) == offset, (line, offset)
    got = [tuple(int(v) for v in lv.split("x")) for lv in m.group(4).split()]
    assert got == levels, (line, levels)
    assert (m.group(5) is None) == up, line


def test_default_radius_is_four_levels(L):
    image, target = letterbox(L, 3840, 1600)
    line = blur_line(plan(L, image, target, pl.render_params("fast", border=3)))
    assert line.startswith("blur: radius 16 passes 4 "), line
    assert line.endswith("levels 3840x1600 1920x800 960x400 480x200 240x100"), line


def test_no_blur_without_a_border_or_as_background(L):
    image, target = letterbox(L, 64, 48)
    assert blur_line(plan(L, image, target, pl.render_params("fast"))) is None
    assert blur_line(plan(L, image, target, pl.render_params("fast", background=3))) is None
    assert blur_line(plan(L, image, target, pl.render_params("fast", border=3,
                                                              skip_target_clearing=True))) is None
    # no intermediates: nothing is planned (the render fails instead)
    assert blur_line(plan(L, image, target, pl.render_params("fast", border=3), fbos=False)) is None
    # an uncropped target has no border
    s, d = FakeTex(L, 64, 48, "rgba16hf"), FakeTex(L, 64, 48, "rgba16hf")
    text = plan(L, pl.frame(s, components=3), pl.frame(d), pl.render_params("fast", border=3))
    assert "output plane 0" in text and blur_line(text) is None, text
