"""When may k_ortho_fast / k_lowpass2 address a MIRRORED pass with their single reflection (of_tap,
csrc/hip/k_ortho.hip)? plh_ortho_one_reflection (host: shader_sampling.c, through the
plh_test_ortho_one_reflection hook) against a float32 restatement of the kernel's per-pixel
arithmetic -- no GPU.

The rule it replaces,

    n_axis >= 2 * row_size and all(-0.9 < p < 1.9 for p in pos)          (old_rule below)

bounded the rect but forgot how far the taps reach beyond it: first = floor(pos * n - 0.5) -
(N / 2 - 1), last = first + N - 1, and first + N where two pixels share a window. On a small texture
a rect that ends near -0.9 or 1.9 texture sizes put taps past one reflection -- an index outside
[0, n), which the kernel then loaded from. test_old_rule_admits_out_of_range_taps holds that finding
still: the sweep below FAILS for the old rule."""
import ctypes as C

import numpy as np
import pytest

import libplacebo_amd as pl

ROW_SIZES = (2, 4, 6, 8, 10, 12, 16)
# rect ends in texture sizes: inside, on the edges, either side of the old rule's window, periods out
ENDS = (-1.5, -0.9, -0.85, -0.25, 0.0, 1.0, 1.85, 1.9, 2.5)
# (rect ends across the filtered axis, n_across): the renderer's, the old window's, far out and flipped
ACROSS = (((0.0, 1.0), 5), ((-0.85, 1.85), 3), ((2.5, -1.5), None))
F = np.float32


def hook():
    return pl.lib().plh_test_ortho_one_reflection


def corners(n_axis, n_across, along, across, d):
    """sh_bind (shaders.c): pos = (1 / size) * rect, float32; corner order (x0 y0) (x1 y0) (x0 y1) (x1 y1)"""
    a = [F(F(1.0 / n_axis) * F(e * n_axis)) for e in along]
    o = [F(F(1.0 / n_across) * F(e * n_across)) for e in across]
    x, y = (o, a) if d else (a, o)
    return np.array([[x[0], y[0]], [x[1], y[0]], [x[0], y[1]], [x[1], y[1]]], F)


def old_rule(n_axis, row_size, pos):
    return n_axis >= 2 * row_size and bool(np.all((pos > F(-0.9)) & (pos < F(1.9))))


def fma(a, b, c):
    # (a float32 product is exact in float64)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def mix(x, y, a):
    """plh_mix (devmath.hiph): fma(y, a, fma(-x, a, x))"""
    return fma(y, a, fma(-x, a, x))


COLS, ROWS = 32, 3


def pixels(n, k):
    """(G,) sizes -> (G, k) pixel indices: every pixel of a short axis (the last one repeated); of a
    long one both ends and a spread in between (the position is affine in the index: its extremes,
    bar rounding, are at the ends)"""
    j = np.arange(k)[None, :]
    n = n[:, None]
    e = 3 * k // 8
    spread = np.where(j < e, j, np.where(j >= k - e, n - k + j, e + (j - e) * (n - 2 * e) // (k - 2 * e)))
    return np.where(n <= k, np.minimum(j, n - 1), spread)


def out_of_reach(pos, n_axis, n_across, N, d, width, height):
    """k_ortho_fast's statements for the pixels of G passes at once (pos: (G, 4, 2); the other
    arguments (G,), `width` along the filtered axis): is some index handed to of_tap -- along the
    filtered axis, the shared window's extra tap included, or across it -- NOT brought into [0, n) by
    one reflection, i < 0 ? -1 - i : (i >= n ? 2 n - 1 - i : i)?"""
    ia, io = pixels(width, COLS), pixels(height, ROWS)
    ma = (F(1.0) / width.astype(F))[:, None] * (ia.astype(F) + F(0.5))      # out_scale * (id + 0.5)
    mo = (F(1.0) / height.astype(F))[:, None] * (io.astype(F) + F(0.5))
    shape = (len(width), ROWS, COLS)
    ma, mo = np.broadcast_to(ma[:, None, :], shape), np.broadcast_to(mo[:, :, None], shape)
    mx, my = (np.where(d[:, None, None] == 1, u, v) for u, v in ((mo, ma), (ma, mo)))
    p = [[np.broadcast_to(pos[:, k, c][:, None, None], shape) for c in (0, 1)] for k in range(4)]
    attr = [mix(mix(p[0][c], p[1][c], mx), mix(p[2][c], p[3][c], mx), my) for c in (0, 1)]
    dd = d[:, None, None] == 1
    pa, po = np.where(dd, attr[1], attr[0]), np.where(dd, attr[0], attr[1])
    na, no, half = n_axis[:, None, None], n_across[:, None, None], (N // 2)[:, None, None]
    ta = (pa * na.astype(F)).astype(F) - F(0.5)
    first = np.floor(ta).astype(np.int64) - (half - 1)
    o0 = np.floor((po * no.astype(F)).astype(F)).astype(np.int64)
    bad = (first < -na) | (first + 2 * half > 2 * na - 1) | (o0 < -no) | (o0 > 2 * no - 1)
    return bad.any(axis=(1, 2))


_SWEEP = None


def sweep():
    """every geometry of the sweep -> (its parameters, the hook's answer, the old rule's answer, "a tap
    is out of one reflection's reach at one of three output sizes")"""
    global _SWEEP
    if _SWEEP is not None:
        return _SWEEP
    fn = hook()
    geo, pos_all = [], []
    for N in ROW_SIZES:
        for n_axis in range(1, 6 * N + 1):
            for d in (0, 1):
                for across, n_across in ACROSS:
                    n_across = n_across or 2 * N + 1
                    for e0 in ENDS:
                        for e1 in ENDS:
                            if e0 != e1:
                                geo.append((N, n_axis, n_across, d, int(round(abs(e1 - e0) * n_axis)) or 1))
                                pos_all.append(corners(n_axis, n_across, (e0, e1), across, d))
    geo, pos_all = np.array(geo, np.int64), np.ascontiguousarray(pos_all, F)
    fp = C.POINTER(C.c_float)
    new = np.array([bool(fn(int(g[1]), int(g[2]), int(g[0]), pos_all[i].ctypes.data_as(fp), int(g[3])))
                    for i, g in enumerate(geo)])
    old = np.array([old_rule(g[1], g[0], pos_all[i]) for i, g in enumerate(geo)])
    sel = np.flatnonzero(new | old)
    N, n_axis, n_across, d, length = geo[sel].T
    bad = np.zeros(len(geo), bool)
    # a 2x upscale, a 3 : 1 downscale, an odd size that is neither; 5 pixels across
    for out in (2 * length, np.maximum(1, length // 3), np.full_like(length, 7)):
        bad[sel] |= out_of_reach(pos_all[sel], n_axis, n_across, N, d, out, np.full_like(length, 5))
    _SWEEP = geo, new, old, bad
    return _SWEEP


def test_one_reflection_serves_every_tap_where_the_guard_says_yes():
    geo, new, old, bad = sweep()
    assert new.sum() > 1000         # (the fast kernel keeps a good part of the sweep)
    assert not (new & bad).any(), geo[new & bad][:5]


def test_old_rule_admits_out_of_range_taps():
    """The same sweep with the rule the launcher had: it accepts geometries whose taps one reflection
    does not bring back into the texture -- among them N = 6 on textures of 12 .. 29 texels, N = 16
    on 32 .. 38."""
    geo, new, old, bad = sweep()
    hit = geo[old & bad]
    assert len(hit)
    assert ((hit[:, 0] == 6) & (hit[:, 1] >= 12) & (hit[:, 1] <= 29)).any()
    assert ((hit[:, 0] == 16) & (hit[:, 1] >= 32) & (hit[:, 1] <= 38)).any()


@pytest.mark.parametrize("N", ROW_SIZES)
def test_the_renderers_mirrored_passes_stay_on_the_fast_kernel(N):
    """pos within [0, 1] (the contrast-recovery low-pass: whole planes, either direction, flipped or
    not) on any texture that holds two windows, and is two texels or more across: yes, as before."""
    fn = hook()
    for n_axis in (2 * N, 2 * N + 1, 3 * N, 64, 617, 2160, 3840):
        for n_across in (2, 3, 33, 3840):
            for d in (0, 1):
                for along in ((0.0, 1.0), (1.0, 0.0), (0.25, 0.75)):
                    for across in ((0.0, 1.0), (1.0, 0.0)):
                        pos = corners(n_axis, n_across, along, across, d)
                        assert fn(n_axis, n_across, N, pos.ctypes.data_as(C.POINTER(C.c_float)), d), \
                            (N, n_axis, n_across, d, along, across)
    # and never below two windows
    pos = corners(2 * N - 1, 8, (0.0, 1.0), (0.0, 1.0), 0)
    assert not fn(2 * N - 1, 8, N, pos.ctypes.data_as(C.POINTER(C.c_float)), 0)
