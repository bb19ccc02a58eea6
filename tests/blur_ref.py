"""A numpy restatement of the blurred border (pl_render_params.border = PL_CLEAR_BLUR): the plan of
the reference's pass_blur (src/renderer.c:2345-2465), its taps in the kernel's order (k_blur.hip),
the rounding of every level to the intermediate format, and the border's direct sample
(clear_target :2504-2547). float32 throughout, fma through float64 (the product is exact there)."""
import math

import numpy as np

import orc

f32 = np.float32
MAX_BLUR_PASSES = 10


def plan(radius, w, h):
    """(passes, offset, [(w, h) of every level], up) as rp_plan_blur computes them"""
    radius = f32(radius)
    if radius <= 0 or (w == 1 and h == 1):
        return 0, f32(0), [(w, h)], False
    a_min, a_max = f32(1.0), f32(1.8)
    q = float(radius * radius / (a_max * a_max))
    passes = math.ceil(f32(math.log(f32(1.0 + q))) / f32(math.log(4.0)))     # (a float quotient)
    passes = min(max(passes, 2), MAX_BLUR_PASSES)

    def off(n):
        return radius / np.sqrt(f32(4.0) ** f32(n) - f32(1.0), dtype=f32)
    offset = off(passes)
    if offset < a_min and passes > 2:
        passes -= 1
        offset = off(passes)
    if offset > a_max and passes < MAX_BLUR_PASSES:
        passes += 1
        offset = off(passes)
    levels = []
    for i in range(passes + 1):
        levels.append((w, h))
        if w == 1 and h == 1:
            passes = i
            break
        w, h = max(w // 2, 1), max(h // 2, 1)
    return passes, f32(offset), levels, levels[passes] != (1, 1)


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def mix(x, y, a):
    return fma(y, a, fma(-x, a, x))


def _mirror(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def tex_linear(img, px, py):
    """samplers.hiph tex_linear with MIRROR addressing; img (h, w, 4) float32"""
    h, w = img.shape[:2]
    u = (px * f32(w)).astype(f32) - f32(0.5)
    v = (py * f32(h)).astype(f32) - f32(0.5)
    fu, fv = np.floor(u), np.floor(v)
    ax, ay = (u - fu)[..., None], (v - fv)[..., None]
    x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
    xa, xb = _mirror(x0, w), _mirror(x0 + 1, w)
    ya, yb = _mirror(y0, h), _mirror(y0 + 1, h)
    return mix(mix(img[ya, xa], img[ya, xb], ax), mix(img[yb, xa], img[yb, xb], ax), ay)


def _positions(src_w, src_h, w, h):
    """pos of every output of a w x h pass over the whole of a src_w x src_h level"""
    os_x, os_y = f32(1.0 / w), f32(1.0 / h)
    mx = (os_x * (np.arange(w, dtype=f32) + f32(0.5))).astype(f32)[None, :]
    my = (os_y * (np.arange(h, dtype=f32) + f32(0.5))).astype(f32)[:, None]
    mx, my = np.broadcast_to(mx, (h, w)), np.broadcast_to(my, (h, w))
    x1 = f32(f32(1.0 / src_w) * f32(src_w))
    y1 = f32(f32(1.0 / src_h) * f32(src_h))
    zero = np.zeros((h, w), f32)
    px = mix(mix(zero, x1, mx), mix(zero, x1, mx), my)
    py = mix(mix(zero, zero, mx), mix(y1 + zero, y1 + zero, mx), my)
    return px, py


def blur_pass(src, w, h, offset, up):
    """one pass into a w x h level (float32, not yet rounded)"""
    sh_, sw = src.shape[:2]
    px, py = _positions(sw, sh_, w, h)
    sx, sy = f32(offset) / f32(sw), f32(offset) / f32(sh_)

    def t(x, y):
        return tex_linear(src, x, y)
    if not up:
        c = t(px, py) * f32(4.0)
        c = c + t(px - sx, py - sy)
        c = c + t(px + sx, py + sy)
        c = c + t(px - sx, py - (-sy))
        c = c + t(px + sx, py + (-sy))
        return (c / f32(8.0)).astype(f32)
    s2x, s2y = sx + sx, sy + sy
    c = t(px - s2x, py - f32(0))
    c = c + t(px + s2x, py + f32(0))
    c = c + t(px - f32(0), py - s2y)
    c = c + t(px + f32(0), py + s2y)
    c = c + t(px + -sx, py + -sy) * f32(2.0)
    c = c + t(px + sx, py + -sy) * f32(2.0)
    c = c + t(px + -sx, py + sy) * f32(2.0)
    c = c + t(px + sx, py + sy) * f32(2.0)
    return (c / f32(12.0)).astype(f32)


def to_f16(img):
    return img.astype(np.float16).astype(f32)


def pyramid(img, radius):
    """the border texture of an image (h, w, 4) float32 as the renderer holds it (rgba16hf levels)"""
    h, w = img.shape[:2]
    passes, offset, levels, up = plan(radius, w, h)
    if not passes:
        return img
    lv = [img]
    for i in range(passes):
        lv.append(to_f16(blur_pass(lv[-1], *levels[i + 1], offset, False)))
    if not up:
        return lv[passes]
    prev = lv[passes]
    for i in range(passes - 1, -1, -1):
        prev = to_f16(blur_pass(prev, *levels[i], offset, True))
    return prev


def border_sample(border, rect, out_w, out_h):
    """pl_shader_sample_direct of the border texture over `rect` onto an out_w x out_h plane
    (bilinear, clamped), the oracle's restatement of the renderer's direct sample"""
    return orc.sample_simple(border, orc.S_BILINEAR, out_w, out_h, rect=rect)

