"""The shape-specialised instances of k_polar_mx's chain epilogue (PL_HIP_CHAIN_SHAPE, colorops.hiph:
run_map_chain_fixed, k_polar_mxs.hip) against the generic CHAIN instance.

A specialised instance runs the same device functions in the same order on the same values, with
every decision the generic instance takes per turn -- which stages there are, which curve, where the
tables lie -- taken by the compiler: its frames must be BIT-IDENTICAL to those of
PL_HIP_CHAIN_SHAPE=0 (the generic instance always). Every case also reads the launcher's own trace
line (PL_HIP_PASS_TRACE) and checks WHICH instance took the launch, so that none of these
comparisons can pass by rendering the generic instance twice.

* the metric's frame (bench.py's ewa_1080p_to_4k_hdr_tonemap parameters: HDR10 -> EWA-Lanczos 2x ->
  tone + gamut map -> BT.1886 -> blue-noise dither to 10 bit), small, at an odd size whose last
  tiles are partial, and 1080p -> 4K;
* the same frame for every target curve that has an instance of its own (BT.1886; the pure power
  laws, which share one; sRGB), and for curves that have none (linear, ST 428), which
  must stay on the generic instance;
* an rgba16hf source whose left half carries PQ "codes" up to 1.6, beyond the tables of cubics: the
  specialised instance's wave-wide fall-back to the closed forms, with the PQ constants it has
  copied out of the kernel arguments itself;
* the 720p -> 4K HDR frame (k_polar_mxr, which keeps the generic chain: nothing may move);
* the metric's frame without the dither op into a 16-bit target. Without a dither the pass does not
  have the specialised instance's shape, so this pins that the switch moves nothing else; the frame
  is held to the oracle and to float64 by util.assert_colormap_parity as test_gpu_metric.py does."""
import ctypes as C
import os

import numpy as np
import pytest

import libplacebo_amd as pl
import orc
import util
from libplacebo_amd import _capi as capi
from test_gpu_fullsize import P1080, colormap_tolerance, hdr_frame16
from test_gpu_metric import HDR, metric_params, resolve, ten_bit

pytestmark = pytest.mark.gpu

P720 = (1280, 720)
# plh_chain_shape's numbers (fastepi.hiph); 0 = no instance for that curve
SHAPE_OF = dict(bt1886=1, gamma22=2, gamma28=2, srgb=3, linear=0, st428=0)


def render(gpu, img, dw, dh, params, repr_, env, fmt="rgba16", transfer="bt1886"):
    env = {"PL_HIP_POLAR_MFMA": "1", **env}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h, w = img.shape[:2]
        rr = pl.Renderer(gpu)
        src = gpu.tex_create(w, h, fmt, img)
        dst = gpu.tex_create(dw, dh, "rgba16")
        util.srand(1)
        assert rr.render(pl.frame(src, components=3, color=pl.color_space(**HDR)),
                         pl.frame(dst, color=pl.color_space("bt709", transfer), repr_=repr_),
                         params), gpu.messages[-4:]
        assert rr.errors() == 0
        out = dst.download()
        meta = capi.HdrMetadata()
        assert pl.lib().pl_renderer_get_hdr_metadata(rr.rr, C.byref(meta))
        rr.destroy(); src.destroy(); dst.destroy()
        return out, meta
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def both(gpu, capfd, img, dw, dh, params, repr_, shape, mx=True, **kw):
    """The frame with PL_HIP_CHAIN_SHAPE=0 and =1. `shape`: the instance =1 must run (plh_chain_shape's
    number; 0: the generic one); =0 must always run the generic one. mx: the launch is k_polar_mx's."""
    out = {}
    for v in ("0", "1"):
        capfd.readouterr()
        out[v], meta = render(gpu, img, dw, dh, params, repr_,
                              {"PL_HIP_CHAIN_SHAPE": v, "PL_HIP_PASS_TRACE": "1"}, **kw)
        lines = [l for l in capfd.readouterr().err.splitlines() if "k_polar_mx chain" in l]
        if not mx:
            assert not lines, lines
            continue
        assert lines, "the chain epilogue of k_polar_mx did not run"
        if v == "1" and shape:
            want = "shape %d, specialised instance" % shape
        else:
            want = "shape %d, generic instance" % (shape if v == "1" else 0)
        assert all(l.endswith(want) for l in lines), (v, want, lines)
    d = np.abs(out["1"].astype(np.int64) - out["0"].astype(np.int64))
    with capfd.disabled():
        print("%dx%d %s: PL_HIP_CHAIN_SHAPE=1 (shape %d) vs =0: %d of %d samples differ, max %d codes"
              % (dw, dh, kw.get("transfer", "bt1886"), shape, int((d > 0).sum()), d.size, int(d.max())))
    assert out["0"][..., :3].std() > 1000
    assert np.array_equal(out["1"], out["0"]), util.diff_stats(out["1"], out["0"])
    return out, meta


@pytest.mark.parametrize("size", [(160, 90), (97, 61), P1080])
def test_metric_frame_bit_identical(gpu, capfd, size):
    sw, sh = size
    both(gpu, capfd, hdr_frame16(sw, sh), 2 * sw, 2 * sh, metric_params(True), ten_bit(), 1)


@pytest.mark.parametrize("size", [(160, 90), (97, 61)])
@pytest.mark.parametrize("transfer", sorted(SHAPE_OF))
def test_every_target_curve(gpu, capfd, transfer, size):
    sw, sh = size
    both(gpu, capfd, hdr_frame16(sw, sh), 2 * sw, 2 * sh, metric_params(True), ten_bit(),
         SHAPE_OF[transfer], transfer=transfer)


@pytest.mark.parametrize("transfer", ["bt1886", "gamma22", "srgb"])
def test_values_beyond_the_cubics(gpu, capfd, transfer):
    """(the frame of test_gpu_kernel_variants.py::test_pq_segments_against_closed_forms, here behind the
    dither that gives the pass the specialised instance's shape)"""
    sw, sh = 97, 61
    f16 = hdr_frame16(sw, sh).astype(np.float32) / 65535.0
    f16[:, : sw // 2, :3] *= 1.6 / max(float(f16[..., :3].max()), 1e-3)
    f16 = f16.astype(np.float16)
    assert float(f16[..., :3].max()) > 1.5
    both(gpu, capfd, f16, 2 * sw, 2 * sh, metric_params(True), ten_bit(), SHAPE_OF[transfer],
         fmt="rgba16hf", transfer=transfer)


@pytest.mark.parametrize("size", [(96, 54), P720])
def test_720p_to_4k_hdr_frame_bit_identical(gpu, capfd, size):
    sw, sh = size
    both(gpu, capfd, hdr_frame16(sw, sh), 3 * sw, 3 * sh, metric_params(True), ten_bit(), 0, mx=False)


def test_undithered_16_bit_target(gpu, capfd):
    import colormap_f64 as c64
    import colormap_ref as cr
    sw, sh = 160, 90
    dw, dh = 2 * sw, 2 * sh
    img = hdr_frame16(sw, sh)
    out, meta = both(gpu, capfd, img, dw, dh, metric_params(False), None, 0)
    # the oracle and the float64 truth, as test_gpu_metric.py composes them
    tex = orc.tex_decode(img, "rgba16")
    tex[..., 3] = 1.0
    w, r, rz = orc.filter_generate_polar(orc.ewa_lanczos())
    b = orc.sample_polar(orc.op_quant_f16(tex), w, r, rz, dw, dh, mask=0x7)
    res = resolve(meta)
    truth = c64.hdr10_to_sdr(b.reshape(-1, 1, 4), res, 0.0)[0].reshape(-1, 4)
    ref16 = orc.tex_encode(cr.apply(b.copy(), res), "rgba16")
    t16 = np.clip(truth[:, :3], 0.0, 1.0) * 65535.0
    qs = (0.5, 0.99, 0.9999, 1.0)
    d = np.abs(out["1"][..., :3].reshape(-1, 3).astype(np.float64) - t16)
    with capfd.disabled():
        print("undithered: |frame - float64| quantiles %s = %s codes" % (qs, np.round(np.quantile(d, qs), 2).tolist()))
    colormap_tolerance(out["1"], ref16, truth, np.arange(dw * dh))
