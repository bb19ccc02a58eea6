"""Every transfer curve, both directions, and the sigmoid pair of the op interpreter (transfer.hiph:
op_linearize, op_delinearize, op_sigmoidize, op_unsigmoidize) against a float64 restatement of the
reference's shaders (tests/transfer_f64.py), over ALL 65536 sixteen-bit codes -- the statement
test_gpu_color.py::test_pq_pair_error_bound_over_every_code makes for PQ, made for every curve.

Inputs, per curve and black level (the inferred default; min_luma raised to 1 nit; the smallest
min_luma there is with max_luma = 400 nits -- so PLH_TRC_RESCALE, BT.1886's a / b and HLG's lift
each take three values):
* linearize: every code i / 65535 in R, reversed in G, transposed in B; a second small image with
  each knee and its fp32 neighbours either side, 0 and -0, a run of negatives down to -0.25, values
  above 1 up to 1.25 (scRGB: -0.5 .. 7.5). HLG runs grey (its OOTF couples the channels) plus 64 x 64
  random saturated colours;
* delinearize: fp32(truth of every code), the images of the edge set, linear 0 and values below
  black, each linear-side knee with its neighbours;
* sigmoid, both directions, at the default centre / slope and at (0.6, 11): every code, 0 and 1
  with their fp32 neighbours inside and outside [0, 1].
The truth is computed from the fp32 input the GPU received.

Unit: 16-bit codes of the output (delinearize, sigmoidize), or LOCAL codes (linearize, unsigmoidize):
|got - truth| / s, s = the change of the true curve per 16-bit input code there (central difference
at +-1/65535) -- how far the input would have to move to explain the error. Where s == 0 (the clamped
region) the result must be exact.

Held, per curve, direction and black level (transfer_f64.check):
* condition: no sample more than half a code from float64 (beyond it a 16-bit store lands on the
  wrong code). PQ linearize keeps the bound of its own test: 7.5e-6 relative. One exception, which is
  arithmetic and not a choice: where a single fp32 rounding that the reference's formula cannot avoid
  is itself worth more than a tenth of a code -- the result min + (max - min) * v^g of a black-lifted
  power law next to black, whose ulp is that of `min`; the step m * x + c in front of v^(1/g), whose
  rounding the infinite slope at 0 amplifies -- the limit is K such roundings (transfer_f64's `cond`).
  The fp32 oracle is up to 19 codes from float64 on those samples (gamma 2.8, 1 nit black).
* measured: max error(GPU) <= K * max(E_orc, E_ulp), E_orc the oracle's own maximum on the same
  inputs (computed here, at run time), E_ulp half an fp32 ulp of the result -- over all samples, and
  over the well-conditioned ones alone (cond <= 0.05 code), where a handful of samples next to black
  do not set the yardstick.
* K = 5: a float32 emulation of exp2(y * log2 x), exp2(x * log2 10) and log2(x) * ln 2 in numpy
  (0.5 ulp per primitive) is at most 2.19 x max(E_orc, E_ulp) over all cases (ST 428 delinearize;
  2.07 gamma 2.4, 2.03 ProPhoto, 1.85 gamma 1.8, 1.68 V-Log, 1.58 S-Log, 1.48 BT.1886, 1.11 sRGB, 1.0
  HLG: test_transfer_f64.py prints them all); the hardware's primitives round to 1 ulp: twice that,
  rounded up.
* knees: at each knee and its neighbours the result is within the bound of the truth's branch, and
  where the other branch differs by more than twice the bound, not within the bound of that one.
* alpha passes through bit for bit; every output is finite.

Measured on the MI355X, maxima over the three black levels, GPU / oracle / emulation (linearize in
local codes; delinearize in codes):
    sRGB      0.0103 / 0.0092 / 0.0103    0.0092 / 0.0092 / 0.0084
    BT.1886   0.0060 / 0.0054 / 0.0068    0.0078 / 0.0076 / 0.0097
    ProPhoto  0.0058 / 0.0045 / 0.0063    0.0064 / 0.0048 / 0.0090
    HLG       0.0090 / 0.0078 / 0.0077    0.0125 / 0.0115 / 0.0119   (colours: 2.4e-6 / 2.4e-6 absolute)
    V-Log     0.0035 / 0.0023 / 0.0038    0.0073 / 0.0059 / 0.0057
    S-Log1    0.0063 / 0.0041 / 0.0065    0.0073 / 0.0044 / 0.0056
    S-Log2    0.0062 / 0.0042 / 0.0065    0.0074 / 0.0049 / 0.0056
    scRGB     0.0186 (all three: the half ulp)      0.0155
    PQ        0.013  / 0.51   / 0.55      0.0099 / 0.83   / 0.83     (pqmath.hiph's form against the
                                                                      reference's ill-conditioned one)
    gamma 1.8 .. 2.8, ST 428, well-conditioned samples: 0.035 .. 0.049, the oracle's to three digits;
              next to a lifted black up to 8.2 local codes / 19.4 codes, GPU, oracle and emulation alike
    sigmoidize 0.0088 / 0.0072 / 0.0077 (steep 0.040 all three), unsigmoidize 0.0069 / 0.0097 / 0.0069
              (steep 0.060 all three)
The largest GPU / max(E_orc, E_ulp) is 1.9 (gamma 2.2 with the black at 1e-6 nits), against K = 5.
"""
import numpy as np
import pytest

import libplacebo_amd as pl
import transfer_f64 as t64
from test_gpu_color import run_ops
from test_transfer_f64 import (CURVES, SIGMOIDS, oracle, rgba, sigmoid_case, transfer_case)

pytestmark = pytest.mark.gpu


def launch(gpu, img, record):
    """one run_ops call; alpha (a ramp, so that it is not one value) must come back bit for bit"""
    src = rgba(img)
    src[..., 3] = np.linspace(-0.5, 1.5, src.shape[0] * src.shape[1],
                              dtype=np.float32).reshape(src.shape[:2])
    out = run_ops(gpu, src, record)
    assert np.array_equal(out[..., 3].view(np.uint32), src[..., 3].view(np.uint32))
    return out


def sweep(gpu, case, record, name, capsys):
    got = [launch(gpu, img, record) for _, img in case.images()]
    ref = [oracle(case, img) for _, img in case.images()]
    g, o = case.measure(got), case.measure(ref)
    e = case.measure([case.fn(img, be=t64.Emu32) for _, img in case.images()])
    with capsys.disabled():
        print("\n%-30s GPU %9.4g (well %8.4g)  oracle %9.4g (well %8.4g)  emulation %9.4g (well %8.4g)  "
              "E_ulp %9.4g (well %8.4g)  K = %d" % (name, g.E, g.E_well, o.E, o.E_well, e.E, e.E_well,
                                                    o.E_ulp, o.E_ulp_well, t64.K))
    t64.check(case, g, o, what=name)
    for cname, img in t64.colour_images(case):
        cg, co = launch(gpu, img, record), oracle(case, img)
        fig = t64.check_colours(case, cg, co, img, what=name)
        with capsys.disabled():
            print("%-30s colours: max |GPU - float64| %.3g, oracle %.3g, half an ulp %.3g"
                  % (name, *fig))


@pytest.mark.parametrize("black", list(t64.BLACKS))
@pytest.mark.parametrize("direction", ["linearize", "delinearize"])
@pytest.mark.parametrize("trc", CURVES)
def test_transfer_against_float64_over_every_code(gpu, capsys, trc, direction, black):
    case, csp = transfer_case(trc, direction, black)
    sweep(gpu, case, lambda sh: getattr(sh, direction)(csp), "%s %s %s" % (trc, direction, black),
          capsys)


@pytest.mark.parametrize("which", list(SIGMOIDS))
@pytest.mark.parametrize("inverse", [False, True])
def test_sigmoid_against_float64_over_every_code(gpu, capsys, inverse, which):
    case = sigmoid_case(inverse, which)
    c, s = SIGMOIDS[which]
    sweep(gpu, case, lambda sh: sh.sigmoidize(c, s, inverse=inverse),
          "%s %s" % (case.kind, which), capsys)


def test_linear_is_the_identity(gpu):
    img = t64.planes(t64.codes()).astype(np.float32)
    csp = pl.color_space("bt709", "linear")
    for d in ("linearize", "delinearize"):
        out = launch(gpu, img, lambda sh: getattr(sh, d)(csp))
        assert np.array_equal(out[..., :3], img)
