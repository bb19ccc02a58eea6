/*
 * libplacebo-hip — the PL_HIP_* environment switches: which of two kernels (or code paths) that
 * render the same frame is taken, so that tests and profiles can pin one. INTEGRATION.md lists
 * them in this order (tests/test_switch_table.py). One rule for all: unset or empty = the default,
 * otherwise a decimal integer; a value that does not parse completely is ignored. The environment
 * is read on EVERY call: tests flip a switch between two renders of one process.
 */
#ifndef PLH_SWITCH_H_
#define PLH_SWITCH_H_

#ifdef __cplusplus
extern "C" {
#endif

//  X(id, environment name, default, what the values choose between)
#define PLH_SWITCHES(X) \
    X(ASYNC_MEASURE,   "PL_HIP_ASYNC_MEASURE",   -1, "0 | 1 override pl_hip_params.async_measure (the measuring pass on a second stream); unset: the parameter") \
    X(NO_FUSION,       "PL_HIP_NO_FUSION",       -1, "1: the renderer records the reference's separate passes; 0: fuses wherever it is valid; unset: where it also pays") \
    X(FUSED_FEATURES,  "PL_HIP_FUSED_FEATURES",   1, "0: the contrast-recovery feature map as its own pass instead of a side output of the plane pass") \
    X(NT_STORE,        "PL_HIP_NT_STORE",         1, "0: plain stores to unorm targets instead of streaming (non-temporal) ones") \
    X(POLAR_MFMA,      "PL_HIP_POLAR_MFMA",       1, "0: every polar pass on the bit-exact sequential-fma kernels instead of the matrix-pipe ones") \
    X(POLAR_PER_PIXEL, "PL_HIP_POLAR_PER_PIXEL",  0, "1: polar weights evaluated per pixel (k_polar) instead of from phase-class tables (k_polar_pp)") \
    X(POLAR_BAND,      "PL_HIP_POLAR_BAND",       0, "1: every polar pass on k_polar_band (the footprint walked through a ring of source rows) instead of only those whose footprint no other kernel can stage") \
    X(MX_PERSIST,     "PL_HIP_MX_PERSIST",       1, "0: k_polar_mx (a workgroup per tile) instead of k_polar_mxp (persistent workgroups)") \
    X(MAP_CHAIN,       "PL_HIP_MAP_CHAIN",        1, "0: colour-management ops walked by the interpreter instead of the straight-line chain") \
    X(PQ_SEGMENTS,     "PL_HIP_PQ_SEGMENTS",      1, "0: the chain's PQ pair in closed form instead of piecewise cubics in LDS") \
    X(PQ_SEG_COPIES,   "PL_HIP_PQ_SEG_COPIES",    1, "1 | 2 | 4 | 8 | 16 copies of every piece of those cubics in k_polar_mx's LDS") \
    X(CHAIN_SHAPE,     "PL_HIP_CHAIN_SHAPE",      1, "0: k_polar_mx's generic chain instance always, instead of its shape-specialised one for HDR10 -> SDR passes (bit-identical)") \
    X(PASS_NATIVE,     "PL_HIP_PASS_NATIVE",      1, "0: 1:1 passes on k_pass_generic instead of k_pass_native / k_pass_chain / k_pass_merge / k_pass_mix") \
    X(BILIN_ITERS,     "PL_HIP_BILIN_ITERS",      1, "1 | 2 | 4 cells per lane of k_bilinear_fast; 0: k_pass_generic instead of it and of k_nearest_fast") \
    X(ORTHO_FAST,      "PL_HIP_ORTHO_FAST",       1, "0: separable passes on k_ortho instead of k_ortho_fast") \
    X(LOWPASS_FUSED,   "PL_HIP_LOWPASS_FUSED",    1, "0: the feature map's low-pass as two ortho passes instead of the one k_lowpass2 launch") \
    X(DEBAND_FAST,     "PL_HIP_DEBAND_FAST",      1, "0: debanding on k_deband instead of k_deband_fast / k_deband_lds") \
    X(DEBAND_LDS,      "PL_HIP_DEBAND_LDS",       1, "0: k_deband_fast (fetches from memory) instead of k_deband_lds (window staged in LDS)") \
    X(PEAK_FAST,       "PL_HIP_PEAK_FAST",        1, "0: peak detection on k_pass_peak (the op interpreter) instead of k_peak_tiles / k_peak_fast") \
    X(PEAK_TILES,      "PL_HIP_PEAK_TILES",       1, "0: k_peak_fast + k_peak_fold (two launches) instead of k_peak_tiles (folded on chip)") \
    X(PASS_TRACE,      "PL_HIP_PASS_TRACE",       0, "1: one line per pass launch on stderr: sampler, formats, op list (tools/time_ops.py)") \
    X(PP_ROWS,         "PL_HIP_PP_ROWS",          0, "profiling aid: output rows per lane of k_polar_pp; 0: chosen from the geometry") \
    X(PP_DEBUG,        "PL_HIP_PP_DEBUG",         0, "profiling aid, bit mask: 1 no taps, 2 no verification, 4 no stores, 8 no tile loads")

enum plh_switch_id {
#define PLH_SWITCH_ID(id, name, def, doc) PLH_SW_##id,
    PLH_SWITCHES(PLH_SWITCH_ID)
#undef PLH_SWITCH_ID
    PLH_SW_COUNT
};

// the switch's value now, or its default (plh_switch.c)
int plh_switch(enum plh_switch_id id);

// PL_HIP_PASS_TRACE: "[plh] kernel <name>" on stderr behind the pass's own line -- which kernel the
// launcher chose for it (tests assert it, so that a comparison of two kernels cannot pass by running
// one of them twice)
void plh_trace_kernel(const char *name);

#ifdef __cplusplus
}
#endif

#endif // PLH_SWITCH_H_
