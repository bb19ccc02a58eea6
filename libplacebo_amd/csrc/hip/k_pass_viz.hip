/*
 * libplacebo-hip — the generic pass kernel's variant for the colour map's diagnostics
 * (pl_color_map_params.show_clipping / .visualize_lut; cmviz.hiph): the Dolby Vision / corner
 * rounding variant plus one register per pixel for the clip flags, with and without the
 * tricubic LUT lookup. A diagnostic path: every sampler the generic kernel has, one row of two
 * pixels per lane, no tuning. plh_launch_pass (k_pass.hip) sends every pass that carries one of
 * the ops here, and nothing else.
 */
#include "k_pass_generic.hiph"

int plh_launch_generic_viz(hipStream_t stream, const plh_pass *pass, bool cubic)
{
    const dim3 block(PASS_BW, PASS_BH);
    const int cells_w = (pass->width + pass->cell_padx + 1) / 2;
    const int bh = PASS_BH * PASS_ITERS;
    const dim3 grid((cells_w + PASS_BW - 1) / PASS_BW, (pass->height + bh - 1) / bh);
    if (cubic)
        PLH_LAUNCH_LAST((k_pass_generic<false, false, 1, false, true, true, true>), grid, block, 0, stream, *pass);
    else
        PLH_LAUNCH_LAST((k_pass_generic<false, false, 1, false, false, true, true>), grid, block, 0, stream, *pass);
    return plh_launch_status();
}
