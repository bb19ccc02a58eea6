/*
 * libplacebo-hip -- what a colour-mapping request resolves to, as ONE value.
 *
 * pl_shader_color_map_ex (reference: src/shaders/colorspace.c:1612-1790) decides, before it
 * emits anything, which tone curve and which gamut mapper run between which luminance ranges and
 * whether either can be skipped or folded away. Here that decision is a pure function from the
 * request to a `struct plh_colormap_plan`; shader_color.c only records what the plan says.
 * tests/test_colormap_plan.py holds it to the same decision taken with the reference's own
 * build (oracle/_ref) and to tests/colormap_ref.py::resolve, for every tone / gamut function.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <libplacebo/shaders/colorspace.h>

#include "shaders_priv.h"

struct luma_span { float lo, hi, avg; };

// nominal luminance range of a colour space in `unit`, as seen through `source` metadata
static struct luma_span luma_span(const struct pl_color_space *csp, enum pl_hdr_metadata_type source,
                                  enum pl_hdr_scaling unit)
{
    struct luma_span s = {0};
    pl_color_space_nominal_luma_ex(pl_nominal_luma_params(
        .color = csp, .metadata = source, .scaling = unit,
        .out_min = &s.lo, .out_max = &s.hi, .out_avg = &s.avg,
    ));
    return s;
}

// `v`, or `to` when the two are closer than a millionth (float difference, compared as double)
static float snapped(float v, float to)
{
    return fabs(v - to) < 1e-6 ? to : v;
}

static struct pl_tone_map_params tone_request(const struct pl_color_map_params *par,
                                              const struct pl_color_space *src,
                                              const struct pl_color_space *dst)
{
    const struct luma_span in = luma_span(src, par->metadata, PL_HDR_PQ);
    const struct luma_span out = luma_span(dst, PL_HDR_METADATA_HDR10, PL_HDR_PQ);
    struct pl_tone_map_params t = {
        .function = par->tone_mapping_function ? par->tone_mapping_function : &pl_tone_map_clip,
        .param = par->tone_mapping_param,
        .constants = par->tone_constants,
        .input_scaling = PL_HDR_PQ, .output_scaling = PL_HDR_PQ,
        .lut_size = par->lut_size ? par->lut_size : pl_color_map_default_params.lut_size,
        .input_min = in.lo, .input_max = in.hi, .input_avg = in.avg,
        .output_min = out.lo, .output_max = out.hi,
        .hdr = src->hdr,
    };
    pl_tone_map_params_infer(&t);
    // end points that coincide up to rounding are made to coincide; and a curve never brightens
    // unless inverse tone mapping was asked for
    t.output_max = snapped(t.output_max, t.input_max);
    t.output_min = snapped(t.output_min, t.input_min);
    if (!par->inverse_tone_mapping && t.output_max > t.input_max)
        t.output_max = t.input_max;
    return t;
}

static struct pl_gamut_map_params gamut_request(const struct pl_color_map_params *par,
                                                const struct pl_color_space *src,
                                                const struct pl_color_space *dst)
{
    const struct luma_span out = luma_span(dst, PL_HDR_METADATA_HDR10, PL_HDR_PQ);
    struct pl_gamut_map_params g = {
        .function = par->gamut_mapping ? par->gamut_mapping : &pl_gamut_map_clip,
        .constants = par->gamut_constants,
        .input_gamut = src->hdr.prim, .output_gamut = dst->hdr.prim,
        .min_luma = out.lo, .max_luma = out.hi,
        .lut_stride = 3,
    };
    int *const dims[3] = { &g.lut_size_I, &g.lut_size_C, &g.lut_size_h };
    for (int k = 0; k < 3; k++)
        *dims[k] = par->lut3d_size[k] ? par->lut3d_size[k] : pl_color_map_default_params.lut3d_size[k];
    // a mapper that works in both directions would also EXPAND a smaller source gamut; unless
    // that is wanted, the target is first cut down to what the source can hold
    if (g.function->bidirectional && !par->gamut_expansion &&
        pl_primaries_compatible(&g.input_gamut, &g.output_gamut))
        g.output_gamut = pl_primaries_clip(&g.output_gamut, &g.input_gamut);
    return g;
}

void plh_colormap_resolve(struct plh_colormap_plan *plan, const struct pl_color_map_params *params,
                          const struct pl_color_space *src, const struct pl_color_space *dst,
                          bool stateful)
{
    const struct pl_color_map_params *par = params ? params : &pl_color_map_default_params;
    memset(plan, 0, sizeof(*plan));
    plan->src = *src;
    plan->dst = *dst;
    pl_color_space_infer_map(&plan->src, &plan->dst);
    plan->identity = pl_color_space_equal(&plan->src, &plan->dst);
    if (plan->identity)
        return;

    plan->tone = tone_request(par, &plan->src, &plan->dst);
    plan->gamut = gamut_request(par, &plan->src, &plan->dst);

    // Without a state object there is nowhere to keep a LUT: the curve degrades to its linear
    // stand-in and the gamut mapper to the one that is a matrix (`clip` is closed-form anyway).
    plan->closed_form = !stateful || !par->force_tone_mapping_lut;
    if (!stateful) {
        if (plan->tone.function != &pl_tone_map_clip)
            plan->tone.function = &pl_tone_map_linear;
        if (plan->gamut.function != &pl_gamut_map_clip)
            plan->gamut.function = &pl_gamut_map_saturation;
    }

    plan->need_tone = !pl_tone_map_params_noop(&plan->tone);
    plan->need_gamut = !pl_gamut_map_params_noop(&plan->gamut);
    plan->tone_direct = plan->need_tone && plan->closed_form &&
                        (plan->tone.function == &pl_tone_map_clip ||
                         plan->tone.function == &pl_tone_map_linear);
    // `saturation` is linear in LMS: it becomes part of the output matrix
    plan->fold_saturation = plan->need_gamut && plan->closed_form &&
                            plan->gamut.function == &pl_gamut_map_saturation;
    if (plan->fold_saturation)
        plan->need_gamut = false;

    // The diagnostics act on the full path only, each plot where the stage it shows exists
    // (reference :1805, :1977, :2014); on the matrix-only path they do nothing.
    if (plan->need_tone || plan->need_gamut) {
        struct plh_colormap_viz *viz = &plan->viz;
        viz->show_clipping = par->show_clipping;
        viz->plot_tone = par->visualize_lut && plan->need_tone;
        viz->plot_gamut = par->visualize_lut && plan->need_gamut;
        if (par->visualize_lut) {
            viz->rect = par->visualize_rect;
            if (!viz->rect.x0 && !viz->rect.x1)
                viz->rect.x1 = 1.0f;
            if (!viz->rect.y0 && !viz->rect.y1)
                viz->rect.y1 = 1.0f;
            viz->hue = par->visualize_hue;
            viz->theta = par->visualize_theta;
        }
    }
}

int plh_colormap_op_kinds(const struct plh_colormap_plan *plan, int *kinds)
{
    if (plan->identity || (!plan->need_tone && !plan->need_gamut))
        return 0;
    const struct plh_colormap_viz *viz = &plan->viz;
    int n = 0;
    // the RGB test reads the colour RGB2IPT overwrites, the I test the one it leaves
    if (viz->show_clipping)
        kinds[n++] = PLH_OP_CLIP_TEST;
    kinds[n++] = PLH_OP_RGB2IPT;
    if (viz->show_clipping)
        kinds[n++] = PLH_OP_CLIP_TEST;
    if (plan->need_tone)
        kinds[n++] = PLH_OP_TONE_MAP;
    if (plan->need_gamut) {
        if (viz->show_clipping)
            kinds[n++] = PLH_OP_CLIP_TEST;
        kinds[n++] = PLH_OP_GAMUT_LUT;
        if (viz->plot_gamut) {
            kinds[n++] = PLH_OP_VIZ_GAMUT;
            kinds[n++] = PLH_OP_VIZ_GAMUT_SRC;
            kinds[n++] = PLH_OP_VIZ_GAMUT_DST;
        }
    }
    kinds[n++] = PLH_OP_IPT2RGB;
    if (viz->show_clipping)
        kinds[n++] = PLH_OP_CLIP_MARK;
    if (viz->plot_tone)
        kinds[n++] = PLH_OP_VIZ_TONE;
    return n;
}

// for tests/test_colormap_plan.py: the plan up to its diagnostics (the test's mirror of the struct
// ends there)
PL_API void plh_test_colormap_resolve(struct plh_colormap_plan *plan, const struct pl_color_map_params *params,
                                      const struct pl_color_space *src, const struct pl_color_space *dst,
                                      bool stateful);
void plh_test_colormap_resolve(struct plh_colormap_plan *plan, const struct pl_color_map_params *params,
                               const struct pl_color_space *src, const struct pl_color_space *dst,
                               bool stateful)
{
    struct plh_colormap_plan full;
    plh_colormap_resolve(&full, params, src, dst, stateful);
    memcpy(plan, &full, offsetof(struct plh_colormap_plan, viz));
}

// for tests/test_colormap_viz_plan.py: the diagnostics' part of the plan, as { show_clipping,
// plot_tone, plot_gamut } and { rect x0 y0 x1 y1, hue, theta }, and the op kinds of the full path
PL_API int plh_test_colormap_viz(const struct pl_color_map_params *params,
                                 const struct pl_color_space *src, const struct pl_color_space *dst,
                                 bool stateful, int flags[3], float fields[6], int *kinds);
int plh_test_colormap_viz(const struct pl_color_map_params *params,
                          const struct pl_color_space *src, const struct pl_color_space *dst,
                          bool stateful, int flags[3], float fields[6], int *kinds)
{
    struct plh_colormap_plan plan;
    plh_colormap_resolve(&plan, params, src, dst, stateful);
    const struct plh_colormap_viz *viz = &plan.viz;
    flags[0] = viz->show_clipping; flags[1] = viz->plot_tone; flags[2] = viz->plot_gamut;
    fields[0] = viz->rect.x0; fields[1] = viz->rect.y0; fields[2] = viz->rect.x1; fields[3] = viz->rect.y1;
    fields[4] = viz->hue; fields[5] = viz->theta;
    return plh_colormap_op_kinds(&plan, kinds);
}
