/*
 * libplacebo-hip — sampling stages: host half of src/shaders/sampling.c.
 *
 * Each pl_shader_sample_* fills the sampler part of the recorded pass. The
 * generation-time decisions the reference makes while emitting GLSL are made
 * here with the same arithmetic:
 *   setup_src                 sampling.c:45-181   ratios, scale, component mask
 *   polar filter + widening   sampling.c:608-631
 *   polar tap pruning/order   sampling.c:503-523 (flags), :776-783 (compute
 *                             order), :798-893 (gather order)
 *   LDS tile size             sampling.c:661-699
 *   ortho filter / LUT        sampling.c:914-942, 1004-1063
 *   deband constants          sampling.c:183-275
 */
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <libplacebo/shaders/sampling.h>

#include "polar_priv.h"

const struct pl_deband_params pl_deband_default_params = { PL_DEBAND_DEFAULTS };

enum filter_req { REQ_NEAREST, REQ_LINEAR, REQ_BEST, REQ_FASTEST };

struct src_info {
    float ratio_x, ratio_y;
    float scale;
    uint8_t comp_mask;
    bool linear; // bound with LINEAR filtering
};

// Size of the source rect and of the output, as setup_src measures them (sampling.c:137-146)
struct src_geometry {
    float src_w, src_h;
    int out_w, out_h;
};

static struct src_geometry src_geometry(const struct pl_sample_src *src)
{
    struct src_geometry g;
    g.src_w = pl_rect_w(src->rect);
    g.src_h = pl_rect_h(src->rect);
    g.src_w = PL_DEF(g.src_w, (float) src->tex->params.w);
    g.src_h = PL_DEF(g.src_h, (float) src->tex->params.h);
    g.out_w = PL_DEF(src->new_w, (int) roundf(fabsf(g.src_w)));
    g.out_h = PL_DEF(src->new_h, (int) roundf(fabsf(g.src_h)));
    return g;
}

// Common source setup; mirrors setup_src (sampling.c:45-181)
static bool setup_src(pl_shader sh, const struct pl_sample_src *src, struct src_info *out,
                      bool resizeable, enum filter_req req)
{
    if (!src->tex) {
        SH_FAIL(sh, "pl_sample_src without `tex`: external samplers are not "
                "supported by the HIP backend");
        return false;
    }

    pl_fmt fmt = src->tex->params.format;
    const bool can_linear = fmt->caps & PL_FMT_CAP_LINEAR;
    if (req == REQ_LINEAR && !can_linear) {
        SH_FAIL(sh, "Trying to use a shader that requires linear sampling with a "
                "texture whose format (%s) does not support PL_FMT_CAP_LINEAR", fmt->name);
        return false;
    }
    out->linear = req == REQ_LINEAR || (req == REQ_BEST && can_linear);

    const struct src_geometry geo = src_geometry(src);
    const float src_w = geo.src_w, src_h = geo.src_h;
    const int out_w = geo.out_w, out_h = geo.out_h;
    if (!out_w || !out_h) {
        SH_FAIL(sh, "Degenerate output size %dx%d", out_w, out_h);
        return false;
    }

    out->ratio_x = out_w / fabs(src_w);
    out->ratio_y = out_h / fabs(src_h);
    out->scale = PL_DEF(src->scale, 1.0);

    const uint8_t tex_mask = (1 << fmt->num_components) - 1;
    uint8_t src_mask = src->component_mask;
    if (!src_mask)
        src_mask = (1 << PL_DEF(src->components, 4)) - 1;
    out->comp_mask = tex_mask & src_mask;

    if (sh->pass.s.type != PLH_SAMPLE_NONE || sh->output != PL_SHADER_SIG_NONE) {
        SH_FAIL(sh, "Illegal sequence of shader operations: a sampling stage must "
                "be the first stage of a shader");
        return false;
    }
    if (!sh_require(sh, PL_SHADER_SIG_NONE, resizeable ? 0 : out_w, resizeable ? 0 : out_h))
        return false;

    const pl_rect2df rect = {
        .x0 = src->rect.x0,
        .y0 = src->rect.y0,
        .x1 = src->rect.x0 + src_w,
        .y1 = src->rect.y0 + src_h,
    };
    if (!sh_bind(sh, src->tex, src->address_mode, &rect))
        return false;

    sh->pass.s.scale = out->scale;
    sh->pass.s.comp_mask = out->comp_mask;
    sh->pass.s.linear = out->linear;
    return true;
}

static bool sample_simple(pl_shader sh, const struct pl_sample_src *src, enum filter_req req,
                          const char *desc)
{
    struct src_info info;
    if (!setup_src(sh, src, &info, true, req))
        return false;
    // 1:1 sampling on the texel grid (what img_sh()/PASS A does): a texture unit returns the
    // texel itself there (its fixed-point lerp weights snap to 0), whereas an exact fp32 lerp
    // would blend in ~1e-5 of a neighbour from the rounding noise in `pos`. Such identity
    // fetches are lowered to nearest - by the dispatch, because these shaders are resizable
    // and only the final output size tells whether the fetch is 1:1 (dispatch.c here).
    sh->pass.s.type = info.linear ? PLH_SAMPLE_BILINEAR : PLH_SAMPLE_NEAREST;
    float rw = pl_rect_w(src->rect), rh = pl_rect_h(src->rect);
    sh->pass.s.rect_w = fabsf(PL_DEF(rw, (float) src->tex->params.w));
    sh->pass.s.rect_h = fabsf(PL_DEF(rh, (float) src->tex->params.h));
    sh->pass.s.rect_on_grid = src->rect.x0 == truncf(src->rect.x0) &&
                              src->rect.y0 == truncf(src->rect.y0);
    if (desc)
        sh_describef(sh, "%s", desc);
    sh_listf(sh, "sample_%s(tex=%dx%d %s, scale=%g)\n", info.linear ? "bilinear" : "nearest",
             src->tex->params.w, src->tex->params.h, src->tex->params.format->name, info.scale);
    return true;
}

bool pl_shader_sample_direct(pl_shader sh, const struct pl_sample_src *src)
{
    return sample_simple(sh, src, REQ_BEST, NULL);
}

bool pl_shader_sample_nearest(pl_shader sh, const struct pl_sample_src *src)
{
    return sample_simple(sh, src, REQ_NEAREST, "nearest");
}

bool pl_shader_sample_bilinear(pl_shader sh, const struct pl_sample_src *src)
{
    return sample_simple(sh, src, REQ_LINEAR, "bilinear");
}

static bool sample_fast(pl_shader sh, const struct pl_sample_src *src, int type, const char *name)
{
    struct src_info info;
    if (!setup_src(sh, src, &info, true, REQ_LINEAR))
        return false;
    if (info.ratio_x < 1 || info.ratio_y < 1) {
        pl_msg(sh->log, PL_LOG_TRACE, "Using fast %s sampling when downscaling. This "
               "will most likely result in nasty aliasing!", name);
    }
    sh->pass.s.type = type;
    sh->pass.s.ratio[0] = info.ratio_x;
    sh->pass.s.ratio[1] = info.ratio_y;
    sh_describef(sh, "%s", name);
    sh_listf(sh, "sample_%s(scale=%g)\n", name, info.scale);
    return true;
}

bool pl_shader_sample_bicubic(pl_shader sh, const struct pl_sample_src *src)
{
    return sample_fast(sh, src, PLH_SAMPLE_BICUBIC, "bicubic");
}

bool pl_shader_sample_hermite(pl_shader sh, const struct pl_sample_src *src)
{
    return sample_fast(sh, src, PLH_SAMPLE_HERMITE, "hermite");
}

bool pl_shader_sample_gaussian(pl_shader sh, const struct pl_sample_src *src)
{
    return sample_fast(sh, src, PLH_SAMPLE_GAUSSIAN, "gaussian");
}

bool pl_shader_sample_oversample(pl_shader sh, const struct pl_sample_src *src, float threshold)
{
    if (!sample_fast(sh, src, PLH_SAMPLE_OVERSAMPLE, "oversample"))
        return false;
    sh->pass.s.threshold = PL_CLAMP(threshold, 0.0f, 0.5f);
    return true;
}

/* ------------------------------------------------------------------------ */
/* complex (LUT based) scalers                                               */

#define SCALER_LUT_SIZE     256
#define SCALER_LUT_CUTOFF   1e-3f

struct sh_sampler_obj {
    pl_filter filter;
    pl_buf lut;         // polar: 256 {L[i], L[i+1]} pairs; ortho: rows
    int num_taps;
    bool taps_gather;   // tap order the list was generated for
    pl_shader_obj pass2; // second ortho pass
    struct polar_tables polar;  // tap list and launch-time tables (polar_tables.c)
};

static void sh_sampler_uninit(pl_gpu gpu, void *ptr)
{
    struct sh_sampler_obj *obj = ptr;
    pl_buf_destroy(gpu, &obj->lut);
    pl_buf_destroy(gpu, &obj->polar.taps);
    pl_buf_destroy(gpu, &obj->polar.pp_blob);
    pl_buf_destroy(gpu, &obj->polar.mx_blob);
    pl_shader_obj_destroy(&obj->pass2);
    pl_filter_free(&obj->filter);
    memset(obj, 0, sizeof(*obj));
}

static void describe_filter(pl_shader sh, const struct pl_filter_config *cfg,
                            const char *stage, float rx, float ry)
{
    const char *dir = rx > 1 && ry > 1 ? "up" : rx < 1 && ry < 1 ? "down"
                    : rx == 1 && ry == 1 ? "noop" : "ana";
    if (cfg->name) {
        sh_describef(sh, "%s %sscaling (%s)", stage, dir, cfg->name);
    } else if (cfg->window) {
        sh_describef(sh, "%s %sscaling (%s+%s)", stage, dir,
                     PL_DEF(cfg->kernel->name, "unknown"), PL_DEF(cfg->window->name, "unknown"));
    } else {
        sh_describef(sh, "%s %sscaling (%s)", stage, dir, PL_DEF(cfg->kernel->name, "unknown"));
    }
}

// Flags of one polar tap, or -1 if it is pruned at generation time
// (polar_sample, sampling.c:508-522)
static int polar_tap_flags(pl_filter filter, int x, int y, bool use_ar)
{
    const int yy = y > 0 ? y - 1 : y;
    const int xx = x > 0 ? x - 1 : x;
    const float dmin = sqrt(xx * xx + yy * yy);
    if (dmin >= filter->radius)
        return -1;
    int fl = 0;
    if (dmin >= filter->radius - M_SQRT2)
        fl |= PLH_TAP_SKIPPABLE;
    if (use_ar && dmin < filter->radius_zero)
        fl |= PLH_TAP_AR;
    return fl;
}

static int add_tap(uint32_t *taps, int n, pl_filter filter, int x, int y, bool use_ar)
{
    const int fl = polar_tap_flags(filter, x, y, use_ar);
    if (fl >= 0)
        taps[n++] = PLH_TAP_PACK(x, y, fl);
    return n;
}

// Evaluation order of the compute-shader formulation (sampling.c:776-783)
static int polar_taps_compute(uint32_t *taps, pl_filter filter, int bound, bool use_ar)
{
    int n = 0;
    for (int y = 1 - bound; y <= bound; y++) {
        for (int x = 1 - bound; x <= bound; x++)
            n = add_tap(taps, n, filter, x, y, use_ar);
    }
    return n;
}

// Evaluation order of the textureGather formulation (sampling.c:798-893),
// which the reference uses for radius >= 6 or when compute is unavailable
static int polar_taps_gather(uint32_t *taps, pl_filter filter, int bound, bool use_ar,
                             const struct pl_glsl_version *glsl)
{
    int n = 0;
    uint64_t gathered_cur = 0x0, gathered_next = 0x0;
    const float radius2 = PL_SQUARE(filter->radius);
    const int base = bound - 1;

    for (int y = 1 - bound; y <= bound; y++) {
        for (int x = 1 - bound; x <= bound; x++) {
            const uint64_t bit = 1llu << (base + x);
            if (gathered_cur & bit)
                continue; // fetched by the previous row's gather

            const int xx = x * x, xx1 = (x + 1) * (x + 1);
            const int yy = y * y, yy1 = (y + 1) * (y + 1);
            bool use_gather = PL_MAX(xx, xx1) + PL_MAX(yy, yy1) < radius2;
            use_gather &= PL_MAX(x, y) <= glsl->max_gather_offset;
            use_gather &= PL_MIN(x, y) >= glsl->min_gather_offset;
            if (!use_gather) {
                n = add_tap(taps, n, filter, x, y, use_ar);
                continue;
            }

            // 2x2 quad, counter-clockwise from the bottom left
            static const int xo[4] = {0, 1, 1, 0};
            static const int yo[4] = {1, 1, 0, 0};
            for (int p = 0; p < 4; p++) {
                if (x + xo[p] > bound || y + yo[p] > bound)
                    continue;
                if (!yo[p] && (gathered_cur & (bit << xo[p])))
                    continue;
                n = add_tap(taps, n, filter, x + xo[p], y + yo[p], use_ar);
            }

            gathered_next |= bit | (bit << 1);
            x++;
        }
        gathered_cur = gathered_next;
        gathered_next = 0;
    }
    return n;
}

/* ---- launch geometry of a polar pass ---------------------------------------------------------- */

#define POLAR_LDS_LIMIT (160 * 1024)    // CDNA4: LDS per CU
#define POLAR_LUT_BYTES 2048            // the 256 weight pairs in front of the texels
static const float polar_margin = 1e-5;

// k_polar_band (csrc/hip/k_polar_band.hip): the footprint walked through a ring of source rows.
// An out_w x out_h tile of output pixels, one per lane, has base texels on at most
//   span = ceil(out_h / ratio_y) + 1 rows, + 2 of rounding slack (one per side, as k_polar's tile)
// and the taps of one turn of the walk lie on two rows, so a turn reads span + 1 rows; the one new
// row of the next turn is staged meanwhile: ring_rows = span + 2. A ring row holds the tile's
// whole width, ceil(out_w / ratio_x) + 1 + (2 bound - 1) + 2 texels, and that is what costs: the
// output tile is narrowed until ring and LUT fit `max_lds` (16 x 1 fits at 16x with bound 32 and
// fp32 texels: 322 x 21 texels = 106 KiB).
struct polar_band_plan {
    int out_w, out_h;
    int ring_rows, ring_w;
    size_t lds;
};

static bool polar_band_plan(float ratio_x, float ratio_y, int bound, size_t texel, size_t max_lds,
                            struct polar_band_plan *out)
{
    static const int shapes[][2] = { {32, 8}, {32, 4}, {32, 2}, {32, 1}, {16, 1} };
    // the reference's own cap (sampling.c:671-674): a row of 2 bound - 1 gathers in a 64-bit mask
    if (bound < 1 || 2 * bound - 1 >= 64 || !(ratio_x > 0) || !(ratio_y > 0))
        return false;
    for (size_t i = 0; i < sizeof(shapes) / sizeof(shapes[0]); i++) {
        out->out_w = shapes[i][0];
        out->out_h = shapes[i][1];
        out->ring_w = (int) ceilf(out->out_w / ratio_x - polar_margin) + 2 * bound + 2;
        out->ring_rows = (int) ceilf(out->out_h / ratio_y - polar_margin) + 3 + 2;
        out->lds = POLAR_LUT_BYTES + (size_t) out->ring_w * out->ring_rows * texel;
        if (out->lds <= max_lds)
            return true;
    }
    return false;
}

// for tests/test_polar_band_plan.py: out = { out_w, out_h, ring_rows, ring_w, lds }
PL_API int plh_test_polar_band_plan(float ratio_x, float ratio_y, int bound, int texel, int max_lds,
                                    int *out);
int plh_test_polar_band_plan(float ratio_x, float ratio_y, int bound, int texel, int max_lds, int *out)
{
    struct polar_band_plan plan;
    if (!polar_band_plan(ratio_x, ratio_y, bound, texel, max_lds, &plan))
        return 0;
    out[0] = plan.out_w;
    out[1] = plan.out_h;
    out[2] = plan.ring_rows;
    out[3] = plan.ring_w;
    out[4] = (int) plan.lds;
    return 1;
}

// Which kernel family stages the source of a polar pass, and how: k_polar and the kernels built
// on its tile (the whole footprint of a 32 x 8*rows output tile in LDS) wherever that fits, else
// the band walk. PL_HIP_POLAR_BAND=1 plans the band walk for every pass (the A/B of the two).
struct polar_geometry {
    bool band;
    int rows, tile_w, tile_h;       // !band: k_polar's tile
    struct polar_band_plan plan;    // band
    size_t shmem;
};

static bool polar_geometry(float ratio_x, float ratio_y, int bound, size_t texel,
                           struct polar_geometry *g)
{
    // LDS tile: footprint of a 32 x (8*rows) output tile + filter support
    // (+2: one texel of rounding slack per side, see k_polar.hip)
    const int padding = 2 * bound - 1;
    const size_t max_lds = POLAR_LDS_LIMIT / 2; // keep two workgroups per CU resident
    g->rows = 4;
    for (;;) {
        g->tile_w = (int) ceilf(POLAR_BW / ratio_x - polar_margin) + padding + 1 + 2;
        g->tile_h = (int) ceilf(POLAR_BH * g->rows / ratio_y - polar_margin) + padding + 1 + 2;
        if (POLAR_LUT_BYTES + (size_t) g->tile_w * g->tile_h * texel <= max_lds || g->rows == 1)
            break;
        g->rows >>= 1;
    }
    g->shmem = POLAR_LUT_BYTES + (size_t) g->tile_w * g->tile_h * texel;
    g->band = g->shmem > POLAR_LDS_LIMIT || plh_switch(PLH_SW_POLAR_BAND) == 1;
    if (!g->band)
        return true;
    if (!polar_band_plan(ratio_x, ratio_y, bound, texel, POLAR_LDS_LIMIT, &g->plan))
        return false;
    g->shmem = g->plan.lds;
    return true;
}

// What a polar request resolves to before anything is recorded: the sampler object with the
// (widened) filter generated, and the launch geometry
struct polar_request {
    struct sh_sampler_obj *obj;
    struct pl_filter_config cfg;
    float ratio_x, ratio_y;
    int bound;
    bool fp32_tile;
    bool over_capacity;     // the radius is beyond the reference's cap: no geometry
    struct polar_geometry geo;
};

// Touches `sh` only to fail it (an object of the wrong kind, no memory)
static bool polar_request(pl_shader sh, const struct pl_sample_src *src,
                          const struct pl_sample_filter_params *params, bool force_f16_tile,
                          struct polar_request *rq)
{
    memset(rq, 0, sizeof(*rq));
    const struct src_geometry sg = src_geometry(src);
    if (!sg.out_w || !sg.out_h)
        return false;   // (setup_src words it)
    rq->ratio_x = sg.out_w / fabs(sg.src_w);
    rq->ratio_y = sg.out_h / fabs(sg.src_h);

    rq->obj = SH_OBJ(sh, params->lut, PL_SHADER_OBJ_SAMPLER, struct sh_sampler_obj, sh_sampler_uninit);
    if (!rq->obj) {
        SH_FAIL(sh, "pl_shader_sample_polar requires `params->lut` state");
        return false;
    }
    struct sh_sampler_obj *obj = rq->obj;

    float inv_scale = 1.0 / PL_MIN(rq->ratio_x, rq->ratio_y);
    inv_scale = PL_MAX(inv_scale, 1.0);
    if (params->no_widening)
        inv_scale = 1.0;

    rq->cfg = params->filter;
    rq->cfg.antiring = PL_DEF(rq->cfg.antiring, params->antiring);
    rq->cfg.blur = PL_DEF(rq->cfg.blur, 1.0f) * inv_scale;
    if (!obj->filter || !pl_filter_config_eq(&obj->filter->params.config, &rq->cfg)) {
        pl_filter_free(&obj->filter);
        // (its LUT and tap list go with it: sample_polar builds them for the new filter)
        pl_buf_destroy(SH_GPU(sh), &obj->lut);
        obj->filter = pl_filter_generate(sh->log, pl_filter_params(
            .config         = rq->cfg,
            .lut_entries    = SCALER_LUT_SIZE,
            .cutoff         = SCALER_LUT_CUTOFF,
        ));
        if (!obj->filter) {
            SH_FAIL(sh, "Failed initializing polar filter!");
            return false;
        }
    }

    rq->bound = ceil(obj->filter->radius);
    // the LDS texels are f16 only where that is lossless: an rgba16hf source, or the fused
    // PASS A whose result the reference rounds to an rgba16hf FBO anyway. unorm8/16 and fp32
    // sources are staged as fp32 (k/255 and k/65535 are not f16 numbers)
    const pl_fmt sfmt = src->tex->params.format;
    const bool f16_src = sfmt->type == PL_FMT_FLOAT && sfmt->component_depth[0] == 16;
    rq->fp32_tile = !force_f16_tile && !f16_src;
    rq->over_capacity = 2 * rq->bound - 1 >= 64 || rq->bound > 127 ||
        !polar_geometry(rq->ratio_x, rq->ratio_y, rq->bound, rq->fp32_tile ? 16 : 8, &rq->geo);
    return true;
}

static bool sample_polar(pl_shader sh, const struct pl_sample_src *src,
                         const struct pl_sample_filter_params *params, bool force_f16_tile);

bool pl_shader_sample_polar(pl_shader sh, const struct pl_sample_src *src,
                            const struct pl_sample_filter_params *params)
{
    return sample_polar(sh, src, params, false);
}

static bool sample_polar(pl_shader sh, const struct pl_sample_src *src,
                         const struct pl_sample_filter_params *params, bool force_f16_tile)
{
    if (!params->filter.polar) {
        SH_FAIL(sh, "Trying to use polar sampling with a non-polar filter?");
        return false;
    }

    struct src_info info;
    if (!setup_src(sh, src, &info, false, REQ_FASTEST))
        return false;

    pl_gpu gpu = SH_GPU(sh);
    struct polar_request rq;
    if (!polar_request(sh, src, params, force_f16_tile, &rq))
        return false;
    struct sh_sampler_obj *obj = rq.obj;
    const struct pl_filter_config cfg = rq.cfg;

    describe_filter(sh, &cfg, "polar", info.ratio_x, info.ratio_y);
    pl_filter filter = obj->filter;
    const bool use_ar = cfg.antiring > 0;
    const int bound = rq.bound;
    if (rq.over_capacity) {
        SH_FAIL(sh, "Polar radius %f exceeds implementation capacity!", filter->radius);
        return false;
    }

    // The reference switches from the LDS formulation to the gather one at
    // radius 6 (sampling.c:671-674); both run on the same LDS kernel here, but
    // the tap *order* (hence fp32 summation order) follows the reference's pick
    const struct pl_glsl_version glsl = sh_glsl(sh);
    const bool gather_order = params->no_compute || !(filter->radius < 6.0);

    if (!obj->lut || !obj->polar.taps || obj->taps_gather != gather_order) {
        // weight LUT as {L[i], L[min(i+1, 255)]} pairs: one ds_read_b64 per tap
        float pairs[2 * SCALER_LUT_SIZE];
        for (int i = 0; i < SCALER_LUT_SIZE; i++) {
            pairs[2 * i + 0] = filter->weights[i];
            pairs[2 * i + 1] = filter->weights[PL_MIN(i + 1, SCALER_LUT_SIZE - 1)];
        }

        const int max_taps = 4 * bound * bound;
        uint32_t *taps = malloc(max_taps * sizeof(uint32_t));
        if (!taps)
            return false;
        obj->num_taps = gather_order ? polar_taps_gather(taps, filter, bound, use_ar, &glsl)
                                     : polar_taps_compute(taps, filter, bound, use_ar);
        obj->taps_gather = gather_order;
        obj->polar.filter_gen++;

        pl_buf_destroy(gpu, &obj->lut);
        pl_buf_destroy(gpu, &obj->polar.taps);
        obj->lut = pl_buf_create(gpu, pl_buf_params(
            .size = sizeof(pairs), .storable = true, .initial_data = pairs));
        obj->polar.taps = pl_buf_create(gpu, pl_buf_params(
            .size = PL_MAX(obj->num_taps, 1) * sizeof(uint32_t), .storable = true,
            .initial_data = taps));
        free(taps);
        if (!obj->lut || !obj->polar.taps) {
            SH_FAIL(sh, "Failed initializing polar LUT!");
            return false;
        }
    }

    // k_polar's tile, or the band walk where that is above the LDS (polar_geometry)
    const struct polar_geometry *geo = &rq.geo;
    const bool fp32_tile = rq.fp32_tile;
    if (geo->band)
        sh_try_compute(sh, geo->plan.out_w, geo->plan.out_h, false, 0);
    else
        sh_try_compute(sh, POLAR_BW, POLAR_BH * geo->rows, false, 0);
    sh->shmem = geo->shmem;

    struct plh_sampler_args *s = &sh->pass.s;
    s->type = PLH_SAMPLE_POLAR;
    s->lut = pl_hip_buf_ptr(obj->lut);
    s->taps = pl_hip_buf_ptr(obj->polar.taps);
    s->num_taps = obj->num_taps;
    s->bound = bound;
    s->radius = filter->radius;
    s->rcp_radius = 1.0f / filter->radius;
    s->radius_zero = filter->radius_zero;
    s->antiring = cfg.antiring;
    s->tile_w = geo->band ? geo->plan.ring_w : geo->tile_w;
    s->tile_h = geo->band ? geo->plan.ring_rows : geo->tile_h;
    s->tile_rows = geo->band ? 1 : geo->rows;
    s->tile_fp32 = fp32_tile;
    s->band_rows = geo->band ? geo->plan.ring_rows : 0;
    s->band_w = geo->plan.ring_w;
    s->band_out_w = geo->plan.out_w;
    s->band_out_h = geo->plan.out_h;
    s->pp = NULL;
    // (anti-ringing needs per-pixel d, see k_polar; the band walk has no tables either)
    sh->polar_obj = use_ar || geo->band ? NULL : &obj->polar;
    sh_hold(sh, *params->lut);

    if (geo->band) {
        sh_listf(sh, "sample_polar(filter=%s, radius=%f, radius_zero=%f, taps=%d (%s order), "
                 "band: ring=%dx%d %s, %zu B of LDS, %dx%d outputs per workgroup, antiring=%g, "
                 "scale=%g, mask=0x%x)\n",
                 PL_DEF(cfg.name, "custom"), filter->radius, filter->radius_zero, obj->num_taps,
                 gather_order ? "gather" : "compute", geo->plan.ring_w, geo->plan.ring_rows,
                 fp32_tile ? "f32" : "f16", geo->shmem, geo->plan.out_w, geo->plan.out_h,
                 cfg.antiring, info.scale, info.comp_mask);
        return true;
    }
    sh_listf(sh, "sample_polar(filter=%s, radius=%f, radius_zero=%f, taps=%d (%s order), "
             "tile=%dx%d %s, rows=%d, antiring=%g, scale=%g, mask=0x%x)\n",
             PL_DEF(cfg.name, "custom"), filter->radius, filter->radius_zero, obj->num_taps,
             gather_order ? "gather" : "compute", geo->tile_w, geo->tile_h, fp32_tile ? "f32" : "f16",
             geo->rows, cfg.antiring, info.scale, info.comp_mask);
    return true;
}


/* ---- PASS A fusion ------------------------------------------------------------------------------ */

// an op that may run per source texel in the polar kernels' tile staging: not position
// dependent, and not one that lives in a kernel of its own (the Dolby Vision ops, rounded
// corners, the colour map's diagnostics: plh_op_generic_only)
static bool polar_fusable_op(int kind)
{
    return kind != PLH_OP_DITHER && kind != PLH_OP_PEAK_DETECT && kind != PLH_OP_PLANE_FETCH &&
           !plh_op_generic_only(kind);
}

// for tests/test_colormap_viz_plan.py
PL_API int plh_test_polar_fusable_ops(const int *kinds, int n);
int plh_test_polar_fusable_ops(const int *kinds, int n)
{
    for (int i = 0; i < n; i++) {
        if (!polar_fusable_op(kinds[i]))
            return 0;
    }
    return 1;
}

/* ---- mirrored addressing of the fast separable kernels ------------------------------------------ */

// k_ortho_fast / k_lowpass2 address a mirrored tap with ONE reflection (of_tap, k_ortho.hip), which
// is GL_MIRRORED_REPEAT only for an index in [-n, 2n). May it serve every tap of every pixel of this
// pass? From the kernel's own expressions over the rect's corners (a pixel's position is a blend of
// them):
//   along the filtered axis   fl = floor(pos * n_axis - 0.5); taps fl - (N/2 - 1) .. fl + N/2, and
//                             fl + N/2 + 1 where two pixels share a window (k_ortho_fast, `extra`)
//   across it                 floor(pos * n_across)
// each with one texel of margin for the float32 rounding of the per-pixel blend. The texture also
// has to hold two windows (n_axis >= 2 N), as ever.
int plh_ortho_one_reflection(int n_axis, int n_across, int row_size, const float pos[4][2], int dir)
{
    if (n_axis < 1 || n_across < 1 || row_size < 1 || n_axis < 2 * row_size)
        return 0;
    const int a = dir ? 1 : 0, o = 1 - a;
    double lo_a = INFINITY, hi_a = -INFINITY, lo_o = INFINITY, hi_o = -INFINITY;
    for (int c = 0; c < 4; c++) {
        const double fa = floor((double) pos[c][a] * n_axis - 0.5);
        const double fo = floor((double) pos[c][o] * n_across);
        if (!isfinite(fa) || !isfinite(fo))
            return 0;
        lo_a = fmin(lo_a, fa); hi_a = fmax(hi_a, fa);
        lo_o = fmin(lo_o, fo); hi_o = fmax(hi_o, fo);
    }
    const int half = row_size / 2;
    return lo_a - (half - 1) - 1 >= -(double) n_axis && hi_a + (half + 1) + 1 <= 2.0 * n_axis - 1 &&
           lo_o - 1 >= -(double) n_across && hi_o + 1 <= 2.0 * n_across - 1;
}

// for tests/test_ortho_mirror_guard.py
PL_API int plh_test_ortho_one_reflection(int n_axis, int n_across, int row_size, const float *pos, int dir);
int plh_test_ortho_one_reflection(int n_axis, int n_across, int row_size, const float *pos, int dir)
{
    return plh_ortho_one_reflection(n_axis, n_across, row_size, (const float (*)[2]) pos, dir);
}

bool plh_shader_sample_polar_fused(pl_shader sh, const pl_shader pre,
                                   const struct pl_sample_src *src,
                                   const struct pl_sample_filter_params *params)
{
    const struct plh_pass *pp = &pre->pass;
    pl_tex tex = pre->src_tex;
    if (!tex || pre->failed || pre->kind != PLH_SHADER_PASS || pre->detect_peak)
        return false;
    // `pre` must be an identity fetch of the whole texture: then FBO texel (i, j) would hold
    // f16(ops(texel (i, j))), including what clamped reads beyond the edges see
    if (pp->s.type != PLH_SAMPLE_NEAREST && !(pp->s.type == PLH_SAMPLE_BILINEAR && pp->s.rect_on_grid))
        return false;
    const pl_rect2df *rc = &pre->src_rect;
    if (rc->x0 != 0 || rc->y0 != 0 || rc->x1 != tex->params.w || rc->y1 != tex->params.h)
        return false;
    int ow, oh;
    if (pl_shader_output_size(pre, &ow, &oh) && (ow != tex->params.w || oh != tex->params.h))
        return false;
    if (src->tex->params.w != tex->params.w || src->tex->params.h != tex->params.h)
        return false; // `src->tex` is the FBO the caller would have rendered `pre` into
    const bool scaled = pp->s.scale != 1.0f;
    if (pp->num_pre_ops || pp->num_ops + scaled > PLH_MAX_OPS - 6)
        return false;
    for (int i = 0; i < pp->num_ops; i++) {
        if (!polar_fusable_op(pp->ops[i].kind))
            return false;
    }

    struct pl_sample_src fsrc = *src;
    fsrc.tex = tex;
    fsrc.address_mode = pp->s.address_mode;
    // the band walk stages a source texel more than once and takes no pre-ops: such a request
    // (and one beyond the radius cap, which pl_shader_sample_polar words) reads an intermediate
    struct polar_request rq;
    if (!polar_request(sh, &fsrc, params, true, &rq) || rq.over_capacity || rq.geo.band)
        return false;
    if (!sample_polar(sh, &fsrc, params, true))
        return false;

    // sample -> * scale -> ops, per source texel; the f16 tile rounds like the FBO store would
    struct plh_pass *p = &sh->pass;
    int n = 0;
    if (scaled) {
        struct plh_op *op = &p->ops[n++];
        memset(op, 0, sizeof(*op));
        op->kind = PLH_OP_SCALE;
        op->f[0] = op->f[1] = op->f[2] = op->f[3] = pp->s.scale;
    }
    memcpy(&p->ops[n], pp->ops, pp->num_ops * sizeof(struct plh_op));
    n += pp->num_ops;
    p->num_pre_ops = p->num_ops = n;
    for (int i = 0; i < pre->num_held; i++)
        sh_hold(sh, pre->held[i]);
    sh_listf(sh, "fused_pre_ops(%d ops of '%s' run per source texel, f16 tile)\n", n,
             sh_description(pre));
    return true;
}

/* ---- separable (orthogonal) filters: pl_shader_sample_ortho2, sampling.c:950-1104 -------- */

// The axis a separable pass filters along: the one whose size changes. -1 if both do.
enum ortho_axis { ORTHO_VERT = 0, ORTHO_HORIZ = 1 };
static int ortho_axis_of(const struct src_info *info, float *ratio)
{
    const bool keeps_x = fabs(info->ratio_x - 1.0f) < 1e-6f;
    const bool keeps_y = fabs(info->ratio_y - 1.0f) < 1e-6f;
    if (keeps_x) {
        *ratio = info->ratio_y;
        return ORTHO_VERT;
    }
    if (keeps_y) {
        *ratio = info->ratio_x;
        return ORTHO_HORIZ;
    }
    return -1;
}

// The filter a pass runs: the caller's, with the renderer-wide anti-ringing as its default and
// its kernel stretched by the downscaling factor (a downscale by k sums over k times the
// support) unless widening is switched off.
static struct pl_filter_config effective_filter(const struct pl_sample_filter_params *params, float ratio)
{
    struct pl_filter_config cfg = params->filter;
    float stretch = 1.0 / ratio;
    if (stretch < 1.0f || params->no_widening)
        stretch = 1.0;
    if (!cfg.antiring)
        cfg.antiring = params->antiring;
    cfg.blur = (cfg.blur ? cfg.blur : 1.0f) * stretch;
    return cfg;
}

// Rows of the weight table as the kernel reads them. Filters without negative lobes use the
// "linear trick" (sampling.c:914-942): taps are fetched in pairs through the bilinear unit, so
// a row holds (w0 + w1, w1 / (w0 + w1)) per pair, the padding repeating the last group.
static float *ortho_rows(pl_filter filt, bool paired)
{
    const int taps = filt->row_size, stride = filt->row_stride;
    const size_t entries = (size_t) SCALER_LUT_SIZE * stride;
    float *rows = malloc(entries * sizeof(float));
    if (!rows)
        return NULL;
    memcpy(rows, filt->weights, entries * sizeof(float));
    if (!paired)
        return rows;
    for (int phase = 0; phase < SCALER_LUT_SIZE; phase++) {
        float *row = rows + (size_t) phase * stride;
        for (int t = 0; t < taps; t += 2) {
            const float sum = row[t] + row[t + 1];
            row[t + 1] = row[t + 1] / sum;
            row[t] = sum;
        }
        for (int t = (taps + 1) & ~1; t < stride; t++)
            row[t] = t >= 4 ? row[t - 4] : 0.0f;
    }
    return rows;
}

bool pl_shader_sample_ortho2(pl_shader sh, const struct pl_sample_src *src,
                             const struct pl_sample_filter_params *params)
{
    if (params->filter.polar) {
        SH_FAIL(sh, "Trying to use separated sampling with a polar filter?");
        return false;
    }
    struct src_info info;
    if (!setup_src(sh, src, &info, false, REQ_LINEAR))
        return false;
    float ratio;
    const int pass = ortho_axis_of(&info, &ratio);
    if (pass < 0) {
        SH_FAIL(sh, "Trying to use pl_shader_sample_ortho with a pl_sample_src that requires "
                "scaling in multiple directions (rx=%f, ry=%f), this is not possible!",
                info.ratio_x, info.ratio_y);
        return false;
    }

    // state: one sampler object per axis, the horizontal one hanging off the vertical one
    // (anamorphic content filters the two axes differently, sampling.c:985-995)
    pl_gpu gpu = SH_GPU(sh);
    struct sh_sampler_obj *obj = SH_OBJ(sh, params->lut, PL_SHADER_OBJ_SAMPLER,
                                        struct sh_sampler_obj, sh_sampler_uninit);
    if (obj && pass == ORTHO_HORIZ)
        obj = SH_OBJ(sh, &obj->pass2, PL_SHADER_OBJ_SAMPLER, struct sh_sampler_obj, sh_sampler_uninit);
    if (!obj)
        return false;

    const struct pl_filter_config cfg = effective_filter(params, ratio);
    const bool update = !obj->filter || !pl_filter_config_eq(&obj->filter->params.config, &cfg);
    if (update) {
        pl_filter_free(&obj->filter);
        obj->filter = pl_filter_generate(sh->log, pl_filter_params(
            .config = cfg, .lut_entries = SCALER_LUT_SIZE, .row_stride_align = 4,
            .max_row_size = gpu->limits.max_tex_2d_dim / 4,
        ));
        if (!obj->filter) {
            SH_FAIL(sh, "Failed initializing separated filter!");
            return false;
        }
    }
    pl_filter filt = obj->filter;
    const int N = filt->row_size, stride = filt->row_stride;
    // no negative lobe = the first zero crossing is the radius: pairs of taps per fetch, and
    // nothing for anti-ringing to clamp
    const bool use_linear = filt->radius == filt->radius_zero;
    const bool use_ar = cfg.antiring > 0 && ratio > 1.0 && !use_linear;

    if (update || !obj->lut) {
        float *rows = ortho_rows(filt, use_linear);
        if (!rows)
            return false;
        pl_buf_destroy(gpu, &obj->lut);
        obj->lut = pl_buf_create(gpu, pl_buf_params(
            .size = (size_t) SCALER_LUT_SIZE * stride * sizeof(float), .storable = true,
            .initial_data = rows));
        free(rows);
        if (!obj->lut) {
            SH_FAIL(sh, "Failed initializing separated LUT!");
            return false;
        }
    }

    describe_filter(sh, &cfg, pass ? "ortho (horiz)" : "ortho (vert)", ratio, ratio);

    // A texture unit returns the texel itself at texel centres (its fixed-point weights snap
    // to zero). Along the filtered axis every tap is fetched at a centre by construction;
    // across it the fetch is at a centre when the pass is 1:1 on the texel grid there.
    const float r0 = pass ? src->rect.y0 : src->rect.x0;
    const bool aligned = r0 == truncf(r0);

    struct plh_sampler_args *s = &sh->pass.s;
    s->type = PLH_SAMPLE_ORTHO;
    s->weights = pl_hip_buf_ptr(obj->lut);
    s->row_size = N;
    s->row_stride = stride;
    s->dir = pass ? 0 : 1;      // 0 = horizontal, 1 = vertical
    s->use_linear = use_linear;
    s->use_ar = use_ar;
    s->antiring = cfg.antiring;
    s->linear = !aligned;       // bilinear across the filtered axis
    sh_hold(sh, *params->lut);

    sh_listf(sh, "sample_ortho(filter=%s, dir=%s, taps=%d, stride=%d, linear_trick=%d, "
             "antiring=%g, scale=%g, mask=0x%x, across=%s)\n", PL_DEF(cfg.name, "custom"),
             pass ? "horiz" : "vert", N, stride, use_linear, use_ar ? cfg.antiring : 0.0f,
             info.scale, info.comp_mask, aligned ? "nearest" : "linear");
    return true;
}

/* ---- debanding: pl_shader_deband, sampling.c:183-275 ---------------------------------------- */

void pl_shader_deband(pl_shader sh, const struct pl_sample_src *src,
                      const struct pl_deband_params *params)
{
    struct src_info info;
    if (!setup_src(sh, src, &info, false, REQ_NEAREST))
        return;

    params = PL_DEF(params, &pl_deband_default_params);
    sh_describef(sh, "debanding");

    struct plh_sampler_args *s = &sh->pass.s;
    s->type = PLH_SAMPLE_DEBAND;
    s->linear = false;
    s->comp_mask = info.comp_mask & ~0x8u; // ignore alpha channel
    s->iterations = s->comp_mask ? PL_MAX(params->iterations, 0) : 0;
    s->db_radius = params->radius;
    s->db_threshold = params->threshold / (1000 * info.scale);
    s->db_grain = s->comp_mask && params->grain > 0 ? params->grain / (1000.0 * info.scale) : 0.0f;
    for (int c = 0, k = 0; c < 3; c++) {
        // grain_neutral is indexed by *enabled* component (sampling.c:258-261)
        if (s->comp_mask & (1u << c))
            s->db_neutral[c] = params->grain_neutral[k++] / info.scale;
    }
    s->prng_seed = sh->params.index;
    // (k_deband_lds stages a 98 x 66 texel window: not where the user has lowered the limit)
    s->db_lds = !SH_GPU(sh) || SH_GPU(sh)->glsl.max_shmem_size >= 52 * 1024;

    sh_listf(sh, "deband(iterations=%d, threshold=%g, radius=%g, grain=%g, scale=%g, "
             "mask=0x%x, seed=%u)\n", s->iterations, params->threshold, params->radius,
             params->grain, info.scale, s->comp_mask, s->prng_seed);
}

/* ---- pl_shader_distort (reference src/shaders/sampling.c:1106-1217) ---------------------------- */

const struct pl_distort_params pl_distort_default_params = { PL_DISTORT_DEFAULTS };

void pl_shader_distort(pl_shader sh, pl_tex src_tex, int out_w, int out_h,
                       const struct pl_distort_params *params)
{
    if (!params || !src_tex) {
        SH_FAIL(sh, "pl_shader_distort: parameters and a texture are required");
        return;
    }
    if (sh->pass.s.type != PLH_SAMPLE_NONE || sh->output != PL_SHADER_SIG_NONE) {
        SH_FAIL(sh, "Illegal sequence of shader operations: a sampling stage must "
                "be the first stage of a shader");
        return;
    }
    if (!sh_require(sh, PL_SHADER_SIG_NONE, out_w, out_h))
        return;

    // the image in aspect-normalised coordinates: its longer side spans [-1, 1], y up
    const int src_w = src_tex->params.w, src_h = src_tex->params.h;
    float rx = 1.0f, ry = 1.0f;
    if (src_w > src_h) {
        ry = (float) src_h / src_w;
    } else {
        rx = (float) src_w / src_h;
    }
    const pl_transform2x2 tex2norm = {
        .mat.m = {{ 2 * rx, 0 }, { 0, -2 * ry }},
        .c = { -rx, ry },
    };
    // ... and from there to the canvas [-1, 1]^2
    const float sx = params->unscaled ? (float) src_w / out_w : 1.0f;
    const float sy = params->unscaled ? (float) src_h / out_h : 1.0f;
    const pl_transform2x2 norm2canvas = {
        .mat.m = {{ sx / rx, 0 }, { 0, sy / ry }},
    };

    pl_transform2x2 transform = params->transform;
    pl_transform2x2_mul(&transform, &tex2norm);
    pl_transform2x2_rmul(&norm2canvas, &transform);
    if (params->constrain) {
        const pl_rect2df unit = { .x1 = 1, .y1 = 1 };
        const pl_rect2df bb = pl_transform2x2_bounds(&transform, &unit);
        const float k = fmaxf(fmaxf(pl_rect_w(bb), pl_rect_h(bb)), 2.0f);
        pl_transform2x2_scale(&transform, 2.0f / k);
    }

    // the kernel walks the canvas (a vertex attribute in the reference, :1156-1161: y runs from +1
    // at the top row to -1) and needs the way back: canvas -> texture coordinates
    if (!sh_bind(sh, src_tex, params->address_mode, NULL))
        return;
    pl_transform2x2_invert(&transform);
    sh_describef(sh, "distortion");

    struct plh_pass *pass = &sh->pass;
    struct plh_sampler_args *s = &pass->s;
    s->type = PLH_SAMPLE_DISTORT;
    s->pos[0][0] = -1.0f; s->pos[0][1] =  1.0f;
    s->pos[1][0] =  1.0f; s->pos[1][1] =  1.0f;
    s->pos[2][0] = -1.0f; s->pos[2][1] = -1.0f;
    s->pos[3][0] =  1.0f; s->pos[3][1] = -1.0f;
    s->scale = 1.0f;
    s->comp_mask = 0xf;
    s->linear = true;
    pass->distort = (struct plh_distort_args) {
        .m = { transform.mat.m[0][0], transform.mat.m[0][1],
               transform.mat.m[1][0], transform.mat.m[1][1] },
        .c = { transform.c[0], transform.c[1] },
        .bicubic = params->bicubic,
        .alpha_mode = params->alpha_mode,
    };
    sh_listf(sh, "distort(tf=[%g %g; %g %g] + (%g, %g)%s%s)\n", pass->distort.m[0],
             pass->distort.m[1], pass->distort.m[2], pass->distort.m[3], pass->distort.c[0],
             pass->distort.c[1], params->bicubic ? ", bicubic" : "",
             params->alpha_mode ? ", transparent outside" : "");
}
