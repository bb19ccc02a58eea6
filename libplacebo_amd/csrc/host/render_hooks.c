/*
 * libplacebo-hip — pl_render_params.hooks: the caller's C callbacks at the renderer's stages
 * (behaviour of the reference's pass_hook, src/renderer.c:1036-1181; the stages themselves are
 * fired by renderer.c where the reference fires them).
 *
 * A hook sees the image the way it asks for it (pl_hook.input): not at all, as the recording so
 * far (plh_work_shader) or as a texture (plh_work_texture: whatever is recorded runs first), and
 * hands back nothing, a recording or a texture, which then IS the image. Nothing here knows about
 * kernels: a hook that leaves a texture leaves the image resident, one that appends to the
 * recording leaves it recorded with more ops, and the fusion decisions that follow (renderer.c)
 * look at the image as they find it.
 */
#include <stdlib.h>
#include <string.h>

#include <libplacebo/hip.h>

#include "renderer_priv.h"

void plh_reset_hooks(const struct pl_render_params *params)
{
    for (int i = 0; params->hooks && i < params->num_hooks; i++) {
        if (params->hooks[i]->reset)
            params->hooks[i]->reset(params->hooks[i]->priv);
    }
}

static pl_tex hook_get_tex(void *priv, int width, int height)
{
    struct frame_job *job = priv;
    if (width <= 0 || height <= 0)
        return NULL;
    return plh_borrow_fbo(job, width, height, NULL, 4);
}

static bool hook_is_disabled(pl_renderer rr, uint64_t signature)
{
    for (int i = 0; i < rr->num_disabled_hooks; i++) {
        if (rr->disabled_hooks[i] == signature)
            return true;
    }
    return false;
}

static void hook_disable(pl_renderer rr, uint64_t signature)
{
    rr->errors |= PL_RENDER_ERR_HOOKS;
    if (hook_is_disabled(rr, signature))
        return;
    if (rr->num_disabled_hooks == rr->cap_disabled_hooks) {
        const int cap = PL_MAX(8, 2 * rr->cap_disabled_hooks);
        uint64_t *list = realloc(rr->disabled_hooks, cap * sizeof(*list));
        if (!list)
            return;     // (the error bit stands; the hook fails again next frame)
        rr->disabled_hooks = list;
        rr->cap_disabled_hooks = cap;
    }
    rr->disabled_hooks[rr->num_disabled_hooks++] = signature;
}

static bool same_rect(pl_rect2df a, pl_rect2df b)
{
    return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1;
}

// A PL_HOOK_SIG_COLOR hook appends ops to the image's recording, whose op list is finite
// (PLH_MAX_OPS, plh_device.h) and partly used. When it is full (sh_op, shaders.c) what is recorded
// runs into an intermediate and the shader the hook holds continues as a fetch of it: the ops are
// split over two passes, with the intermediate's rounding between them, none is dropped.
struct spill_ctx {
    struct frame_job *job;
    struct work_image *img;
};

static bool spill_recording(void *priv, pl_shader sh)
{
    struct spill_ctx *ctx = priv;
    struct frame_job *job = ctx->job;
    struct work_image *img = ctx->img;
    pl_renderer rr = job->rr;
    if (sh->kind != PLH_SHADER_PASS || sh->input != PL_SHADER_SIG_NONE)
        return false;

    pl_tex fbo = plh_borrow_fbo(job, img->w, img->h, NULL, img->comps);
    pl_shader run = fbo ? pl_dispatch_begin(rr->dp) : NULL;
    if (!run)
        return false;
    // the caller keeps its pointer: the recording moves to `run`, `sh` becomes the fresh shader
    struct pl_shader_t tmp = *run;
    *run = *sh;
    *sh = tmp;
    run->spill = NULL;
    run->spill_priv = NULL;
    const bool ok = pl_dispatch_finish(rr->dp, pl_dispatch_params( .shader = &run, .target = fbo ));
    if (!ok || !pl_shader_sample_direct(sh, pl_sample_src( .tex = fbo ))) {
        SH_FAIL(sh, "Failed flushing a full op list in front of a hook's operations");
        return false;
    }
    RR_LOG(rr, PL_LOG_DEBUG, "hook: op list full, image stored and continued from the copy");
    sh->spill = spill_recording;
    sh->spill_priv = priv;
    img->copy_of = fbo;
    job->peak_pending = false;      // whatever rode on the recording has run
    return true;
}

bool plh_run_hooks(struct frame_job *job, struct work_image *img, uint64_t stage)
{
    const struct pl_render_params *params = job->params;
    pl_renderer rr = job->rr;
    if (!(job->hook_stages & stage) || !job->caps.fbo[4])
        return false;

    bool applied = false;
    for (int n = 0; n < params->num_hooks; n++) {
        const struct pl_hook *hook = params->hooks[n];
        if (!(hook->stages & stage) || hook_is_disabled(rr, hook->signature))
            continue;

        struct pl_hook_params hp = {
            .gpu        = rr->gpu,
            .dispatch   = rr->dp,
            .get_tex    = hook_get_tex,
            .priv       = job,
            .stage      = (enum pl_hook_stage) stage,
            .rect       = img->rect,
            .repr       = img->repr,
            .color      = img->color,
            .components = img->comps,
            .orig_repr  = &job->image.repr,
            .orig_color = &job->image.color,
            .src_rect   = job->ref_rect,
            .dst_rect   = job->geo.dst,
        };

        struct spill_ctx spill = { job, img };
        switch (hook->input) {
        case PL_HOOK_SIG_TEX:
            hp.tex = plh_work_texture(job, img);
            job->peak_pending = false;
            if (!hp.tex) {
                RR_LOG(rr, PL_LOG_ERR, "Failed dispatching shader prior to hook!");
                goto hook_error;
            }
            break;
        case PL_HOOK_SIG_COLOR:
            hp.sh = plh_work_shader(job, img);
            hp.sh->spill = spill_recording;
            hp.sh->spill_priv = &spill;
            break;
        case PL_HOOK_SIG_NONE:
        default:
            break;
        }

        struct pl_hook_res res = hook->hook(hook->priv, &hp);
        if (hp.sh) {
            hp.sh->spill = NULL;
            hp.sh->spill_priv = NULL;
        }
        if (res.failed) {
            RR_LOG(rr, PL_LOG_ERR, "Failed executing hook, disabling");
            goto hook_error;
        }

        const bool resizable = pl_hook_stage_resizable((enum pl_hook_stage) stage);
        switch (res.output) {
        case PL_HOOK_SIG_TEX:
            if (!res.tex) {
                RR_LOG(rr, PL_LOG_ERR, "User hook returned no texture!");
                goto hook_error;
            }
            if (!resizable && (res.tex->params.w != img->w || res.tex->params.h != img->h ||
                               !same_rect(res.rect, img->rect))) {
                RR_LOG(rr, PL_LOG_ERR, "User hook tried resizing non-resizable stage!");
                goto hook_error;
            }
            // (a recording the hook did not ask to see is replaced unrun)
            pl_dispatch_abort(rr->dp, &img->rec);
            *img = (struct work_image) {
                .tex   = res.tex,
                .repr  = res.repr,
                .color = res.color,
                .comps = res.components,
                .rect  = res.rect,
                .w     = res.tex->params.w,
                .h     = res.tex->params.h,
            };
            break;

        case PL_HOOK_SIG_COLOR: {
            if (!res.sh) {
                RR_LOG(rr, PL_LOG_ERR, "User hook returned no shader!");
                goto hook_error;
            }
            int w = img->w, h = img->h;
            (void) pl_shader_output_size(res.sh, &w, &h);
            if (!resizable && (w != img->w || h != img->h || !same_rect(res.rect, img->rect))) {
                RR_LOG(rr, PL_LOG_ERR, "User hook tried resizing non-resizable stage!");
                goto hook_error;
            }
            const bool same = res.sh == img->rec;
            if (!same)
                pl_dispatch_abort(rr->dp, &img->rec);
            *img = (struct work_image) {
                .rec      = res.sh,
                .copy_of  = same ? img->copy_of : NULL,
                .repr     = res.repr,
                .color    = res.color,
                .comps    = res.components,
                .rect     = res.rect,
                .w        = w,
                .h        = h,
                .fail_bit = PL_RENDER_ERR_HOOKS,
                .fail_msg = "Failed applying user hook",
                .fail_tex = hp.tex,
            };
            break;
        }

        case PL_HOOK_SIG_NONE:
        default:
            break;
        }
        applied = true;
        continue;

hook_error:
        hook_disable(rr, hook->signature);
    }

    // the image stays usable whatever happened (:1176-1179)
    if (!img->tex && !img->rec)
        img->rec = pl_dispatch_begin(rr->dp);
    return applied;
}

/* ---- what exists of the reference's ways of making a hook from shader text ------------------ */

bool pl_shader_custom(pl_shader sh, const struct pl_custom_shader *params)
{
    (void) params;
    SH_FAIL(sh, "pl_shader_custom: this backend has no shader compiler (fixed HIP kernels, "
            "INTEGRATION.md section 2): custom GLSL cannot be embedded");
    return false;
}

const struct pl_hook *pl_mpv_user_shader_parse(pl_gpu gpu, const char *shader_text,
                                               size_t shader_len)
{
    (void) shader_text;
    (void) shader_len;
    pl_msg(gpu ? gpu->log : NULL, PL_LOG_ERR, "pl_mpv_user_shader_parse: this backend has no "
           "shader compiler (fixed HIP kernels, INTEGRATION.md section 2): mpv user shaders are "
           "GLSL; write the hook as a C callback (struct pl_hook)");
    return NULL;
}

void pl_mpv_user_shader_destroy(const struct pl_hook **hook)
{
    if (hook)
        *hook = NULL;   // (parse never returns one: there is nothing to free)
}
