/*
 * Renderer hooks for tests/test_gpu_hooks.py: `struct pl_hook` objects written the way a caller
 * writes them (in C: a hook returns `struct pl_hook_res` by value), a log of every call the
 * renderer makes, and a reset counter. Python reads the exported objects with ctypes, puts their
 * addresses into pl_render_params.hooks and may change `stages` between renders.
 *
 * The three ways a hook can compute on this backend are all here: appending the library's own
 * operations to the recorded shader (th_lut), and launching a kernel of its own on the stage
 * texture (th_invert, th_double: tests/hooks/hook_kernels.hip) into a texture from get_tex.
 */
#include <string.h>

#include <libplacebo/hip.h>
#include <libplacebo/renderer.h>
#include <libplacebo/shaders/custom.h>
#include <libplacebo/shaders/lut.h>

#define TH_EXPORT __attribute__((visibility("default")))

int th_launch_invert(void *stream, const void *src, size_t src_pitch, void *dst, size_t dst_pitch,
                     int w, int h);
int th_launch_double_nearest(void *stream, const void *src, size_t src_pitch, void *dst,
                             size_t dst_pitch, int w, int h);

/* ---- the call log ---------------------------------------------------------------------------- */

struct th_call {
    int stage;              // pl_hook_params.stage
    int tag;                // th_priv.tag of the hook that was called
    float rect[4];          // pl_hook_params.rect
    int components;
    int sys;                // repr.sys
    int transfer;           // color.transfer
    int has_tex, has_sh;    // what the renderer handed over
    int tex_w, tex_h;       // size of `tex`, if any
    float src_rect[4];
    int dst_rect[4];
};

#define TH_MAX_CALLS 512
TH_EXPORT struct th_call th_calls[TH_MAX_CALLS];
TH_EXPORT int th_num_calls;
TH_EXPORT int th_num_resets;

TH_EXPORT void th_clear(void)
{
    th_num_calls = 0;
    th_num_resets = 0;
}

// what every hook's `priv` points at
struct th_priv {
    int tag;
    int count;                          // th_lut: how many times the LUT is applied
    const struct pl_custom_lut *lut;    // th_lut
    pl_shader_obj lut_state;
};

static void note(void *priv, const struct pl_hook_params *p)
{
    if (th_num_calls >= TH_MAX_CALLS)
        return;
    struct th_call *c = &th_calls[th_num_calls++];
    *c = (struct th_call) {
        .stage = p->stage,
        .tag = priv ? ((struct th_priv *) priv)->tag : -1,
        .rect = { p->rect.x0, p->rect.y0, p->rect.x1, p->rect.y1 },
        .components = p->components,
        .sys = p->repr.sys,
        .transfer = p->color.transfer,
        .has_tex = !!p->tex,
        .has_sh = !!p->sh,
        .tex_w = p->tex ? p->tex->params.w : 0,
        .tex_h = p->tex ? p->tex->params.h : 0,
        .src_rect = { p->src_rect.x0, p->src_rect.y0, p->src_rect.x1, p->src_rect.y1 },
        .dst_rect = { p->dst_rect.x0, p->dst_rect.y0, p->dst_rect.x1, p->dst_rect.y1 },
    };
}

static void on_reset(void *priv)
{
    (void) priv;
    th_num_resets++;
}

static const struct pl_hook_res failed = { .failed = true };

static struct pl_hook_res same_image(const struct pl_hook_params *p, enum pl_hook_sig sig)
{
    return (struct pl_hook_res) {
        .output = sig,
        .sh = p->sh,
        .tex = p->tex,
        .repr = p->repr,
        .color = p->color,
        .components = p->components,
        .rect = p->rect,
    };
}

/* ---- the hooks -------------------------------------------------------------------------------- */

static struct pl_hook_res hook_silent(void *priv, const struct pl_hook_params *p)
{
    note(priv, p);
    return (struct pl_hook_res) { .output = PL_HOOK_SIG_NONE };
}

static struct pl_hook_res hook_identity_tex(void *priv, const struct pl_hook_params *p)
{
    note(priv, p);
    return p->tex ? same_image(p, PL_HOOK_SIG_TEX) : failed;
}

static struct pl_hook_res hook_fail(void *priv, const struct pl_hook_params *p)
{
    note(priv, p);
    return failed;
}

static bool is_f16_rgba(pl_tex tex)
{
    return tex && tex->params.format && !strcmp(tex->params.format->name, "rgba16hf");
}

// A kernel of the hook's own: stage texture -> texture from get_tex, on the backend's stream,
// each texture announced first (pl_hip_tex_access)
static struct pl_hook_res run_kernel(const struct pl_hook_params *p, int factor)
{
    pl_tex in = p->tex;
    if (!is_f16_rgba(in))
        return failed;
    const int w = in->params.w, h = in->params.h;
    pl_tex out = p->get_tex(p->priv, factor * w, factor * h);
    if (!is_f16_rgba(out) || out->params.w != factor * w || out->params.h != factor * h)
        return failed;

    pl_hip hip = pl_hip_get(p->gpu);
    if (!hip)
        return failed;
    pl_hip_tex_access(p->gpu, in, false);
    pl_hip_tex_access(p->gpu, out, true);
    size_t in_pitch, out_pitch;
    const void *src = pl_hip_tex_ptr(in, &in_pitch);
    void *dst = pl_hip_tex_ptr(out, &out_pitch);
    const int err = factor == 1
        ? th_launch_invert(hip->stream, src, in_pitch, dst, out_pitch, w, h)
        : th_launch_double_nearest(hip->stream, src, in_pitch, dst, out_pitch, w, h);
    if (err)
        return failed;

    struct pl_hook_res res = same_image(p, PL_HOOK_SIG_TEX);
    res.tex = out;
    res.rect = (pl_rect2df) { factor * p->rect.x0, factor * p->rect.y0,
                              factor * p->rect.x1, factor * p->rect.y1 };
    return res;
}

static struct pl_hook_res hook_invert(void *priv, const struct pl_hook_params *p)
{
    note(priv, p);
    return run_kernel(p, 1);
}

static struct pl_hook_res hook_double(void *priv, const struct pl_hook_params *p)
{
    note(priv, p);
    return run_kernel(p, 2);
}

// the library's own operations, appended to the recorded shader: a custom LUT, `count` times
static struct pl_hook_res hook_lut(void *priv, const struct pl_hook_params *p)
{
    struct th_priv *st = priv;
    note(priv, p);
    if (!p->sh || !st->lut)
        return failed;
    for (int i = 0; i < st->count; i++)
        pl_shader_custom_lut(p->sh, st->lut, &st->lut_state);
    return same_image(p, PL_HOOK_SIG_COLOR);
}

#define TH_HOOK(name, tag_, stages_, input_, fn, sig)                           \
    TH_EXPORT struct th_priv name##_priv = { .tag = tag_, .count = 1 };         \
    TH_EXPORT struct pl_hook name = {                                           \
        .stages = stages_, .input = input_, .priv = &name##_priv,               \
        .reset = on_reset, .hook = fn, .signature = sig,                        \
    }

TH_HOOK(th_identity_tex, 100, PL_HOOK_PRE_KERNEL, PL_HOOK_SIG_TEX, hook_identity_tex, 0x7e57000000000100ull);
TH_HOOK(th_invert, 101, PL_HOOK_OUTPUT, PL_HOOK_SIG_TEX, hook_invert, 0x7e57000000000101ull);
TH_HOOK(th_double, 102, PL_HOOK_RGB_INPUT, PL_HOOK_SIG_TEX, hook_double, 0x7e57000000000102ull);
TH_HOOK(th_lut, 103, PL_HOOK_RGB, PL_HOOK_SIG_COLOR, hook_lut, 0x7e57000000000103ull);
TH_HOOK(th_fail, 104, PL_HOOK_SCALED, PL_HOOK_SIG_NONE, hook_fail, 0x7e57000000000104ull);
TH_HOOK(th_count_rgb, 105, PL_HOOK_RGB, PL_HOOK_SIG_NONE, hook_silent, 0x7e57000000000105ull);
TH_HOOK(th_count_output, 106, PL_HOOK_OUTPUT, PL_HOOK_SIG_NONE, hook_silent, 0x7e57000000000106ull);

// sixteen silent hooks, one per stage (tag = the stage's bit number)
#define SILENT(i) { .stages = 1 << (i), .input = PL_HOOK_SIG_NONE, .priv = &th_silent_priv[i],  \
                    .reset = (i) ? NULL : on_reset, .hook = hook_silent,                         \
                    .signature = 0x7e57000000000000ull + (i) }
TH_EXPORT struct th_priv th_silent_priv[16] = {
    {0}, {1}, {2}, {3}, {4}, {5}, {6}, {7}, {8}, {9}, {10}, {11}, {12}, {13}, {14}, {15},
};
TH_EXPORT struct pl_hook th_silent[16] = {
    SILENT(0), SILENT(1), SILENT(2), SILENT(3), SILENT(4), SILENT(5), SILENT(6), SILENT(7),
    SILENT(8), SILENT(9), SILENT(10), SILENT(11), SILENT(12), SILENT(13), SILENT(14), SILENT(15),
};

// the device copy of th_lut's table belongs to a pl_gpu: to be released before that goes away
TH_EXPORT void th_release(void)
{
    pl_shader_obj_destroy(&th_lut_priv.lut_state);
    th_lut_priv.lut = NULL;
    th_lut_priv.count = 1;
}

// sizeof / offsets for the Python mirrors of the two structs above
TH_EXPORT int th_sizeof_call(void) { return sizeof(struct th_call); }
TH_EXPORT int th_sizeof_priv(void) { return sizeof(struct th_priv); }
