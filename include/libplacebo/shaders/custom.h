/*
 * libplacebo-hip: renderer hooks (pl_render_params.hooks) and the custom-shader entry points.
 * Layout-compatible with the reference's src/include/libplacebo/shaders/custom.h
 * (pl_custom_shader :36-95, pl_hook_stage :106-129, pl_hook_sig :160-165, pl_hook_params :167-226,
 * pl_hook_res :228-259, pl_hook_par :276-299, pl_hook :305-327; tests/test_hooks_abi.py).
 *
 * A pl_hook is a C struct with a C callback: the renderer calls it at each of the sixteen stages
 * its `stages` mask names. There is no run-time shader compiler on this backend (INTEGRATION.md
 * section 2), so the two ways of MAKING a hook from shader text are exported but always fail:
 * pl_shader_custom and pl_mpv_user_shader_parse. A hook the caller writes in C works, and has
 * three ways of computing ("Hooks"):
 *   - PL_HOOK_SIG_COLOR: append the library's own pl_shader_* operations to `params->sh`;
 *   - run passes of its own through `params->dispatch` into textures from `params->get_tex`;
 *   - PL_HOOK_SIG_TEX: launch its own HIP kernels on pl_hip_get(gpu)->stream, reading
 *     `params->tex` and writing a texture from `get_tex` (device pointers: pl_hip_tex_ptr), each
 *     announced with pl_hip_tex_access first (hip.h).
 */
#ifndef LIBPLACEBO_SHADERS_CUSTOM_H_
#define LIBPLACEBO_SHADERS_CUSTOM_H_

#include <stdlib.h>

#include <libplacebo/colorspace.h>
#include <libplacebo/dispatch.h>
#include <libplacebo/shaders.h>

PL_API_BEGIN

// Shader text to embed into a pl_shader. Carried for layout compatibility only.
struct pl_custom_shader {
    const char *prelude;        // before the input declarations (#extension, #define)
    const char *header;         // helper functions, extra uniforms
    const char *description;    // friendly name
    const char *body;           // appended to main()
    enum pl_shader_sig input;
    enum pl_shader_sig output;

    const struct pl_shader_desc *descriptors;
    int num_descriptors;
    const struct pl_shader_var *variables;
    int num_variables;
    const struct pl_shader_va *vertex_attribs;
    int num_vertex_attribs;
    const struct pl_shader_const *constants;
    int num_constants;

    bool compute;               // must be a compute shader ...
    size_t compute_shmem;       // ... with this much shared memory
    int compute_group_size[2];  // ... and this workgroup size (0 = any)

    int output_w;               // fixed output size (0 = any)
    int output_h;
};

// Always fails `sh` and returns false, with one error message: GLSL cannot be compiled here.
PL_API bool pl_shader_custom(pl_shader sh, const struct pl_custom_shader *params);

// The stages of pl_render_image a hook can attach to, in the order they are visited. A stage is
// "resizable" if the hook may return an image of another size (pl_hook_stage_resizable).
enum pl_hook_stage {
    // the planes as the source provides them, one call per plane of that kind (resizable)
    PL_HOOK_RGB_INPUT       = 1 << 0,
    PL_HOOK_LUMA_INPUT      = 1 << 1,
    PL_HOOK_CHROMA_INPUT    = 1 << 2,
    PL_HOOK_ALPHA_INPUT     = 1 << 3,
    PL_HOOK_XYZ_INPUT       = 1 << 4,

    // chroma / alpha planes brought onto the reference plane's grid
    PL_HOOK_CHROMA_SCALED   = 1 << 5,
    PL_HOOK_ALPHA_SCALED    = 1 << 6,

    PL_HOOK_NATIVE          = 1 << 7,  // the merged image in its native colour system (resizable)
    PL_HOOK_RGB             = 1 << 8,  // decoded to RGB (resizable)
    PL_HOOK_LINEAR          = 1 << 9,  // linear light, before scaling
    PL_HOOK_SIGMOID         = 1 << 10, // sigmoidized
    PL_HOOK_PRE_KERNEL      = 1 << 11, // what the main scaler reads
    PL_HOOK_POST_KERNEL     = 1 << 12, // what the main scaler produced
    PL_HOOK_SCALED          = 1 << 13, // at output size, before colour management
    PL_HOOK_PRE_OUTPUT      = 1 << 14, // in the target's colour space, before blending / rotation
    PL_HOOK_OUTPUT          = 1 << 15, // blended, encoded, rotated; before dithering
};

static inline bool pl_hook_stage_resizable(enum pl_hook_stage stage) {
    switch (stage) {
    case PL_HOOK_RGB_INPUT:
    case PL_HOOK_LUMA_INPUT:
    case PL_HOOK_CHROMA_INPUT:
    case PL_HOOK_ALPHA_INPUT:
    case PL_HOOK_XYZ_INPUT:
    case PL_HOOK_NATIVE:
    case PL_HOOK_RGB:
        return true;

    case PL_HOOK_CHROMA_SCALED:
    case PL_HOOK_ALPHA_SCALED:
    case PL_HOOK_LINEAR:
    case PL_HOOK_SIGMOID:
    case PL_HOOK_PRE_KERNEL:
    case PL_HOOK_POST_KERNEL:
    case PL_HOOK_SCALED:
    case PL_HOOK_PRE_OUTPUT:
    case PL_HOOK_OUTPUT:
        return false;
    }

    abort();
}

// How the image is handed to a hook, and how the hook hands it back
enum pl_hook_sig {
    PL_HOOK_SIG_NONE,   // nothing
    PL_HOOK_SIG_COLOR,  // a pl_shader whose colour is the image (recorded, not yet run)
    PL_HOOK_SIG_TEX,    // a pl_tex holding the image
    PL_HOOK_SIG_COUNT,
};

struct pl_hook_params {
    // the renderer's own objects, for the hook's use
    pl_gpu gpu;
    pl_dispatch dispatch;

    // A temporary texture from the renderer's pool: four components in the format of the
    // renderer's intermediates (rgba16hf on this backend), sampleable, renderable and storable.
    // Valid until the end of the frame; never to be destroyed by the hook. NULL if none is to be
    // had. `priv` is the member below.
    pl_tex (*get_tex)(void *priv, int width, int height);
    void *priv;

    enum pl_hook_stage stage;   // the stage that fired

    // PL_HOOK_SIG_COLOR: the image so far. Operations may be appended; it must not be
    // dispatched, finished or reset.
    pl_shader sh;

    // PL_HOOK_SIG_TEX: the image. Owned by the renderer, to be read only; its contents hold for
    // this frame.
    pl_tex tex;

    // The part of `sh` / `tex` that is the image, and what its values mean. Set for
    // PL_HOOK_SIG_NONE as well.
    pl_rect2df rect;
    struct pl_color_repr repr;
    struct pl_color_space color;
    int components;

    // the source frame's own description
    const struct pl_color_repr *orig_repr;
    const struct pl_color_space *orig_color;

    // The crops of the whole render: the image's (as earlier hooks left it) and the target's
    pl_rect2df src_rect;
    pl_rect2d dst_rect;
};

struct pl_hook_res {
    bool failed;                // the hook could not do its work: it is disabled (by signature)
    enum pl_hook_sig output;    // PL_HOOK_SIG_NONE: the image stays as it is, the rest is ignored

    pl_shader sh;               // PL_HOOK_SIG_COLOR: the image, recorded (normally params->sh)
    pl_tex tex;                 // PL_HOOK_SIG_TEX: the image (normally from params->get_tex)

    // the description of what is returned
    struct pl_color_repr repr;
    struct pl_color_space color;
    int components;
    pl_rect2df rect;            // must equal params->rect on a stage that is not resizable
};

enum pl_hook_par_mode {
    PL_HOOK_PAR_VARIABLE,
    PL_HOOK_PAR_DYNAMIC,
    PL_HOOK_PAR_CONSTANT,
    PL_HOOK_PAR_DEFINE,
    PL_HOOK_PAR_MODE_COUNT,
};

typedef union pl_var_data {
    int i;
    unsigned u;
    float f;
} pl_var_data;

// A tunable a hook exports. The renderer never looks at these: it carries the pointer.
struct pl_hook_par {
    const char *name;
    enum pl_var_type type;
    enum pl_hook_par_mode mode;
    const char *description;
    pl_var_data *data;          // current value
    pl_var_data initial;
    pl_var_data minimum;
    pl_var_data maximum;
    const char * const *names;  // of the values minimum.i .. maximum.i of an integer option
};

// Callers create these themselves.
struct pl_hook {
    enum pl_hook_stage stages;  // mask of the stages to be called at
    enum pl_hook_sig input;     // how the image is to be handed over
    void *priv;                 // passed to both callbacks

    const struct pl_hook_par *parameters;
    int num_parameters;

    // Once per rendered frame, before its first stage (optional)
    void (*reset)(void *priv);

    struct pl_hook_res (*hook)(void *priv, const struct pl_hook_params *params);

    // Identifies the hook in pl_render_errors.disabled_hooks: after a failure every hook of
    // this signature is skipped until pl_renderer_reset_errors clears it.
    uint64_t signature;
};

// mpv's user-shader format is GLSL: always NULL here, with one error message.
PL_API const struct pl_hook *
pl_mpv_user_shader_parse(pl_gpu gpu, const char *shader_text, size_t shader_len);

// Accepts NULL and a pointer to NULL.
PL_API void pl_mpv_user_shader_destroy(const struct pl_hook **hook);

PL_API_END

#endif // LIBPLACEBO_SHADERS_CUSTOM_H_
