/*
 * libplacebo-hip: pl_options, the option-string front end of pl_render_params.
 * API- and layout-compatible with the reference's src/include/libplacebo/options.h
 * (pl_options_t :30-58, pl_opt_data_t :78-93, the entry points :67-133, pl_option_type and
 * pl_opt_t :143-190, the list :193-197); tests/test_options.py holds the layouts to
 * tests/golden/abi_layout_options.json and the list to tests/golden/options_list.json.
 *
 * A pl_options owns one pl_render_params together with storage for everything it points to, and
 * turns "key=value,key=value" text into that struct and back: what mpv's --libplacebo-opts and
 * plplay's settings panel are built on. Every parameter the list reaches is one the renderer
 * already honours; the ICC keys are stored and ignored (no lcms2, shaders/icc.h).
 */
#ifndef LIBPLACEBO_OPTIONS_H_
#define LIBPLACEBO_OPTIONS_H_

#include <libplacebo/renderer.h>

PL_API_BEGIN

typedef const struct pl_opt_t *pl_opt;

typedef struct pl_options_t {
    // what is handed to pl_render_image. A non-NULL `params.*_params` always points at the
    // member of the same name below, never outside this object.
    struct pl_render_params params;

    // storage behind `params.*_params`: a struct is in use while the pointer in `params` is set,
    // and keeps its values while it is not
    struct pl_deband_params deband_params;
    struct pl_sigmoid_params sigmoid_params;
    struct pl_color_adjustment color_adjustment;
    struct pl_peak_detect_params peak_detect_params;
    struct pl_color_map_params color_map_params;
    struct pl_dither_params dither_params;
    struct pl_icc_params icc_params PL_DEPRECATED_IN(v6.327);
    struct pl_cone_params cone_params;
    struct pl_blend_params blend_params;
    struct pl_deinterlace_params deinterlace_params;
    struct pl_distort_params distort_params;

    // one "custom" filter per scaler. `params.upscaler` etc. point either at a built-in
    // pl_filter_config or at the slot of the same name; a slot's `name`, `description` and
    // `allowed` are always valid for its kind of filter.
    struct pl_filter_config upscaler;
    struct pl_filter_config downscaler;
    struct pl_filter_config plane_upscaler;
    struct pl_filter_config plane_downscaler;
    struct pl_filter_config frame_mixer;
} *pl_options;

// A new options object in the "empty" configuration: PL_RENDER_DEFAULTS, which is
// pl_render_fast_params. Parse errors etc. go to `log` (may be NULL).
PL_API pl_options pl_options_alloc(pl_log log);
PL_API void pl_options_free(pl_options *opts);

// Start over from `preset`: its values, with every params struct it points to copied into `opts`,
// and a scaler that is not one of the built-in configs copied into its custom slot (all of it,
// `antiring` included; the slot keeps its own name, description and usages). Everything
// `preset` does not reach (the unused params structs, the custom slots) goes back to its default.
// NULL: the empty configuration of a fresh object.
PL_API void pl_options_reset(pl_options opts, const struct pl_render_params *preset);

typedef const struct pl_opt_data_t {
    pl_options opts;    // the object queried
    pl_opt opt;         // the option this is the value of

    // the option's bytes inside `opts`. PL_OPT_BOOL / _INT / _FLOAT options that are plain
    // fields are a bool / int / float; for every other kind the representation is private.
    const void *value;

    // the value as locale-independent text, the form pl_options_set_str takes. Inside an
    // iteration callback: valid until the callback returns.
    const char *text;
} *pl_opt_data;

// The value of one option, or NULL (with an error logged) for an unknown key or a preset.
// Valid until the next pl_options_* call on `opts`.
PL_API pl_opt_data pl_options_get(pl_options opts, const char *key);

// Set one option from text, parsed according to the option's kind. Returns success; `opts` is
// unchanged on failure.
PL_API bool pl_options_set_str(pl_options opts, const char *key, const char *value);

// Call `cb` for every option (presets excepted) whose value differs from the empty
// configuration, in list order.
PL_API void pl_options_iterate(pl_options opts,
                               void (*cb)(void *priv, pl_opt_data data),
                               void *priv);

// The same walk as "key=value,key=value" text ("" for the empty configuration). The string
// belongs to `opts`: valid until the next pl_options_save or pl_options_free.
PL_API const char *pl_options_save(pl_options opts);

// Apply "key=value" entries separated by commas, semicolons, colons or whitespace; a key on its
// own switches a boolean on. Returns true if every entry was accepted; the entries after a
// rejected one are applied all the same.
PL_API bool pl_options_load(pl_options opts, const char *str);

// `opts->params.hooks` as an array `opts` owns (an array set by the caller is copied on the first
// call). A negative index counts from the end: -1 inserts after / removes the last hook.
// Hooks are not part of pl_options_save.
PL_API void pl_options_add_hook(pl_options opts, const struct pl_hook *hook);
PL_API void pl_options_insert_hook(pl_options opts, const struct pl_hook *hook, int idx);
PL_API void pl_options_remove_hook_at(pl_options opts, int idx);

// The option list. It leaves out what text cannot express: `info_callback`, `lut`, `hooks`.
enum pl_option_type {
    PL_OPT_BOOL,    // yes/no, on/off, true/false, ...
    PL_OPT_INT,     // decimal integer
    PL_OPT_FLOAT,   // decimal number, scientific notation or a fraction a/b; "C" locale
    PL_OPT_STRING,  // a name out of letters, digits, '_' and '-': enums, presets, filters and
                    // functions. Says how the text looks, not how the value is stored.
    PL_OPT_TYPE_COUNT,
};

struct pl_opt_t {
    const char *key;    // what pl_options_set_str / _load / _get take
    const char *name;   // for people
    enum pl_option_type type;
    float min, max;     // range of an int / float option; min == max == 0: unlimited
    bool deprecated;    // still accepted, with a warning
    bool preset;        // write-only: sets other options, which are what gets saved
    const void *priv;
};

PL_API extern const struct pl_opt_t pl_option_list[];   // ends with a {0} entry
PL_API extern const int pl_option_count;                // without that entry
PL_API pl_opt pl_find_option(const char *key);          // NULL if there is none

PL_API_END

#endif // LIBPLACEBO_OPTIONS_H_
