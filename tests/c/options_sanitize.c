/*
 * pl_options under AddressSanitizer / UBSan: a program of its own, built and run by `make -f
 * tests/c/options_sanitize.mk` from this file, csrc/host/options.c and the pure host files it walks tables of, all
 * compiled with -fsanitize=address,undefined (the preset structs come from libplacebo_hip.so).
 * CPU only; not built by build().
 *
 * It knows no option by name: the list tells it each option's type and range, and a pool of
 * words (the names the library exports, plus the enum and preset names) is offered to every
 * string option. Whatever is accepted must survive save -> reset -> load byte for byte; whatever
 * is malformed must be refused with one error and without a change.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <libplacebo/options.h>

static int failures, errors_logged;

#define CHECK(cond, ...) do {                                       \
        if (!(cond)) {                                              \
            failures++;                                             \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                                    \
            printf("\n");                                           \
        }                                                           \
    } while (0)

static void on_log(void *priv, enum pl_log_level level, const char *msg)
{
    if (level <= PL_LOG_ERR)
        errors_logged++;
}

static const char *const WORDS[] = {
    "none", "custom", "any", "hdr10", "hdr10plus", "cie_y", "blue", "ordered_lut", "ordered", "white",
    "auto", "perceptual", "relative", "saturation", "absolute", "l", "m", "s", "lm", "ms", "ls", "lms",
    "zero", "one", "alpha", "one_minus_alpha", "weave", "bob", "yadif", "bwdif", "clamp", "repeat",
    "mirror", "unknown", "independent", "premultiplied", "native", "normalized", "conversion",
    "color", "tiles", "skip", "blur", "default", "fast", "high_quality", "neutral", "normal",
    "protanomaly", "protanopia", "deuteranomaly", "deuteranopia", "tritanomaly", "tritanopia",
    "monochromacy", "achromatopsia", "alpha_overlay",
};

static const char *pool[512];
static int num_pool;

static void fill_pool(void)
{
    for (size_t i = 0; i < sizeof(WORDS) / sizeof(WORDS[0]); i++)
        pool[num_pool++] = WORDS[i];
    for (int i = 0; i < pl_num_filter_configs; i++)
        pool[num_pool++] = pl_filter_configs[i]->name;
    for (int i = 0; pl_filter_functions[i]; i++)
        pool[num_pool++] = pl_filter_functions[i]->name;
    for (int i = 0; pl_tone_map_functions[i]; i++)
        pool[num_pool++] = pl_tone_map_functions[i]->name;
    for (int i = 0; pl_gamut_map_functions[i]; i++)
        pool[num_pool++] = pl_gamut_map_functions[i]->name;
    for (int i = 0; pl_error_diffusion_kernels[i]; i++)
        pool[num_pool++] = pl_error_diffusion_kernels[i]->name;
}

// set `key` to `text` in an empty configuration; the result must come back from its own string
static bool round_trip(pl_options opts, pl_log log, pl_opt opt, const char *text, bool must_take)
{
    char saved[4096];
    struct pl_options_t after;
    pl_options_reset(opts, NULL);
    pl_log_level_update(log, must_take ? PL_LOG_ERR : PL_LOG_NONE);
    const bool taken = pl_options_set_str(opts, opt->key, text);
    pl_log_level_update(log, PL_LOG_ERR);
    if (!taken) {
        CHECK(!must_take, "%s=%s", opt->key, text);
        return false;
    }
    if (!opt->preset) {
        pl_opt_data data = pl_options_get(opts, opt->key);
        CHECK(data && data->opt == opt && data->text, "%s", opt->key);
        CHECK(data && (const char *) data->value >= (const char *) opts &&
              (const char *) data->value < (const char *) (opts + 1), "%s", opt->key);
    }
    snprintf(saved, sizeof(saved), "%s", pl_options_save(opts));
    memcpy(&after, opts, sizeof(after));
    pl_options_reset(opts, NULL);
    CHECK(pl_options_load(opts, saved), "%s=%s -> %s", opt->key, text, saved);
    CHECK(!memcmp(opts, &after, sizeof(after)), "%s=%s -> %s", opt->key, text, saved);
    CHECK(!strcmp(pl_options_save(opts), saved), "%s=%s -> %s", opt->key, text, saved);
    return true;
}

static void sweep(pl_options opts, pl_log log)
{
    char text[64];
    for (pl_opt opt = pl_option_list; opt->key; opt++) {
        const bool ranged = opt->min != opt->max;
        int taken = 0;
        switch (opt->type) {
        case PL_OPT_BOOL:
            taken += round_trip(opts, log, opt, "yes", true);
            taken += round_trip(opts, log, opt, "no", true);
            taken += round_trip(opts, log, opt, "", true);
            break;
        case PL_OPT_INT: {
            const int vals[] = { ranged ? opt->min : -3, ranged ? opt->max : 7,
                                 ranged ? (opt->min + opt->max) / 2 : 1 << 20 };
            for (int i = 0; i < 3; i++) {
                snprintf(text, sizeof(text), "%d", vals[i]);
                taken += round_trip(opts, log, opt, text, true);
            }
            break;
        }
        case PL_OPT_FLOAT: {
            const float vals[] = { ranged ? opt->min : -2.5f, ranged ? opt->max : 1e-3f,
                                   ranged ? (opt->min + opt->max) / 2 : 123456.789f,
                                   ranged ? opt->min + (opt->max - opt->min) / 3 : 1e30f };
            for (int i = 0; i < 4; i++) {
                snprintf(text, sizeof(text), "%.9g", vals[i]);
                taken += round_trip(opts, log, opt, text, true);
            }
            const char *const fractions[] = { "1/3", "2/3", "7/3" };
            for (int i = 0; i < 3; i++)
                taken += round_trip(opts, log, opt, fractions[i], false);
            CHECK(taken >= 5, "%s takes no fraction", opt->key);
            break;
        }
        case PL_OPT_STRING:
            for (int i = 0; i < num_pool; i++)
                taken += round_trip(opts, log, opt, pool[i], false);
            break;
        case PL_OPT_TYPE_COUNT:
            break;
        }
        CHECK(taken >= (opt->preset ? 1 : 2), "%s took %d values", opt->key, taken);
    }
    CHECK(!errors_logged, "%d errors logged by legal values", errors_logged);
    errors_logged = 0;
}

static void refusals(pl_options opts)
{
    static const char *const bad[] = {
        "bogus=1", "deband_iterations=100", "lut_entries=-1", "brightness=2.0", "sigmoid_slope=0.5",
        "gamma=nan", "gamma=inf", "hue=-inf", "hue=1/0", "hue=1e-40", "hue=1e60", "hue=1e999",
        "dither_method=invalid", "tone_mapping=nope", "upscaler=nope", "preset=slow",
        "upscaler_preset=help", "tone_lut_size=abc", "tile_size=32x", "tile_size=99999999999999999999",
        "tile_size=32.0", "show_clipping=hello", "gamma=oops", "gamma=0x1p0", "gamma=1/", "gamma=/2",
        "tile_size", "=", "preset==bar", "invalid", "peak_percentile=E8203125", "deband=maybe",
        "upscaler=aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa"
        "aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa",
        "aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa=1",
    };
    struct pl_options_t before;
    pl_options_reset(opts, &pl_render_high_quality_params);
    CHECK(pl_options_load(opts, "upscaler=custom,upscaler_preset=mitchell,gamma=1.5"), "setup");
    memcpy(&before, opts, sizeof(before));
    for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); i++) {
        errors_logged = 0;
        CHECK(!pl_options_load(opts, bad[i]), "%s", bad[i]);
        CHECK(errors_logged == 1, "%s: %d errors", bad[i], errors_logged);
        CHECK(!memcmp(opts, &before, sizeof(before)), "%s changed the object", bad[i]);
    }
    errors_logged = 0;
    CHECK(!pl_options_get(opts, "preset") && !pl_options_get(opts, "bogus") &&
          !pl_options_get(opts, NULL), "get");
    CHECK(errors_logged == 3, "get: %d errors", errors_logged);
    errors_logged = 0;
    CHECK(!pl_options_load(opts, "deband=no,bogus=1,dither=no"), "mixed");
    CHECK(errors_logged == 1 && !opts->params.deband_params && !opts->params.dither_params, "mixed");
    CHECK(pl_options_load(opts, NULL) && !pl_options_set_str(opts, NULL, NULL), "NULL strings");
    errors_logged = 0;
}

static void hooks(pl_options opts)
{
    static const struct pl_hook some[40];
    const struct pl_hook *mine[2] = { &some[38], &some[39] };
    pl_options_reset(opts, NULL);
    opts->params.hooks = mine;
    opts->params.num_hooks = 2;
    for (int i = 0; i < 30; i++)                    // (grows the array several times)
        pl_options_insert_hook(opts, &some[i], i % 3 == 0 ? 0 : i % 3 == 1 ? -1 : i / 2);
    CHECK(opts->params.num_hooks == 32 && opts->params.hooks != mine, "%d", opts->params.num_hooks);
    CHECK(mine[0] == &some[38] && mine[1] == &some[39], "the caller's array was written to");
    CHECK(opts->params.hooks[0] == &some[27] && opts->params.hooks[31] == &some[28], "order");
    pl_options_add_hook(opts, &some[30]);
    CHECK(opts->params.hooks[32] == &some[30], "order");
    for (int i = 0; i < 33; i++)
        pl_options_remove_hook_at(opts, i % 2 ? -1 : 0);
    CHECK(opts->params.num_hooks == 0 && !errors_logged, "%d left", opts->params.num_hooks);
    pl_options_remove_hook_at(opts, -1);
    pl_options_insert_hook(opts, &some[0], 1);
    CHECK(errors_logged == 2 && opts->params.num_hooks == 0, "out-of-range positions");
    CHECK(!strcmp(pl_options_save(opts), ""), "hooks are not saved");
    errors_logged = 0;
}

static void count(void *priv, pl_opt_data data)
{
    CHECK(data->opts && data->opt && data->value && data->text[0], "iterate");
    ++*(int *) priv;
}

// one object holding a non-default value of every option, through one string
static void everything_at_once(pl_options opts, pl_log log)
{
    char was[64], text[64], saved[16384];
    struct pl_options_t after;
    int expected = 0, visited = 0;
    pl_options_reset(opts, NULL);
    pl_options fresh = pl_options_alloc(NULL);
    for (pl_opt opt = pl_option_list; opt->key; opt++) {
        if (opt->preset)
            continue;
        expected++;
        snprintf(was, sizeof(was), "%s", pl_options_get(fresh, opt->key)->text);
        const bool ranged = opt->min != opt->max;
        snprintf(text, sizeof(text), opt->type == PL_OPT_INT ? "%.0f" : "%.9g",
                 ranged ? opt->min + (opt->max - opt->min) * 0.3141 : 3.0);
        bool done = false;
        if (opt->type == PL_OPT_BOOL) {
            done = pl_options_set_str(opts, opt->key, strcmp(was, "yes") ? "yes" : "no");
        } else if (opt->type != PL_OPT_STRING) {
            done = pl_options_set_str(opts, opt->key, text);
        } else {
            pl_log_level_update(log, PL_LOG_NONE);
            for (int i = 0; i < num_pool && !done; i++)
                done = strcmp(pool[i], was) && pl_options_set_str(opts, opt->key, pool[i]);
            pl_log_level_update(log, PL_LOG_ERR);
        }
        CHECK(done, "%s", opt->key);
    }
    pl_options_free(&fresh);
    pl_options_iterate(opts, count, &visited);
    CHECK(visited == expected, "%d of %d options differ from their defaults", visited, expected);
    snprintf(saved, sizeof(saved), "%s", pl_options_save(opts));
    memcpy(&after, opts, sizeof(after));
    pl_options_reset(opts, NULL);
    CHECK(pl_options_load(opts, saved) && !memcmp(opts, &after, sizeof(after)), "%s", saved);
    CHECK(!errors_logged, "%d errors", errors_logged);
    errors_logged = 0;
}

int main(void)
{
    pl_log log = pl_log_create(PL_API_VER, &(struct pl_log_params) { on_log, NULL, PL_LOG_ERR });
    pl_options opts = pl_options_alloc(log);
    CHECK(pl_option_list[pl_option_count].key == NULL && pl_option_count > 200, "list");
    fill_pool();
    sweep(opts, log);
    refusals(opts);
    hooks(opts);

    everything_at_once(opts, log);

    pl_options_free(&opts);
    pl_options_free(&opts);
    pl_options_free(NULL);
    pl_log_destroy(&log);
    printf("options_sanitize: %d failures\n", failures);
    return failures ? 1 : 0;
}
