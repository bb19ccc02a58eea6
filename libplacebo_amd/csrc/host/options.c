/*
 * libplacebo-hip: pl_options, the option-string front end of pl_render_params
 * (include/libplacebo/options.h; role of the reference's src/options.c, whose keys, ranges,
 * flags and order are API and are pinned by tests/golden/options_list.json).
 *
 * One table (options_table.inc, generated): every option is a row giving its key, its kind and
 * where in struct pl_options_t its value lives. A kind is a (parse, print) pair further down; nothing
 * else in this file knows about individual options. Parsers write only on success, so a
 * rejected entry leaves the object as it was.
 */
#include <errno.h>
#include <limits.h>
#include <locale.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <libplacebo/options.h>

#include "host_common.h"

/* ---- the object ------------------------------------------------------------------------ */

struct options {
    struct pl_options_t pub;        // first: a pl_options points here
    pl_log log;
    const struct pl_hook **hooks;   // behind params.hooks once a hook helper ran
    int num_hooks, cap_hooks;
    char *saved;                    // pl_options_save
    size_t saved_cap;
    char text[64];                  // `text` of ...
    struct pl_opt_data_t data;      // ... what pl_options_get / _iterate hand out
};

#define OFF(field)  offsetof(struct pl_options_t, field)
#define SIZE(field) sizeof(((struct pl_options_t *) 0)->field)

#pragma GCC diagnostic ignored "-Wdeprecated-declarations"  // icc_params

// The eleven params structs: the pointer in `params`, the member of the same name it may point
// to, and the exported object that member starts out as (none: zeroes).
static const struct { size_t ptr, store, size; const void *init; } STRUCTS[] = {
#define S(f, init) { OFF(params.f), OFF(f), SIZE(f), init }
    S(deband_params,      &pl_deband_default_params),
    S(sigmoid_params,     &pl_sigmoid_default_params),
    S(color_adjustment,   &pl_color_adjustment_neutral),
    S(peak_detect_params, &pl_peak_detect_default_params),
    S(color_map_params,   &pl_color_map_default_params),
    S(dither_params,      &pl_dither_default_params),
    S(icc_params,         &pl_icc_default_params),
    S(cone_params,        &pl_vision_normal),
    S(blend_params,       NULL),
    S(deinterlace_params, &pl_deinterlace_default_params),
    S(distort_params,     &pl_distort_default_params),
#undef S
};

// The five scalers: the pointer in `params` and the custom slot of the same name, with what
// identifies the slot whatever filter is put into it
static const struct { size_t ptr, slot; const char *description; enum pl_filter_usage usage; } SCALERS[] = {
#define S(f, desc, usage) { OFF(params.f), OFF(f), desc, usage }
    S(upscaler,         "Custom upscaler",         PL_FILTER_UPSCALING),
    S(downscaler,       "Custom downscaler",       PL_FILTER_DOWNSCALING),
    S(plane_upscaler,   "Custom plane upscaler",   PL_FILTER_UPSCALING),
    S(plane_downscaler, "Custom plane downscaler", PL_FILTER_DOWNSCALING),
    S(frame_mixer,      "Custom frame mixer",      PL_FILTER_FRAME_MIXING),
#undef S
};

// The members of pl_render_params no option reaches: a preset loaded by name leaves them alone
static const struct { size_t offset, size; } UNREACHED[] = {
#define M(f) { offsetof(struct pl_render_params, f), sizeof(((struct pl_render_params *) 0)->f) }
    M(hooks), M(num_hooks), M(lut), M(info_callback), M(info_priv),
#undef M
};

static inline void *at(const struct pl_options_t *opts, size_t offset)
{
    return (char *) opts + offset;
}

// the empty configuration: pl_render_fast_params, every struct at its library default, empty slots.
// Its pointers point at the exported objects; only whether they are set is ever looked at.
static struct pl_options_t empty;
static pthread_once_t empty_once = PTHREAD_ONCE_INIT;

static void empty_init(void)
{
    memcpy(&empty.params, &pl_render_fast_params, sizeof(empty.params));
    for (size_t i = 0; i < PL_ARRAY_SIZE(STRUCTS); i++) {
        if (STRUCTS[i].init)
            memcpy(at(&empty, STRUCTS[i].store), STRUCTS[i].init, STRUCTS[i].size);
    }
    for (size_t i = 0; i < PL_ARRAY_SIZE(SCALERS); i++) {
        struct pl_filter_config *slot = at(&empty, SCALERS[i].slot);
        slot->name = "custom";
        slot->description = SCALERS[i].description;
        slot->allowed = SCALERS[i].usage;
    }
}

static const struct pl_options_t *defaults(void)
{
    pthread_once(&empty_once, empty_init);
    return &empty;
}

// copy what each non-NULL params pointer points at into `opts` and point it there
static void adopt_structs(pl_options opts)
{
    for (size_t i = 0; i < PL_ARRAY_SIZE(STRUCTS); i++) {
        const void **ptr = at(opts, STRUCTS[i].ptr);
        void *store = at(opts, STRUCTS[i].store);
        if (*ptr && *ptr != store)
            memcpy(store, *ptr, STRUCTS[i].size);
        if (*ptr)
            *ptr = store;
    }
}

// put a filter into a custom slot: everything it is made of (antiring included), while the slot
// stays the slot: its name, description and usages are not the filter's
static void fill_slot(struct pl_filter_config *slot, const struct pl_filter_config *filter)
{
    const struct pl_filter_config id = *slot;
    memcpy(slot, filter, sizeof(*slot));
    slot->name = id.name;
    slot->description = id.description;
    slot->allowed = id.allowed;
    slot->recommended = id.recommended;
}

static bool is_builtin_filter(const struct pl_filter_config *f)
{
    for (int i = 0; i < pl_num_filter_configs; i++) {
        if (pl_filter_configs[i] == f)
            return true;
    }
    return false;
}

void pl_options_reset(pl_options opts, const struct pl_render_params *preset)
{
    // built aside: the preset may be this object's own params and point into it
    struct pl_options_t next;
    memcpy(&next, defaults(), sizeof(next));
    if (preset)
        memcpy(&next.params, preset, sizeof(next.params));

    for (size_t i = 0; i < PL_ARRAY_SIZE(STRUCTS); i++) {
        const void **ptr = at(&next, STRUCTS[i].ptr);
        if (*ptr) {
            memcpy(at(&next, STRUCTS[i].store), *ptr, STRUCTS[i].size);
            *ptr = at(opts, STRUCTS[i].store);
        }
    }
    for (size_t i = 0; i < PL_ARRAY_SIZE(SCALERS); i++) {
        const struct pl_filter_config **ptr = at(&next, SCALERS[i].ptr);
        if (*ptr && !is_builtin_filter(*ptr)) {
            fill_slot(at(&next, SCALERS[i].slot), *ptr);
            *ptr = at(opts, SCALERS[i].slot);
        }
    }
    memcpy(opts, &next, sizeof(next));
}

pl_options pl_options_alloc(pl_log log)
{
    struct options *p = calloc(1, sizeof(*p));
    if (!p)
        return NULL;
    p->log = log;
    pl_options_reset(&p->pub, NULL);
    return &p->pub;
}

void pl_options_free(pl_options *popts)
{
    if (!popts || !*popts)
        return;
    struct options *p = (struct options *) *popts;
    free(p->saved);
    free(p->hooks);
    free(p);
    *popts = NULL;
}

/* ---- hooks ----------------------------------------------------------------------------- */

// make params.hooks the array this object owns, with room for one more
static bool own_hooks(struct options *p)
{
    struct pl_render_params *params = &p->pub.params;
    const int num = params->hooks ? PL_MAX(params->num_hooks, 0) : 0;
    const bool foreign = params->hooks != (const struct pl_hook *const *) p->hooks;
    if (num + 1 > p->cap_hooks) {
        const int cap = PL_MAX(2 * p->cap_hooks, num + 4);
        const struct pl_hook **arr = malloc(cap * sizeof(*arr));
        if (!arr) {
            pl_msg(p->log, PL_LOG_ERR, "pl_options: out of memory for %d hooks", cap);
            return false;
        }
        if (num)
            memcpy(arr, params->hooks, num * sizeof(*arr));
        free(p->hooks);
        p->hooks = arr;
        p->cap_hooks = cap;
    } else if (foreign && num) {
        memmove(p->hooks, params->hooks, num * sizeof(*p->hooks));
    }
    p->num_hooks = num;
    params->hooks = (const struct pl_hook *const *) p->hooks;
    params->num_hooks = num;
    return true;
}

void pl_options_insert_hook(pl_options opts, const struct pl_hook *hook, int idx)
{
    struct options *p = (struct options *) opts;
    if (!own_hooks(p))
        return;
    if (idx < 0)
        idx += p->num_hooks + 1;
    if (idx < 0 || idx > p->num_hooks) {
        pl_msg(p->log, PL_LOG_ERR, "pl_options_insert_hook: no position %d among %d hooks",
               idx, p->num_hooks);
        return;
    }
    memmove(&p->hooks[idx + 1], &p->hooks[idx], (p->num_hooks - idx) * sizeof(*p->hooks));
    p->hooks[idx] = hook;
    opts->params.num_hooks = ++p->num_hooks;
}

void pl_options_add_hook(pl_options opts, const struct pl_hook *hook)
{
    pl_options_insert_hook(opts, hook, -1);
}

void pl_options_remove_hook_at(pl_options opts, int idx)
{
    struct options *p = (struct options *) opts;
    if (!own_hooks(p))
        return;
    if (idx < 0)
        idx += p->num_hooks;
    if (idx < 0 || idx >= p->num_hooks) {
        pl_msg(p->log, PL_LOG_ERR, "pl_options_remove_hook_at: no hook %d among %d",
               idx, p->num_hooks);
        return;
    }
    memmove(&p->hooks[idx], &p->hooks[idx + 1], (p->num_hooks - idx - 1) * sizeof(*p->hooks));
    opts->params.num_hooks = --p->num_hooks;
}

/* ---- kinds of option --------------------------------------------------------------------- */

enum opt_kind {
    KIND_BOOL,          // bool field
    KIND_INT,           // int field
    KIND_FLOAT,         // float field
    KIND_ENUM,          // unsigned field, one of `choices` (name, value)
    KIND_TOGGLE,        // params pointer: NULL or the struct at `target`
    KIND_NAMED,         // pointer to an entry of `table`, or NULL ("none")
    KIND_SCALER,        // params scaler pointer: a built-in config, the slot at `target`, NULL
    KIND_PRESET,        // write-only: copies one of `choices` (name, struct) over a params struct
    KIND_PRESET_ALL,    // write-only: the global preset
    KIND_PRESET_SCALER, // write-only: copies a built-in config into a custom slot
    KIND_COUNT,
};

struct choice {
    const char *name;
    unsigned value;     // KIND_ENUM
    const void *preset; // KIND_PRESET*
};

// every table of named objects the library exports is a NULL-terminated array of pointers to
// structs that begin with their name
#define TABLE(arr) ((const void *const *) (arr))
_Static_assert(offsetof(struct pl_filter_function, name) == 0, "name first");
_Static_assert(offsetof(struct pl_filter_config, name) == 0, "name first");
_Static_assert(offsetof(struct pl_tone_map_function, name) == 0, "name first");
_Static_assert(offsetof(struct pl_gamut_map_function, name) == 0, "name first");
_Static_assert(offsetof(struct pl_error_diffusion_kernel, name) == 0, "name first");

static const char *name_of(const void *obj)
{
    return *(const char *const *) obj;
}

struct opt_info {
    enum opt_kind kind;
    size_t offset, size;            // the value: what is compared, printed and written
    size_t target;                  // KIND_TOGGLE, KIND_SCALER
    const struct choice *choices;   // ends with a {0} entry
    const void *const *table;
    enum pl_filter_usage usage;     // KIND_SCALER, KIND_PRESET_SCALER
};

struct opt_ctx {
    pl_options opts;
    pl_log log;
    pl_opt opt;
    const struct opt_info *info;
};

#define REJECT(ctx, ...) (pl_msg((ctx)->log, PL_LOG_ERR, __VA_ARGS__), false)

/* numbers: always the "C" locale, whatever the application has set. Where no "C" locale object
 * can be made, the application's decimal point is exchanged for '.' around the conversion. */

static locale_t c_locale_obj;
static pthread_once_t c_locale_once = PTHREAD_ONCE_INIT;

static void c_locale_init(void)
{
    c_locale_obj = newlocale(LC_ALL_MASK, "C", (locale_t) 0);
}

static locale_t c_locale(void)
{
    pthread_once(&c_locale_once, c_locale_init);
    return c_locale_obj;
}

// the application's decimal point, if it is a single character other than '.'; else 0
static char foreign_point(void)
{
    const char *point = localeconv()->decimal_point;
    return point && point[0] != '.' && point[0] && !point[1] ? point[0] : 0;
}

static void exchange(char *s, char from, char to)
{
    for (; *s; s++) {
        if (*s == from)
            *s = to;
    }
}

static bool only_chars(const char *s, const char *allowed)
{
    return *s && strspn(s, allowed) == strlen(s);
}

// `s` holds digits, signs, '.', 'e' only: what is left of the locale is the decimal point
static double read_double(const char *s, char **end)
{
    locale_t loc = c_locale();
    if (loc)
        return strtod_l(s, end, loc);
    char tmp[64];
    snprintf(tmp, sizeof(tmp), "%s", s);
    if (foreign_point())
        exchange(tmp, '.', foreign_point());
    char *tmp_end;
    const double v = strtod(tmp, &tmp_end);
    *end = (char *) s + (tmp_end - tmp);
    return v;
}

static bool parse_number(const char *s, double *out)
{
    if (!only_chars(s, "0123456789+-.eE") || strlen(s) >= 64)
        return false;
    char *end;
    *out = read_double(s, &end);
    return end != s && !*end;
}

// a word strtod would take as a non-finite value
static bool is_nonfinite_word(const char *s)
{
    if (*s == '+' || *s == '-')
        s++;
    return !strcasecmp(s, "nan") || !strcasecmp(s, "inf") || !strcasecmp(s, "infinity");
}

// the fewest digits that read back as the same value: written out plainly (1000, 0.001) where
// the exponent is small, as d.ddde+xx beyond that
static void print_number(char *buf, size_t len, double v)
{
    locale_t loc = c_locale(), old = loc ? uselocale(loc) : (locale_t) 0;
    const char point = loc ? 0 : foreign_point();
    for (int digits = 1; digits <= 17; digits++) {
        char *end;
        snprintf(buf, len, "%.*e", digits - 1, v);
        if (point)
            exchange(buf, point, '.');
        if (read_double(buf, &end) != v && digits < 17)
            continue;
        const int exponent = atoi(strchr(buf, 'e') + 1);
        if (exponent >= -4 && exponent < 16) {
            snprintf(buf, len, "%.*f", PL_MAX(digits - 1 - exponent, 0), v);
            if (point)
                exchange(buf, point, '.');
        }
        break;
    }
    if (loc)
        uselocale(old);
}

static const char *const WORDS_TRUE[]  = { "yes", "y", "on", "true", "enabled", "" };
static const char *const WORDS_FALSE[] = { "no", "n", "off", "false", "disabled" };

static bool read_bool(const struct opt_ctx *ctx, const char *str, bool *out)
{
    for (size_t i = 0; i < PL_ARRAY_SIZE(WORDS_TRUE); i++) {
        if (!strcmp(str, WORDS_TRUE[i])) {
            *out = true;
            return true;
        }
    }
    for (size_t i = 0; i < PL_ARRAY_SIZE(WORDS_FALSE); i++) {
        if (!strcmp(str, WORDS_FALSE[i])) {
            *out = false;
            return true;
        }
    }
    return REJECT(ctx, "option '%s': '%s' is not a boolean (yes / no)", ctx->opt->key, str);
}

static bool parse_bool(const struct opt_ctx *ctx, const char *str, void *val)
{
    return read_bool(ctx, str, val);
}

static void print_bool(const struct opt_ctx *ctx, const void *val, char *buf, size_t len)
{
    snprintf(buf, len, "%s", *(const bool *) val ? "yes" : "no");
}

static bool in_range(pl_opt opt, double v)
{
    return opt->min == opt->max || (v >= opt->min && v <= opt->max);
}

static bool parse_int(const struct opt_ctx *ctx, const char *str, void *val)
{
    pl_opt opt = ctx->opt;
    char *end;
    errno = 0;
    const long v = only_chars(str, "0123456789+-") ? strtol(str, &end, 10) : 0;
    if (!only_chars(str, "0123456789+-") || end == str || *end || errno || v < INT_MIN || v > INT_MAX)
        return REJECT(ctx, "option '%s': '%s' is not an integer", opt->key, str);
    if (!in_range(opt, v)) {
        return REJECT(ctx, "option '%s': %ld is outside [%d, %d]", opt->key, v,
                      (int) opt->min, (int) opt->max);
    }
    *(int *) val = v;
    return true;
}

static void print_int(const struct opt_ctx *ctx, const void *val, char *buf, size_t len)
{
    snprintf(buf, len, "%d", *(const int *) val);
}

static bool parse_float(const struct opt_ctx *ctx, const char *str, void *val)
{
    pl_opt opt = ctx->opt;
    char num[64];
    double n = 0.0, d = 1.0;
    float v;
    const char *slash = strchr(str, '/');
    bool ok;
    if (is_nonfinite_word(str)) {
        ok = true;
        v = NAN;
    } else if (slash && (size_t) (slash - str) < sizeof(num)) {
        memcpy(num, str, slash - str);
        num[slash - str] = 0;
        ok = parse_number(num, &n) && parse_number(slash + 1, &d);
        v = (float) n / (float) d;
    } else {
        ok = parse_number(str, &n);
        v = n;
    }
    if (!ok)
        return REJECT(ctx, "option '%s': '%s' is not a number or a fraction", opt->key, str);

    const int cls = fpclassify(v);
    if (cls != FP_ZERO && cls != FP_NORMAL) {
        return REJECT(ctx, "option '%s': '%s' is not a finite, normal number", opt->key, str);
    }
    if (!in_range(opt, v)) {
        return REJECT(ctx, "option '%s': %g is outside [%g, %g]", opt->key, v, opt->min, opt->max);
    }
    *(float *) val = v;
    return true;
}

static void print_float(const struct opt_ctx *ctx, const void *val, char *buf, size_t len)
{
    print_number(buf, len, *(const float *) val);
}

// "a, b, c" of the names an option takes, for the one error message a bad name gets
static void list_names(char *buf, size_t len, const char *first, const char *second,
                       const struct choice *choices, const void *const *table,
                       enum pl_filter_usage usage)
{
    size_t pos = 0;
    buf[0] = 0;
#define ADD(name) do {                                                          \
        if (pos < len)                                                          \
            pos += snprintf(buf + pos, len - pos, "%s%s", pos ? ", " : "", name); \
    } while (0)
    if (first)
        ADD(first);
    if (second)
        ADD(second);
    for (int i = 0; choices && choices[i].name; i++)
        ADD(choices[i].name);
    for (int i = 0; table && table[i]; i++)
        ADD(name_of(table[i]));
    for (int i = 0; usage && i < pl_num_filter_configs; i++) {
        if (pl_filter_configs[i]->allowed & usage)
            ADD(pl_filter_configs[i]->name);
    }
#undef ADD
}

static bool reject_name(const struct opt_ctx *ctx, const char *str, const char *first,
                        const char *second)
{
    char names[768];
    list_names(names, sizeof(names), first, second, ctx->info->choices, ctx->info->table,
               ctx->info->usage);
    return REJECT(ctx, "option '%s': unknown value '%s'; one of: %s", ctx->opt->key, str, names);
}

static const struct choice *find_choice(const struct opt_ctx *ctx, const char *str)
{
    for (const struct choice *c = ctx->info->choices; c->name; c++) {
        if (!strcmp(str, c->name))
            return c;
    }
    return NULL;
}

static const struct pl_filter_config *find_filter(const struct opt_ctx *ctx, const char *str)
{
    for (int i = 0; i < pl_num_filter_configs; i++) {
        const struct pl_filter_config *f = pl_filter_configs[i];
        if ((f->allowed & ctx->info->usage) && !strcmp(str, f->name))
            return f;
    }
    return NULL;
}

static bool parse_enum(const struct opt_ctx *ctx, const char *str, void *val)
{
    const struct choice *c = find_choice(ctx, str);
    if (!c)
        return reject_name(ctx, str, NULL, NULL);
    *(unsigned *) val = c->value;
    return true;
}

static void print_enum(const struct opt_ctx *ctx, const void *val, char *buf, size_t len)
{
    // a value no name stands for can only have been written past this interface
    snprintf(buf, len, "%u", *(const unsigned *) val);
    for (const struct choice *c = ctx->info->choices; c->name; c++) {
        if (c->value == *(const unsigned *) val) {
            snprintf(buf, len, "%s", c->name);
            return;
        }
    }
}

static bool parse_toggle(const struct opt_ctx *ctx, const char *str, void *val)
{
    bool on;
    if (!read_bool(ctx, str, &on))
        return false;
    *(const void **) val = on ? at(ctx->opts, ctx->info->target) : NULL;
    return true;
}

static void print_toggle(const struct opt_ctx *ctx, const void *val, char *buf, size_t len)
{
    snprintf(buf, len, "%s", *(const void *const *) val ? "yes" : "no");
}

static bool parse_named(const struct opt_ctx *ctx, const char *str, void *val)
{
    const void *found = NULL;
    for (int i = 0; !found && ctx->info->table[i]; i++) {
        if (!strcmp(str, name_of(ctx->info->table[i])))
            found = ctx->info->table[i];
    }
    if (!found && strcmp(str, "none"))
        return reject_name(ctx, str, "none", NULL);
    *(const void **) val = found;
    return true;
}

static void print_named(const struct opt_ctx *ctx, const void *val, char *buf, size_t len)
{
    const void *obj = *(const void *const *) val;
    snprintf(buf, len, "%s", obj ? name_of(obj) : "none");
}

static bool parse_scaler(const struct opt_ctx *ctx, const char *str, void *val)
{
    const struct pl_filter_config *f = NULL;
    if (!strcmp(str, "custom")) {
        f = at(ctx->opts, ctx->info->target);
    } else if (strcmp(str, "none") && !(f = find_filter(ctx, str))) {
        return reject_name(ctx, str, "none", "custom");
    }
    *(const struct pl_filter_config **) val = f;
    return true;
}

static bool parse_preset(const struct opt_ctx *ctx, const char *str, void *val)
{
    const struct choice *c = find_choice(ctx, str);
    if (!c)
        return reject_name(ctx, str, NULL, NULL);
    memcpy(val, c->preset, ctx->info->size);
    return true;
}

// the whole of pl_render_params, bar the members no option reaches; params structs the preset
// does not use keep their values
static bool parse_preset_all(const struct opt_ctx *ctx, const char *str, void *val)
{
    const struct choice *c = find_choice(ctx, str);
    if (!c)
        return reject_name(ctx, str, NULL, NULL);
    struct pl_render_params next;
    memcpy(&next, c->preset, sizeof(next));
    for (size_t i = 0; i < PL_ARRAY_SIZE(UNREACHED); i++) {
        memcpy((char *) &next + UNREACHED[i].offset, (const char *) val + UNREACHED[i].offset,
               UNREACHED[i].size);
    }
    memcpy(val, &next, sizeof(next));
    adopt_structs(ctx->opts);
    return true;
}

static bool parse_preset_scaler(const struct opt_ctx *ctx, const char *str, void *val)
{
    const struct pl_filter_config *f = find_filter(ctx, str);
    if (f) {
        fill_slot(val, f);
    } else if (!strcmp(str, "none")) {
        memcpy(val, at(defaults(), ctx->info->offset), sizeof(*f));
    } else {
        return reject_name(ctx, str, "none", NULL);
    }
    return true;
}

static const struct {
    bool (*parse)(const struct opt_ctx *ctx, const char *str, void *val);
    void (*print)(const struct opt_ctx *ctx, const void *val, char *buf, size_t len);
} KINDS[KIND_COUNT] = {
    [KIND_BOOL]          = { parse_bool,          print_bool },
    [KIND_INT]           = { parse_int,           print_int },
    [KIND_FLOAT]         = { parse_float,         print_float },
    [KIND_ENUM]          = { parse_enum,          print_enum },
    [KIND_TOGGLE]        = { parse_toggle,        print_toggle },
    [KIND_NAMED]         = { parse_named,         print_named },
    [KIND_SCALER]        = { parse_scaler,        print_named }, // (a config begins with its name)
    [KIND_PRESET]        = { parse_preset,        NULL },
    [KIND_PRESET_ALL]    = { parse_preset_all,    NULL },
    [KIND_PRESET_SCALER] = { parse_preset_scaler, NULL },
};

/* ---- the list ---------------------------------------------------------------------------- */

// Rows of plain data, written by tools/gen_options_table.py: what is API about an option (key,
// type, range, flags, position, value names) from tests/golden/options_list.json, where its value
// lives from the generator's own statement of which member each key stands for.
#include "options_table.inc"

const int pl_option_count = PL_ARRAY_SIZE(pl_option_list) - 1;

pl_opt pl_find_option(const char *key)
{
    for (int i = 0; key && i < pl_option_count; i++) {
        if (!strcmp(key, pl_option_list[i].key))
            return &pl_option_list[i];
    }
    return NULL;
}

/* ---- get / iterate / save ---------------------------------------------------------------- */

static pl_opt_data describe(struct options *p, pl_opt opt)
{
    const struct opt_info *info = opt->priv;
    const struct opt_ctx ctx = { &p->pub, p->log, opt, info };
    const void *val = at(&p->pub, info->offset);
    KINDS[info->kind].print(&ctx, val, p->text, sizeof(p->text));
    p->data = (struct pl_opt_data_t) { &p->pub, opt, val, p->text };
    return &p->data;
}

pl_opt_data pl_options_get(pl_options opts, const char *key)
{
    struct options *p = (struct options *) opts;
    pl_opt opt = pl_find_option(key);
    if (!opt || opt->preset) {
        pl_msg(p->log, PL_LOG_ERR, "pl_options_get: '%s' is %s", key ? key : "(null)",
               opt ? "a preset and has no value" : "not an option");
        return NULL;
    }
    return describe(p, opt);
}

static bool is_default(pl_options opts, const struct opt_info *info)
{
    const void *val = at(opts, info->offset);
    const void *ref = at(defaults(), info->offset);
    if (info->kind == KIND_TOGGLE)
        return !*(const void *const *) val == !*(const void *const *) ref;
    return !memcmp(val, ref, info->size);
}

void pl_options_iterate(pl_options opts, void (*cb)(void *priv, pl_opt_data data), void *priv)
{
    for (pl_opt opt = pl_option_list; opt->key; opt++) {
        if (!opt->preset && !is_default(opts, opt->priv))
            cb(priv, describe((struct options *) opts, opt));
    }
}

struct save_state {
    struct options *p;
    size_t len;
    bool failed;
};

static void save_one(void *priv, pl_opt_data data)
{
    struct save_state *s = priv;
    struct options *p = s->p;
    const size_t need = s->len + strlen(data->opt->key) + strlen(data->text) + 3;
    if (need > p->saved_cap) {
        char *buf = realloc(p->saved, 2 * need);
        if (!buf) {
            s->failed = true;
            return;
        }
        p->saved = buf;
        p->saved_cap = 2 * need;
    }
    s->len += sprintf(p->saved + s->len, "%s%s=%s", s->len ? "," : "", data->opt->key, data->text);
}

const char *pl_options_save(pl_options opts)
{
    struct save_state s = { (struct options *) opts };
    pl_options_iterate(opts, save_one, &s);
    if (s.failed)
        pl_msg(s.p->log, PL_LOG_ERR, "pl_options_save: out of memory, the string is incomplete");
    return s.len ? s.p->saved : "";
}

/* ---- set / load -------------------------------------------------------------------------- */

static const char SPACE[] = " \t\r\n\f\v";

// key and value as counted strings, not yet stripped
static bool set_raw(struct options *p, const char *key, size_t klen, const char *val, size_t vlen)
{
    while (klen && strchr(SPACE, key[0]))
        key++, klen--;
    while (klen && strchr(SPACE, key[klen - 1]))
        klen--;
    while (vlen && strchr(SPACE, val[0]))
        val++, vlen--;
    while (vlen && strchr(SPACE, val[vlen - 1]))
        vlen--;

    char kbuf[64], vbuf[128];
    if (klen >= sizeof(kbuf) || vlen >= sizeof(vbuf) || memchr(key, 0, klen) || memchr(val, 0, vlen)) {
        pl_msg(p->log, PL_LOG_ERR, "option '%.*s=%.*s' is too long to be one",
               (int) PL_MIN(klen, 40), key, (int) PL_MIN(vlen, 40), val);
        return false;
    }
    memcpy(kbuf, key, klen);
    memcpy(vbuf, val, vlen);
    kbuf[klen] = vbuf[vlen] = 0;

    pl_opt opt = pl_find_option(kbuf);
    if (!opt) {
        pl_msg(p->log, PL_LOG_ERR, "'%s' is not an option (in '%s=%s')", kbuf, kbuf, vbuf);
        return false;
    }
    pl_msg(p->log, PL_LOG_TRACE, "option '%s' = '%s'", opt->key, vbuf);
    if (opt->deprecated)
        pl_msg(p->log, PL_LOG_WARN, "option '%s' is deprecated", opt->key);

    const struct opt_info *info = opt->priv;
    const struct opt_ctx ctx = { &p->pub, p->log, opt, info };
    return KINDS[info->kind].parse(&ctx, vbuf, at(&p->pub, info->offset));
}

bool pl_options_set_str(pl_options opts, const char *key, const char *value)
{
    key = PL_DEF(key, "");
    value = PL_DEF(value, "");
    return set_raw((struct options *) opts, key, strlen(key), value, strlen(value));
}

bool pl_options_load(pl_options opts, const char *str)
{
    bool ok = true;
    for (str = PL_DEF(str, ""); *str; ) {
        const size_t len = strcspn(str, " ,;:\n");
        const char *eq = memchr(str, '=', len);
        // (an entry of nothing but blanks is no entry)
        size_t blank = 0;
        while (blank < len && strchr(SPACE, str[blank]))
            blank++;
        if (blank < len) {
            ok &= eq ? set_raw((struct options *) opts, str, eq - str, eq + 1, len - (eq + 1 - str))
                     : set_raw((struct options *) opts, str, len, "", 0);
        }
        str += len + (str[len] ? 1 : 0);
    }
    return ok;
}
