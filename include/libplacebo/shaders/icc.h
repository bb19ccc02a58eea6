/*
 * libplacebo-hip: ICC colour management (the reference's src/include/libplacebo/shaders/icc.h).
 * Profiles are interpreted by LittleCMS 2, which is loaded at run time (liblcms2.so.2) on the
 * first pl_icc_open: no header and no link-time dependency. Where it cannot be loaded the
 * entry points behave like the reference's compiled without PL_HAVE_LCMS (pl_icc_open fails
 * and says why), and a frame carrying an `icc` object or a `profile` is rendered from its
 * pl_color_space alone, with a warning logged once.
 */
#ifndef LIBPLACEBO_SHADERS_ICC_H_
#define LIBPLACEBO_SHADERS_ICC_H_

#include <libplacebo/cache.h>
#include <libplacebo/colorspace.h>
#include <libplacebo/shaders.h>

PL_API_BEGIN

struct pl_icc_params {
    enum pl_rendering_intent intent;
    int size_r, size_g, size_b;
    float max_luma;
    bool force_bpc;
    pl_cache cache;
    // deprecated since v6.321
    void *cache_priv;
    void (*cache_save)(void *priv, uint64_t sig, const uint8_t *cache, size_t size);
    bool (*cache_load)(void *priv, uint64_t sig, uint8_t *cache, size_t size);
};

typedef const struct pl_icc_object_t {
    struct pl_icc_params params;
    uint64_t signature;
    struct pl_color_space csp;
    float gamma;
    enum pl_color_primaries containing_primaries;
} *pl_icc_object;

#define PL_ICC_DEFAULTS                         \
    .intent = PL_INTENT_RELATIVE_COLORIMETRIC,  \
    .max_luma = PL_COLOR_SDR_WHITE,

#define pl_icc_params(...) (&(struct pl_icc_params) { PL_ICC_DEFAULTS __VA_ARGS__ })
PL_API extern const struct pl_icc_params pl_icc_default_params;

// The entry points (icc.h:97-131). pl_icc_open: only RGB profiles; NULL on failure (message
// logged). pl_icc_update: the same profile (by signature) under the same parameters keeps the
// object, under other parameters reopens it in place; another profile replaces it.
// pl_icc_decode: profile -> linear light in the profile's containing primaries (*out_csp);
// pl_icc_encode: the inverse. `lut` holds the direction's 3D table on the device.
PL_API pl_icc_object pl_icc_open(pl_log log, const struct pl_icc_profile *profile,
                                 const struct pl_icc_params *params);
PL_API void pl_icc_close(pl_icc_object *icc);
PL_API bool pl_icc_update(pl_log log, pl_icc_object *obj,
                          const struct pl_icc_profile *profile,
                          const struct pl_icc_params *params);
PL_API void pl_icc_decode(pl_shader sh, pl_icc_object profile, pl_shader_obj *lut,
                          struct pl_color_space *out_csp);
PL_API void pl_icc_encode(pl_shader sh, pl_icc_object profile, pl_shader_obj *lut);

PL_API_END

#endif // LIBPLACEBO_SHADERS_ICC_H_
