/*
 * libplacebo-hip -- ICC colour management on LittleCMS 2, loaded at run time.
 *
 * Restates the behaviour of the reference's src/shaders/icc.c:
 *   detect_csp        :90-265   (primaries, known transfer, gamma estimate of a profile)
 *   detect_contrast   :267-303  (black point, v4 fall-back to the perceptual intent)
 *   infer_clut_size   :305-413
 *   icc_init          :415-521  (the approximation profile, the LUT signature)
 *   pl_icc_open / _update :523-622
 *   fill_lut          :624-680  (the 3D table through cmsDoTransform, force_bpc)
 *   pl_icc_decode / _encode :698-800 (device: colormap.hiph op_icc_decode / op_icc_encode)
 *
 * lcms2 is looked up in the process first and then loaded as liblcms2.so.2 (lcms_api.h), on the
 * first pl_icc_open that has a profile to open. Where that fails the entry points are those of
 * a libplacebo compiled without LittleCMS (src/shaders/icc.c:802-836): pl_icc_open fails with
 * the reference's message, pl_icc_update clears the object and fails (the message once),
 * pl_icc_close is a no-op, and the renderer renders a frame that carries a profile from its
 * pl_color_space (renderer.c: note_ignored_members).
 */
#include <dlfcn.h>
#include <math.h>
#include <pthread.h>
#include <stdbool.h>
#include <stdlib.h>
#include <string.h>

#include <libplacebo/shaders/icc.h>
#include <libplacebo/tone_mapping.h>

#include <libplacebo/hip.h>

#include "cache_priv.h"
#include "gpu_priv.h"
#include "host_common.h"
#include "lcms_api.h"
#include "shaders_priv.h"

const struct pl_icc_params pl_icc_default_params = { PL_ICC_DEFAULTS };

static const char no_lcms[] = "libplacebo compiled without LittleCMS 2 support!";

/* ---- the library ------------------------------------------------------------------------ */

static struct plh_lcms lcms_table;
static bool lcms_ok;
static pthread_once_t lcms_once = PTHREAD_ONCE_INIT;

static bool lcms_resolve(void *from)
{
#define RESOLVE(ret, name, args)                                    \
    *(void **) &lcms_table.name = dlsym(from, #name);               \
    if (!lcms_table.name)                                           \
        return false;
    PLH_LCMS_ENTRY_POINTS(RESOLVE)
#undef RESOLVE
    return true;
}

static void lcms_load(void)
{
    // the process scope first: an application that links lcms2 itself keeps its copy
    if (dlsym(RTLD_DEFAULT, "cmsCreateContext") && lcms_resolve(RTLD_DEFAULT)) {
        lcms_ok = true;
        return;
    }
    void *dl = dlopen("liblcms2.so.2", RTLD_NOW | RTLD_LOCAL);
    if (!dl)
        return;
    lcms_ok = lcms_resolve(dl);
    if (!lcms_ok)
        dlclose(dl);
}

static const struct plh_lcms *lcms_get(void)
{
    pthread_once(&lcms_once, lcms_load);
    return lcms_ok ? &lcms_table : NULL;
}

bool plh_icc_available(void)
{
    return lcms_get() != NULL;
}

/* ---- the object -------------------------------------------------------------------------- */

struct icc_obj {
    struct pl_icc_object_t pub;     // (first: a pl_icc_object points here)
    struct icc_obj *next_live;
    const struct plh_lcms *L;
    pl_log log;
    pl_cache cache;                 // the deprecated cache_save / cache_load callbacks as a pl_cache
    plh_cmsContext cms;
    plh_cmsHPROFILE profile;
    plh_cmsHPROFILE approx;         // approximation profile
    float a, b, scale;              // Y = scale * (a X + b)^gamma
    plh_cmsCIEXYZ *white, black;
    float gamma_stddev;
    uint64_t lut_sig;
};

// The objects that exist. A build without LittleCMS took any value in *obj (there never was an
// object: pl_icc_update and pl_icc_close only cleared it); a pointer that is none of ours is
// still only cleared, never read.
static struct icc_obj *live_objs;
static pthread_mutex_t live_lock = PTHREAD_MUTEX_INITIALIZER;

static struct icc_obj *icc_live(pl_icc_object icc)
{
    struct icc_obj *found = NULL;
    pthread_mutex_lock(&live_lock);
    for (struct icc_obj *o = live_objs; o && !found; o = o->next_live) {
        if (&o->pub == icc)
            found = o;
    }
    pthread_mutex_unlock(&live_lock);
    return found;
}

#define ICC_MSG(p, lev, ...) pl_msg((p)->log, lev, __VA_ARGS__)

static void error_callback(plh_cmsContext cms, uint32_t code, const char *msg)
{
    const struct plh_lcms *L = lcms_get();
    pl_log log = L ? L->cmsGetContextUserData(cms) : NULL;
    pl_msg(log, PL_LOG_ERR, "lcms2: [%d] %s", (int) code, msg);
}

static void legacy_set(void *priv, pl_cache_obj obj)
{
    pl_icc_object icc = priv;
    icc->params.cache_save(icc->params.cache_priv, obj.key, obj.data, obj.size);
}

static pl_cache_obj legacy_get(void *priv, uint64_t key)
{
    pl_icc_object icc = priv;
    const size_t size = (size_t) icc->params.size_r * icc->params.size_g * icc->params.size_b *
                        sizeof(uint16_t[4]);
    void *data = malloc(size);
    if (!data || !icc->params.cache_load(icc->params.cache_priv, key, data, size)) {
        free(data);
        return (pl_cache_obj) {0};
    }
    return (pl_cache_obj) { .key = key, .data = data, .size = size, .free = free };
}

static void icc_free(struct icc_obj *p)
{
    if (p->approx)
        p->L->cmsCloseProfile(p->approx);
    if (p->profile)
        p->L->cmsCloseProfile(p->profile);
    if (p->cms)
        p->L->cmsDeleteContext(p->cms);
    pl_cache_destroy(&p->cache);
    free(p);
}

void pl_icc_close(pl_icc_object *picc)
{
    if (!picc || !*picc)
        return;
    struct icc_obj *p = NULL;
    pthread_mutex_lock(&live_lock);
    for (struct icc_obj **o = &live_objs; *o; o = &(*o)->next_live) {
        if (&(*o)->pub == *picc) {
            p = *o;
            *o = p->next_live;
            break;
        }
    }
    pthread_mutex_unlock(&live_lock);
    if (p)
        icc_free(p);
    *picc = NULL;
}

// The probe of detect_csp: the primaries, white, black, mid grey, then the grey ramp without
// its end points
enum { T_RED, T_GREEN, T_BLUE, T_WHITE, T_BLACK, T_GRAY, T_RAMP, T_COUNT = T_RAMP + 254 };

static bool detect_csp(struct icc_obj *p)
{
    const struct plh_lcms *L = p->L;
    struct pl_icc_object_t *icc = &p->pub;
    plh_cmsHPROFILE xyz = L->cmsCreateXYZProfileTHR(p->cms);
    if (!xyz)
        return false;

    // an unadapted observer, for the raw values
    const double prev_adapt = L->cmsSetAdaptationStateTHR(p->cms, 0.0);
    plh_cmsHTRANSFORM tf = L->cmsCreateTransformTHR(p->cms, p->profile, PLH_CMS_TYPE_RGB_8, xyz,
            PLH_CMS_TYPE_XYZ_DBL, PLH_CMS_INTENT_ABSOLUTE_COLORIMETRIC,
            PLH_CMS_FLAGS_NOCACHE | PLH_CMS_FLAGS_NOOPTIMIZE);
    L->cmsSetAdaptationStateTHR(p->cms, prev_adapt);
    L->cmsCloseProfile(xyz);
    if (!tf)
        return false;

    uint8_t test[T_COUNT][3] = {
        [T_RED]   = { 0xFF, 0, 0 },
        [T_GREEN] = { 0, 0xFF, 0 },
        [T_BLUE]  = { 0, 0, 0xFF },
        [T_WHITE] = { 0xFF, 0xFF, 0xFF },
        [T_BLACK] = { 0, 0, 0 },
        [T_GRAY]  = { 0x80, 0x80, 0x80 },
    };
    for (int i = T_RAMP; i < T_COUNT; i++)
        test[i][0] = test[i][1] = test[i][2] = i - T_RAMP + 1;

    plh_cmsCIEXYZ dst[T_COUNT] = {0};
    L->cmsDoTransform(tf, test, dst, T_COUNT);
    L->cmsDeleteTransform(tf);

    struct pl_raw_primaries *measured = &icc->csp.hdr.prim;
    measured->red   = pl_cie_from_XYZ(dst[T_RED].X, dst[T_RED].Y, dst[T_RED].Z);
    measured->green = pl_cie_from_XYZ(dst[T_GREEN].X, dst[T_GREEN].Y, dst[T_GREEN].Z);
    measured->blue  = pl_cie_from_XYZ(dst[T_BLUE].X, dst[T_BLUE].Y, dst[T_BLUE].Z);
    measured->white = pl_cie_from_XYZ(dst[T_WHITE].X, dst[T_WHITE].Y, dst[T_WHITE].Z);

    // a named match, else the smallest named gamut that contains the measured one
    const struct pl_raw_primaries *best = NULL;
    for (int prim = 1; prim < PL_COLOR_PRIM_COUNT; prim++) {
        const struct pl_raw_primaries *raw = pl_raw_primaries_get(prim);
        if (!icc->csp.primaries && pl_raw_primaries_similar(raw, measured)) {
            icc->containing_primaries = icc->csp.primaries = prim;
            best = raw;
            break;
        }
        if (pl_primaries_superset(raw, measured) && (!best || pl_primaries_superset(best, raw))) {
            icc->containing_primaries = prim;
            best = raw;
        }
    }
    if (!best) {
        ICC_MSG(p, PL_LOG_WARN, "ICC profile too wide to handle, colors may be clipped!");
        icc->containing_primaries = PL_COLOR_PRIM_ACES_AP0;
    }

    // a known transfer function: 0.5 % stddev of the error over the ramp (:200-228, with the
    // reference's own black level for the comparison curve)
    const float contrast = icc->csp.hdr.max_luma / icc->csp.hdr.min_luma;
    const int N = T_COUNT - T_RAMP;
    float best_errsum = 0.0f;
    for (int trc = 1; trc < PL_COLOR_TRC_COUNT; trc++) {
        const struct pl_color_space ref = {
            .primaries = icc->csp.primaries,
            .transfer = trc,
            .hdr.max_luma = PL_COLOR_SDR_WHITE,
            .hdr.min_luma = PL_COLOR_SDR_WHITE * contrast,
        };
        float errsum = 0.0f;
        for (int i = T_RAMP; i < T_COUNT; i++) {
            const float x = test[i][0] / 255.0;
            float color[3] = { x, x, x };
            pl_color_linearize(&ref, color);
            const float delta = dst[i].Y - color[0];
            errsum += delta * delta;
        }
        const float tolerance = 5e-3f;
        if (errsum > N * PL_SQUARE(tolerance))
            continue;
        if (!icc->csp.transfer || errsum < best_errsum) {
            icc->csp.transfer = trc;
            best_errsum = errsum;
        }
    }

    // overall gamma from mid grey, as the starting point for the curve's black point
    const float y_approx = dst[T_GRAY].Y ? log(dst[T_GRAY].Y) / log(0.5) : 1.0f;
    const float kb = fmaxf(dst[T_BLACK].Y, 0.0f);
    float b = powf(kb, 1 / y_approx);

    // mean and stddev of the gamma over the ramp (Welford), the black point following the mean
    float M = 0.0, S = 0.0;
    int k = 1;
    for (int i = T_RAMP; i < T_COUNT; i++) {
        if (dst[i].Y <= 0 || dst[i].Y >= 1)
            continue;
        const float src = (1 - b) * (test[i][0] / 255.0) + b;
        const float y = log(dst[i].Y) / log(src);
        const float tmpM = M;
        M += (y - tmpM) / k;
        S += (y - tmpM) * (y - M);
        k++;
        b = powf(kb, 1 / M);
    }
    S = sqrt(S / (k - 1));

    if (M <= 0) {
        ICC_MSG(p, PL_LOG_ERR, "Arithmetic error in ICC profile gamma estimation? "
                "Please open an issue");
        return false;
    }
    icc->gamma = M;
    p->gamma_stddev = S;
    return true;
}

static bool detect_contrast(struct icc_obj *p, struct pl_icc_params *params)
{
    const struct plh_lcms *L = p->L;
    struct pl_hdr_metadata *hdr = &p->pub.csp.hdr;
    enum pl_rendering_intent intent = params->intent;

    // lcms refuses to detect a black point under the absolute colorimetric intent; only the
    // brightness matters here
    if (intent == PL_INTENT_ABSOLUTE_COLORIMETRIC)
        intent = PL_INTENT_RELATIVE_COLORIMETRIC;
    if (!L->cmsDetectDestinationBlackPoint(&p->black, p->profile, intent, 0)) {
        // v4 profiles carry a black point for the perceptual / saturation intents only
        if (L->cmsGetEncodedICCversion(p->profile) >= 0x4000000 && intent != PL_INTENT_PERCEPTUAL) {
            params->intent = PL_INTENT_PERCEPTUAL;
            return detect_contrast(p, params);
        }
        ICC_MSG(p, PL_LOG_ERR, "Failed detecting ICC profile black point!");
        return false;
    }

    float max_luma = params->max_luma;
    p->white = L->cmsReadTag(p->profile, PLH_CMS_SIG_LUMINANCE_TAG);
    if (max_luma <= 0)
        max_luma = p->white ? p->white->Y : PL_COLOR_SDR_WHITE;
    hdr->max_luma = max_luma;
    hdr->min_luma = p->black.Y * max_luma;
    hdr->min_luma = PL_MAX(hdr->min_luma, 1e-6);   // never a true 0
    return true;
}

// the pipeline whose CLUT stages set the table's resolution: B2A of the intent or the next one
// down (saturation -> colorimetric -> perceptual), else A2B likewise
static plh_cmsPipeline *intent_pipeline(struct icc_obj *p, const uint32_t tags[3])
{
    const struct plh_lcms *L = p->L;
    int first;
    switch (p->pub.params.intent) {
    case PL_INTENT_SATURATION: first = 2; break;
    case PL_INTENT_PERCEPTUAL: first = 0; break;
    default:                   first = 1; break;
    }
    for (int i = first; i >= 0; i--) {
        plh_cmsPipeline *pipe = L->cmsReadTag(p->profile, tags[i]);
        if (pipe)
            return pipe;
    }
    return NULL;
}

static void require_size(struct pl_icc_params *params, int n)
{
    params->size_r = PL_MAX(params->size_r, n);
    params->size_g = PL_MAX(params->size_g, n);
    params->size_b = PL_MAX(params->size_b, n);
}

static void infer_clut_size(struct icc_obj *p)
{
    const struct plh_lcms *L = p->L;
    struct pl_icc_params *params = &p->pub.params;
    if (params->size_r && params->size_g && params->size_b) {
        ICC_MSG(p, PL_LOG_DEBUG, "Using fixed 3DLUT size: %dx%dx%d",
                params->size_r, params->size_g, params->size_b);
        return;
    }

    require_size(params, 9);

    // enough steps to follow the (absolute) black point
    if (p->black.Y > 1e-4) {
        const float black_rel = powf(p->black.Y, 1.0f / p->pub.gamma);
        require_size(params, 2 * (int) ceilf(1.0f / black_rel));
    }

    // ... and the gamma curve
    if (p->gamma_stddev > 1e-2) {
        require_size(params, 65);
    } else if (p->gamma_stddev > 1e-3) {
        require_size(params, 33);
    } else if (p->gamma_stddev > 1e-4) {
        require_size(params, 17);
    }

    // ... and the profile's own CLUTs
    static const uint32_t b2a[3] = { PLH_CMS_SIG_BTOA0_TAG, PLH_CMS_SIG_BTOA1_TAG, PLH_CMS_SIG_BTOA2_TAG };
    static const uint32_t a2b[3] = { PLH_CMS_SIG_ATOB0_TAG, PLH_CMS_SIG_ATOB1_TAG, PLH_CMS_SIG_ATOB2_TAG };
    plh_cmsPipeline *pipe = intent_pipeline(p, b2a);
    if (!pipe)
        pipe = intent_pipeline(p, a2b);
    if (pipe) {
        for (plh_cmsStage *stage = L->cmsPipelineGetPtrToFirstStage(pipe); stage;
             stage = L->cmsStageNext(stage))
        {
            if (L->cmsStageType(stage) != PLH_CMS_SIG_CLUT_ELEM_TYPE)
                continue;
            const plh_cmsStageCLutData *data = L->cmsStageData(stage);
            if (data->Params->nInputs != 3)
                continue;
            params->size_r = PL_MAX(params->size_r, (int) data->Params->nSamples[0]);
            params->size_g = PL_MAX(params->size_g, (int) data->Params->nSamples[1]);
            params->size_b = PL_MAX(params->size_b, (int) data->Params->nSamples[2]);
        }
    }

    params->size_r = PL_MIN(params->size_r, 129);
    params->size_g = PL_MIN(params->size_g, 129);
    params->size_b = PL_MIN(params->size_b, 129);

    // roughly a million entries at the most
    const size_t max_size = 1000000;
    const size_t total_size = (size_t) params->size_r * params->size_g * params->size_b;
    if (total_size > max_size) {
        const float factor = powf((float) max_size / total_size, 1 / 3.0f);
        params->size_r = ceilf(factor * params->size_r);
        params->size_g = ceilf(factor * params->size_g);
        params->size_b = ceilf(factor * params->size_b);
    }
}

static bool icc_init(struct icc_obj *p)
{
    const struct plh_lcms *L = p->L;
    struct pl_icc_object_t *icc = &p->pub;
    struct pl_icc_params *params = &icc->params;
    if (params->intent < 0 || params->intent > PL_INTENT_ABSOLUTE_COLORIMETRIC)
        params->intent = L->cmsGetHeaderRenderingIntent(p->profile);

    if (!detect_contrast(p, params))
        return false;
    if (!detect_csp(p))
        return false;
    infer_clut_size(p);
    // (a fixed size is taken as given; one point per axis is no grid, and negative is no size)
    if (params->size_r < 2 || params->size_g < 2 || params->size_b < 2) {
        ICC_MSG(p, PL_LOG_ERR, "Invalid ICC 3DLUT size: %dx%dx%d", params->size_r, params->size_g,
                params->size_b);
        return false;
    }

    // The approximation profile: a pure power curve of the profile's gamma whose input is
    // stretched over the luminance range, Y = scale * (a X + b)^gamma (X the encoded value)
    p->scale = pl_hdr_rescale(PL_HDR_NITS, PL_HDR_NORM, icc->csp.hdr.max_luma);
    p->b = powf(icc->csp.hdr.min_luma / icc->csp.hdr.max_luma, 1.0f / icc->gamma);
    p->a = (1 - p->b);
    plh_cmsToneCurve *curve = L->cmsBuildParametricToneCurve(p->cms, 2,
            (double[3]) { icc->gamma, p->a, p->b });
    if (!curve)
        return false;

    const struct pl_raw_primaries *prim = pl_raw_primaries_get(icc->containing_primaries);
    const plh_cmsCIExyY wp_xyY = { prim->white.x, prim->white.y, 1.0 };
    const plh_cmsCIExyYTRIPLE prim_xyY = {
        .Red   = { prim->red.x,   prim->red.y,   1.0 },
        .Green = { prim->green.x, prim->green.y, 1.0 },
        .Blue  = { prim->blue.x,  prim->blue.y,  1.0 },
    };
    p->approx = L->cmsCreateRGBProfileTHR(p->cms, &wp_xyY, &prim_xyY,
                                          (plh_cmsToneCurve *[3]) { curve, curve, curve });
    L->cmsFreeToneCurve(curve);
    if (!p->approx)
        return false;

    // (v2: a v4 perceptual profile has normalised semantics; wanted is a colorimetric mapping
    // with black point compensation)
    L->cmsSetHeaderRenderingIntent(p->approx, icc->params.intent);
    L->cmsSetProfileVersion(p->approx, 2.2);

    // everything the generated table depends on
    p->lut_sig = PLH_CACHE_KEY_ICC_3DLUT;
    plh_hash_merge(&p->lut_sig, icc->signature);
    plh_hash_merge(&p->lut_sig, params->intent);
    plh_hash_merge(&p->lut_sig, params->size_r);
    plh_hash_merge(&p->lut_sig, params->size_g);
    plh_hash_merge(&p->lut_sig, params->size_b);
    plh_hash_merge(&p->lut_sig, params->force_bpc);
    union { double d; uint64_t u; } v = { .d = icc->csp.hdr.max_luma };
    plh_hash_merge(&p->lut_sig, v.u);

    if ((params->cache_save || params->cache_load) && !params->cache) {
        p->cache = pl_cache_create(pl_cache_params(
            .log  = p->log,
            .set  = params->cache_save ? legacy_set : NULL,
            .get  = params->cache_load ? legacy_get : NULL,
            .priv = icc,
        ));
    }

    ICC_MSG(p, PL_LOG_INFO, "Opened ICC profile:");
    if (p->white) {
        ICC_MSG(p, PL_LOG_DEBUG, "    Raw white point: X=%.2f Y=%.2f Z=%.2f cd/m^2",
                p->white->X, p->white->Y, p->white->Z);
    }
    ICC_MSG(p, PL_LOG_DEBUG, "    Raw black point: X=%.6f%% Y=%.6f%% Z=%.6f%%",
            p->black.X * 100, p->black.Y * 100, p->black.Z * 100);
    ICC_MSG(p, PL_LOG_INFO, "    Contrast = %.0f cd/m^2 : %.3f mcd/m^2 ≈ %.0f : 1",
            icc->csp.hdr.max_luma, icc->csp.hdr.min_luma * 1000,
            icc->csp.hdr.max_luma / icc->csp.hdr.min_luma);
    if (icc->csp.primaries) {
        ICC_MSG(p, PL_LOG_INFO, "    Detected primaries: %s",
                pl_color_primaries_name(icc->csp.primaries));
    } else {
        const struct pl_raw_primaries *raw = &icc->csp.hdr.prim;
        ICC_MSG(p, PL_LOG_DEBUG, "    Measured primaries:");
        ICC_MSG(p, PL_LOG_DEBUG, "      White: x=%.6f, y=%.6f", raw->white.x, raw->white.y);
        ICC_MSG(p, PL_LOG_DEBUG, "      Red:   x=%.3f, y=%.3f", raw->red.x, raw->red.y);
        ICC_MSG(p, PL_LOG_DEBUG, "      Green: x=%.3f, y=%.3f", raw->green.x, raw->green.y);
        ICC_MSG(p, PL_LOG_DEBUG, "      Blue:  x=%.3f, y=%.3f", raw->blue.x, raw->blue.y);
        ICC_MSG(p, PL_LOG_INFO, "    Containing primaries: %s",
                pl_color_primaries_name(icc->containing_primaries));
    }
    if (icc->csp.transfer) {
        ICC_MSG(p, PL_LOG_INFO, "    Transfer function: %s",
                pl_color_transfer_name(icc->csp.transfer));
    } else {
        ICC_MSG(p, PL_LOG_INFO, "    Approximation gamma: %.3f (stddev %.1f%s)",
                icc->gamma, p->gamma_stddev, p->gamma_stddev > 0.5 ? ", inaccurate!" : "");
    }
    return true;
}

pl_icc_object pl_icc_open(pl_log log, const struct pl_icc_profile *profile,
                          const struct pl_icc_params *params)
{
    if (!profile || !profile->len)
        return NULL;
    const struct plh_lcms *L = lcms_get();
    if (!L) {
        pl_msg(log, PL_LOG_ERR, "%s", no_lcms);
        return NULL;
    }

    struct icc_obj *p = calloc(1, sizeof(*p));
    if (!p)
        return NULL;
    p->L = L;
    p->pub.params = params ? *params : pl_icc_default_params;
    p->pub.signature = profile->signature;
    p->log = log;
    p->cms = L->cmsCreateContext(NULL, (void *) log);
    if (!p->cms) {
        ICC_MSG(p, PL_LOG_ERR, "Failed creating LittleCMS context!");
        goto error;
    }

    L->cmsSetLogErrorHandlerTHR(p->cms, error_callback);
    ICC_MSG(p, PL_LOG_DEBUG, "Opening new ICC profile");
    p->profile = L->cmsOpenProfileFromMemTHR(p->cms, profile->data, profile->len);
    if (!p->profile) {
        ICC_MSG(p, PL_LOG_ERR, "Failed opening ICC profile");
        goto error;
    }
    if (L->cmsGetColorSpace(p->profile) != PLH_CMS_SIG_RGB_DATA) {
        ICC_MSG(p, PL_LOG_ERR, "Invalid ICC profile: not RGB");
        goto error;
    }
    if (!icc_init(p))
        goto error;

    pthread_mutex_lock(&live_lock);
    p->next_live = live_objs;
    live_objs = p;
    pthread_mutex_unlock(&live_lock);
    return &p->pub;

error:
    icc_free(p);
    return NULL;
}

static bool icc_reopen(struct icc_obj *p, const struct pl_icc_params *params)
{
    p->L->cmsCloseProfile(p->approx);
    pl_cache_destroy(&p->cache);

    p->pub = (struct pl_icc_object_t) {
        .params    = *params,
        .signature = p->pub.signature,
    };
    p->approx = NULL;
    p->a = p->b = p->scale = 0.0f;
    p->white = NULL;
    p->black = (plh_cmsCIEXYZ) {0};
    p->gamma_stddev = 0.0f;
    p->lut_sig = 0;

    ICC_MSG(p, PL_LOG_DEBUG, "Reinitializing ICC profile in-place");
    return icc_init(p);
}

bool pl_icc_update(pl_log log, pl_icc_object *out_icc, const struct pl_icc_profile *profile,
                   const struct pl_icc_params *params)
{
    params = PL_DEF(params, &pl_icc_default_params);
    struct icc_obj *p = icc_live(*out_icc);
    if (!p)
        *out_icc = NULL;    // (whatever it was, it was no object)
    if (!p && !profile)
        return false;       // nothing to update
    if (!p && !lcms_get()) {
        static bool warned;
        if (!warned) {
            pl_msg(log, PL_LOG_ERR, "%s", no_lcms);
            warned = true;
        }
        return false;
    }

    const uint64_t sig = profile ? profile->signature : p->pub.signature;
    if (!p || p->pub.signature != sig) {
        pl_icc_close(out_icc);
        *out_icc = pl_icc_open(log, profile, params);
        return *out_icc != NULL;
    }

    const struct pl_icc_params *cur = &p->pub.params;
    const int size_r = PL_DEF(params->size_r, cur->size_r);
    const int size_g = PL_DEF(params->size_g, cur->size_g);
    const int size_b = PL_DEF(params->size_b, cur->size_b);
    const bool compat = params->intent    == cur->intent    &&
                        params->max_luma  == cur->max_luma  &&
                        params->force_bpc == cur->force_bpc &&
                        size_r            == cur->size_r    &&
                        size_g            == cur->size_g    &&
                        size_b            == cur->size_b;
    if (compat)
        return true;

    // the same profile under other parameters: reopened in place
    if (!icc_reopen(p, params)) {
        pl_icc_close(out_icc);
        return false;
    }
    return true;
}

/* ---- the tables --------------------------------------------------------------------------- */

struct fill_args {
    struct icc_obj *p;
    bool decode;
};

static int icc_fills;   // tables generated (not taken from a cache), for tests/test_icc.py

// size_r x size_g x size_b texels of RGBA16, red fastest: the grid through the transform
// profile -> approximation (decode) or back (encode)
static void fill_lut(void *datap, void *priv)
{
    const struct fill_args *args = priv;
    struct icc_obj *p = args->p;
    const struct plh_lcms *L = p->L;
    const struct pl_icc_params *params = &p->pub.params;
    plh_cmsHPROFILE srcp = args->decode ? p->profile : p->approx;
    plh_cmsHPROFILE dstp = args->decode ? p->approx : p->profile;
    const int s_r = params->size_r, s_g = params->size_g, s_b = params->size_b;

    __atomic_add_fetch(&icc_fills, 1, __ATOMIC_RELAXED);
    memset(datap, 0, (size_t) s_r * s_g * s_b * sizeof(uint16_t[4]));
    plh_cmsHTRANSFORM tf = L->cmsCreateTransformTHR(p->cms, srcp, PLH_CMS_TYPE_RGB_16, dstp,
            PLH_CMS_TYPE_RGBA_16, params->intent,
            PLH_CMS_FLAGS_BLACKPOINTCOMPENSATION | PLH_CMS_FLAGS_NOCACHE | PLH_CMS_FLAGS_NOOPTIMIZE);
    uint16_t *tmp = tf ? malloc((size_t) s_r * 3 * sizeof(tmp[0])) : NULL;
    if (!tmp)
        goto done;

    for (int b = 0; b < s_b; b++) {
        for (int g = 0; g < s_g; g++) {
            for (int r = 0; r < s_r; r++) {
                tmp[r * 3 + 0] = r * 65535 / (s_r - 1);
                tmp[r * 3 + 1] = g * 65535 / (s_g - 1);
                tmp[r * 3 + 2] = b * 65535 / (s_b - 1);
            }
            uint16_t *data = (uint16_t *) datap + ((size_t) b * s_g + g) * s_r * 4;
            L->cmsDoTransform(tf, tmp, data, s_r);
            if (!params->force_bpc)
                continue;

            // the black point by hand, for profiles black point compensation does not reach:
            // below the knee the output is pulled towards the input's own grey level
            const uint16_t knee = 16u << 8;
            if (tmp[0] >= knee || tmp[1] >= knee)
                continue;
            for (int r = 0; r < s_r; r++) {
                const uint16_t s = (2 * tmp[1] + tmp[2] + tmp[r * 3]) >> 2;
                if (s >= knee)
                    break;
                for (int c = 0; c < 3; c++)
                    data[r * 4 + c] = (s * data[r * 4 + c] + (knee - s) * s) >> 12;
            }
        }
    }

done:
    free(tmp);
    if (tf)
        L->cmsDeleteTransform(tf);
}

// the table of one direction, memoised with the sh_lut protocol under the reference's
// signatures (lut_sig for decode, ~lut_sig for encode); returns false if out of memory
static bool icc_table(struct icc_obj *p, bool decode, pl_cache fallback, uint16_t *out)
{
    const struct pl_icc_params *params = &p->pub.params;
    const size_t size = (size_t) params->size_r * params->size_g * params->size_b * sizeof(uint16_t[4]);
    pl_cache cache = PL_DEF(params->cache, PL_DEF(p->cache, fallback));
    struct fill_args args = { p, decode };
    const bool hit = plh_cache_memoize(cache, decode ? p->lut_sig : ~p->lut_sig, out, size,
                                       fill_lut, &args);
    ICC_MSG(p, PL_LOG_DEBUG, hit ? "Re-using cached ICC 3DLUT (%s)" : "Generated ICC 3DLUT (%s)",
            decode ? "decode" : "encode");
    return true;
}

// Test hooks (tests/test_icc.py): the table as it would be uploaded, without a device; returns
// the number of texels (out == NULL: only that). plh_test_icc_fills: tables generated so far.
PL_API size_t plh_test_icc_lut(pl_icc_object icc, int encode, uint16_t *out);
size_t plh_test_icc_lut(pl_icc_object icc, int encode, uint16_t *out)
{
    struct icc_obj *p = icc_live(icc);
    if (!p)
        return 0;
    const struct pl_icc_params *params = &icc->params;
    if (out)
        icc_table(p, !encode, NULL, out);
    return (size_t) params->size_r * params->size_g * params->size_b;
}

PL_API int plh_test_icc_fills(void);
int plh_test_icc_fills(void)
{
    return __atomic_load_n(&icc_fills, __ATOMIC_RELAXED);
}

/* ---- the shader stages --------------------------------------------------------------------- */

struct sh_icc_lut_obj {
    uint64_t signature;
    int size[3];
    pl_buf buf;     // rgba16 texels
};

static void icc_lut_uninit(pl_gpu gpu, void *priv)
{
    struct sh_icc_lut_obj *obj = priv;
    pl_buf_destroy(gpu, &obj->buf);
    memset(obj, 0, sizeof(*obj));
}

// the device table of one direction in `lut_obj`; NULL (shader failed) if it cannot be made
static struct plh_op *icc_lut_op(pl_shader sh, pl_icc_object icc, pl_shader_obj *lut_obj,
                                 bool decode, const char *who)
{
    struct icc_obj *p = icc_live(icc);
    if (!p) {
        SH_FAIL(sh, "%s: not an ICC object", who);
        return NULL;
    }
    if (!sh_require(sh, PL_SHADER_SIG_COLOR, 0, 0))
        return NULL;
    pl_gpu gpu = SH_GPU(sh);
    if (!gpu || !pl_find_named_fmt(gpu, "rgba16")) {
        SH_FAIL(sh, "Failed finding ICC 3DLUT texture format!");
        return NULL;
    }
    struct sh_icc_lut_obj *obj = SH_OBJ(sh, lut_obj, PL_SHADER_OBJ_LUT, struct sh_icc_lut_obj,
                                        icc_lut_uninit);
    if (!obj) {
        SH_FAIL(sh, "%s: failed generating LUT object", who);
        return NULL;
    }

    const struct pl_icc_params *params = &icc->params;
    const int size[3] = { params->size_r, params->size_g, params->size_b };
    const uint64_t sig = decode ? p->lut_sig : ~p->lut_sig;
    if (!obj->buf || obj->signature != sig || memcmp(obj->size, size, sizeof(size))) {
        const size_t bytes = (size_t) size[0] * size[1] * size[2] * sizeof(uint16_t[4]);
        uint16_t *texels = malloc(bytes);
        if (texels)
            icc_table(p, decode, plh_gpu_cache(gpu), texels);
        pl_buf_destroy(gpu, &obj->buf);
        if (texels) {
            obj->buf = pl_buf_create(gpu, pl_buf_params(.size = bytes, .storable = true,
                                                        .initial_data = texels));
        }
        free(texels);
        if (!obj->buf) {
            SH_FAIL(sh, "%s: failed generating LUT object", who);
            return NULL;
        }
        obj->signature = sig;
        memcpy(obj->size, size, sizeof(size));
    }

    struct plh_op *op = sh_op(sh, decode ? PLH_OP_ICC_DECODE : PLH_OP_ICC_ENCODE);
    if (!op)
        return NULL;
    op->i0 = size[0];
    op->i1 = size[1];
    op->i2 = size[2];
    op->ptr = pl_hip_buf_ptr(obj->buf);
    sh_hold(sh, *lut_obj);
    sh_describef(sh, "ICC 3DLUT");
    return op;
}

void pl_icc_decode(pl_shader sh, pl_icc_object icc, pl_shader_obj *lut_obj,
                   struct pl_color_space *out_csp)
{
    struct plh_op *op = icc_lut_op(sh, icc, lut_obj, true, "pl_icc_decode");
    if (!op)
        return;
    const struct icc_obj *p = icc_live(icc);

    // color.rgb = lut(color.rgb); Y = scale * (a X + b)^gamma
    op->f[0] = p->a;
    op->f[1] = p->b;
    op->f[2] = icc->gamma;
    op->f[3] = p->scale;
    sh_listf(sh, "icc_decode(%dx%dx%d, tetrahedral): color.rgb = %f * pow(%f * lut(color.rgb) + %f, %f)\n",
             op->i0, op->i1, op->i2, p->scale, p->a, p->b, icc->gamma);

    if (out_csp) {
        *out_csp = (struct pl_color_space) {
            .primaries  = icc->containing_primaries,
            .transfer   = PL_COLOR_TRC_LINEAR,
            .hdr        = icc->csp.hdr,
        };
    }
}

void pl_icc_encode(pl_shader sh, pl_icc_object icc, pl_shader_obj *lut_obj)
{
    struct plh_op *op = icc_lut_op(sh, icc, lut_obj, false, "pl_icc_encode");
    if (!op)
        return;
    const struct icc_obj *p = icc_live(icc);

    // X = 1/a * (Y / scale)^(1/gamma) - b/a; color.rgb = lut(X)
    op->f[0] = 1.0f / p->scale;
    op->f[1] = 1.0f / icc->gamma;
    op->f[2] = 1.0f / p->a;
    op->f[3] = p->b / p->a;
    sh_listf(sh, "icc_encode(%dx%dx%d, tetrahedral): color.rgb = lut(%f * pow(%f * max(color.rgb, 0), %f) - %f)\n",
             op->i0, op->i1, op->i2, op->f[2], op->f[0], op->f[1], op->f[3]);
}
