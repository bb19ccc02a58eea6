/*
 * libplacebo-hip -- the part of LittleCMS 2's interface that shader_icc.c uses, declared by
 * hand: the library is loaded at run time (like RCCL in multigpu.c), so that neither a
 * link-time dependency nor an installed header is needed, and a machine without lcms2 keeps
 * the behaviour of a build without it.
 *
 * Every name here carries a plh_ / PLH_ prefix, so that tests/c/lcms_api_check.c can include
 * this file next to the installed lcms2.h / lcms2_plugin.h and hold each constant, size and
 * member offset to the header's.
 */
#ifndef PLH_LCMS_API_H_
#define PLH_LCMS_API_H_

#include <stdint.h>

typedef void *plh_cmsContext;
typedef void *plh_cmsHPROFILE;
typedef void *plh_cmsHTRANSFORM;
typedef struct plh_cms_curve plh_cmsToneCurve;      // opaque
typedef struct plh_cms_pipeline plh_cmsPipeline;
typedef struct plh_cms_stage plh_cmsStage;

typedef struct { double X, Y, Z; } plh_cmsCIEXYZ;
typedef struct { double x, y, Y; } plh_cmsCIExyY;
typedef struct { plh_cmsCIExyY Red, Green, Blue; } plh_cmsCIExyYTRIPLE;

// formatters: COLORSPACE_SH(s) = s << 16, EXTRA_SH(e) = e << 7, CHANNELS_SH(c) = c << 3,
// BYTES_SH(b) = b, FLOAT_SH(a) = a << 22; PT_RGB = 4, PT_XYZ = 9
#define PLH_CMS_TYPE_RGB_8      ((4u << 16) | (3u << 3) | 1u)
#define PLH_CMS_TYPE_RGB_16     ((4u << 16) | (3u << 3) | 2u)
#define PLH_CMS_TYPE_RGBA_16    ((4u << 16) | (1u << 7) | (3u << 3) | 2u)
#define PLH_CMS_TYPE_XYZ_DBL    ((1u << 22) | (9u << 16) | (3u << 3) | 0u)

#define PLH_CMS_FLAGS_NOCACHE                   0x0040u
#define PLH_CMS_FLAGS_NOOPTIMIZE                0x0100u
#define PLH_CMS_FLAGS_BLACKPOINTCOMPENSATION    0x2000u

// the rendering intents 0 .. 3 are enum pl_rendering_intent's values
#define PLH_CMS_INTENT_PERCEPTUAL               0u
#define PLH_CMS_INTENT_RELATIVE_COLORIMETRIC    1u
#define PLH_CMS_INTENT_SATURATION               2u
#define PLH_CMS_INTENT_ABSOLUTE_COLORIMETRIC    3u

#define PLH_CMS_SIG_RGB_DATA        0x52474220u     // 'RGB '
#define PLH_CMS_SIG_LUMINANCE_TAG   0x6C756D69u     // 'lumi'
#define PLH_CMS_SIG_ATOB0_TAG       0x41324230u     // 'A2B0'
#define PLH_CMS_SIG_ATOB1_TAG       0x41324231u
#define PLH_CMS_SIG_ATOB2_TAG       0x41324232u
#define PLH_CMS_SIG_BTOA0_TAG       0x42324130u     // 'B2A0'
#define PLH_CMS_SIG_BTOA1_TAG       0x42324131u
#define PLH_CMS_SIG_BTOA2_TAG       0x42324132u
#define PLH_CMS_SIG_CLUT_ELEM_TYPE  0x636C7574u     // 'clut'

// the leading members of cmsInterpParams and _cmsStageCLutData (lcms2_plugin.h): the grid size
// of a profile's own CLUT stages is read from them
#define PLH_CMS_MAX_INPUT_DIMENSIONS 15
typedef struct {
    plh_cmsContext ContextID;
    uint32_t dwFlags;
    uint32_t nInputs;
    uint32_t nOutputs;
    uint32_t nSamples[PLH_CMS_MAX_INPUT_DIMENSIONS];
    // (more follows)
} plh_cmsInterpParams;

typedef struct {
    union { uint16_t *T; float *TFloat; } Tab;
    plh_cmsInterpParams *Params;
    // (more follows)
} plh_cmsStageCLutData;

typedef void (*plh_cmsLogErrorHandlerFunction)(plh_cmsContext cms, uint32_t code, const char *text);

// The entry points, in one list: X(return type, name, parameters)
#define PLH_LCMS_ENTRY_POINTS(X)                                                                    \
    X(plh_cmsContext, cmsCreateContext, (void *plugin, void *user_data))                            \
    X(void, cmsDeleteContext, (plh_cmsContext cms))                                                 \
    X(void *, cmsGetContextUserData, (plh_cmsContext cms))                                          \
    X(void, cmsSetLogErrorHandlerTHR, (plh_cmsContext cms, plh_cmsLogErrorHandlerFunction fn))      \
    X(plh_cmsHPROFILE, cmsOpenProfileFromMemTHR, (plh_cmsContext cms, const void *mem, uint32_t size)) \
    X(int, cmsCloseProfile, (plh_cmsHPROFILE profile))                                              \
    X(uint32_t, cmsGetColorSpace, (plh_cmsHPROFILE profile))                                        \
    X(uint32_t, cmsGetHeaderRenderingIntent, (plh_cmsHPROFILE profile))                             \
    X(void, cmsSetHeaderRenderingIntent, (plh_cmsHPROFILE profile, uint32_t intent))                \
    X(void, cmsSetProfileVersion, (plh_cmsHPROFILE profile, double version))                        \
    X(uint32_t, cmsGetEncodedICCversion, (plh_cmsHPROFILE profile))                                 \
    X(int, cmsDetectDestinationBlackPoint, (plh_cmsCIEXYZ *black, plh_cmsHPROFILE profile,          \
                                            uint32_t intent, uint32_t flags))                       \
    X(void *, cmsReadTag, (plh_cmsHPROFILE profile, uint32_t sig))                                  \
    X(plh_cmsHPROFILE, cmsCreateXYZProfileTHR, (plh_cmsContext cms))                                \
    X(double, cmsSetAdaptationStateTHR, (plh_cmsContext cms, double d))                             \
    X(plh_cmsHTRANSFORM, cmsCreateTransformTHR, (plh_cmsContext cms, plh_cmsHPROFILE in,            \
                                                 uint32_t in_fmt, plh_cmsHPROFILE out,              \
                                                 uint32_t out_fmt, uint32_t intent, uint32_t flags)) \
    X(void, cmsDeleteTransform, (plh_cmsHTRANSFORM tf))                                             \
    X(void, cmsDoTransform, (plh_cmsHTRANSFORM tf, const void *in, void *out, uint32_t count))      \
    X(plh_cmsToneCurve *, cmsBuildParametricToneCurve, (plh_cmsContext cms, int32_t type,           \
                                                        const double params[]))                     \
    X(void, cmsFreeToneCurve, (plh_cmsToneCurve *curve))                                            \
    X(plh_cmsHPROFILE, cmsCreateRGBProfileTHR, (plh_cmsContext cms, const plh_cmsCIExyY *white,     \
                                                const plh_cmsCIExyYTRIPLE *primaries,               \
                                                plh_cmsToneCurve *const curves[3]))                 \
    X(plh_cmsStage *, cmsPipelineGetPtrToFirstStage, (const plh_cmsPipeline *pipe))                 \
    X(plh_cmsStage *, cmsStageNext, (const plh_cmsStage *stage))                                    \
    X(uint32_t, cmsStageType, (const plh_cmsStage *stage))                                          \
    X(void *, cmsStageData, (const plh_cmsStage *stage))

struct plh_lcms {
#define PLH_LCMS_MEMBER(ret, name, args) ret (*name) args;
    PLH_LCMS_ENTRY_POINTS(PLH_LCMS_MEMBER)
#undef PLH_LCMS_MEMBER
};

#endif // PLH_LCMS_API_H_
