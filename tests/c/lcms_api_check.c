/*
 * libplacebo_amd/csrc/host/lcms_api.h declares by hand the part of LittleCMS 2 that the ICC code
 * calls through dlsym. This program includes it next to the installed lcms2.h / lcms2_plugin.h
 * and asserts that every constant, structure size and member offset is the header's, at compile
 * time; run, it also checks that the library the loader finds has every entry point on the list.
 * Prints "lcms_api_check: ok" and returns 0.
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include <lcms2.h>
#include <lcms2_plugin.h>

#include "lcms_api.h"

#define SAME(ours, theirs) _Static_assert((ours) == (theirs), #ours " != " #theirs)
#define SAME_MEMBER(ours, theirs, m)                                                        \
    _Static_assert(offsetof(ours, m) == offsetof(theirs, m), #ours "." #m ": offset");      \
    _Static_assert(sizeof(((ours *) 0)->m) == sizeof(((theirs *) 0)->m), #ours "." #m ": size")

SAME(PLH_CMS_TYPE_RGB_8, TYPE_RGB_8);
SAME(PLH_CMS_TYPE_RGB_16, TYPE_RGB_16);
SAME(PLH_CMS_TYPE_RGBA_16, TYPE_RGBA_16);
SAME(PLH_CMS_TYPE_XYZ_DBL, TYPE_XYZ_DBL);
SAME(PLH_CMS_FLAGS_NOCACHE, cmsFLAGS_NOCACHE);
SAME(PLH_CMS_FLAGS_NOOPTIMIZE, cmsFLAGS_NOOPTIMIZE);
SAME(PLH_CMS_FLAGS_BLACKPOINTCOMPENSATION, cmsFLAGS_BLACKPOINTCOMPENSATION);
SAME(PLH_CMS_INTENT_PERCEPTUAL, INTENT_PERCEPTUAL);
SAME(PLH_CMS_INTENT_RELATIVE_COLORIMETRIC, INTENT_RELATIVE_COLORIMETRIC);
SAME(PLH_CMS_INTENT_SATURATION, INTENT_SATURATION);
SAME(PLH_CMS_INTENT_ABSOLUTE_COLORIMETRIC, INTENT_ABSOLUTE_COLORIMETRIC);
SAME(PLH_CMS_SIG_RGB_DATA, cmsSigRgbData);
SAME(PLH_CMS_SIG_LUMINANCE_TAG, cmsSigLuminanceTag);
SAME(PLH_CMS_SIG_ATOB0_TAG, cmsSigAToB0Tag);
SAME(PLH_CMS_SIG_ATOB1_TAG, cmsSigAToB1Tag);
SAME(PLH_CMS_SIG_ATOB2_TAG, cmsSigAToB2Tag);
SAME(PLH_CMS_SIG_BTOA0_TAG, cmsSigBToA0Tag);
SAME(PLH_CMS_SIG_BTOA1_TAG, cmsSigBToA1Tag);
SAME(PLH_CMS_SIG_BTOA2_TAG, cmsSigBToA2Tag);
SAME(PLH_CMS_SIG_CLUT_ELEM_TYPE, cmsSigCLutElemType);
SAME(PLH_CMS_MAX_INPUT_DIMENSIONS, MAX_INPUT_DIMENSIONS);

// the scalar types the prototypes are written with
SAME(sizeof(uint32_t), sizeof(cmsUInt32Number));
SAME(sizeof(int32_t), sizeof(cmsInt32Number));
SAME(sizeof(int), sizeof(cmsBool));
SAME(sizeof(double), sizeof(cmsFloat64Number));
SAME(sizeof(uint32_t), sizeof(cmsColorSpaceSignature));
SAME(sizeof(uint32_t), sizeof(cmsTagSignature));
SAME(sizeof(uint32_t), sizeof(cmsStageSignature));
SAME(sizeof(void *), sizeof(cmsContext));
SAME(sizeof(void *), sizeof(cmsHPROFILE));
SAME(sizeof(void *), sizeof(cmsHTRANSFORM));

SAME(sizeof(plh_cmsCIEXYZ), sizeof(cmsCIEXYZ));
SAME_MEMBER(plh_cmsCIEXYZ, cmsCIEXYZ, X);
SAME_MEMBER(plh_cmsCIEXYZ, cmsCIEXYZ, Y);
SAME_MEMBER(plh_cmsCIEXYZ, cmsCIEXYZ, Z);
SAME(sizeof(plh_cmsCIExyY), sizeof(cmsCIExyY));
SAME_MEMBER(plh_cmsCIExyY, cmsCIExyY, x);
SAME_MEMBER(plh_cmsCIExyY, cmsCIExyY, y);
SAME_MEMBER(plh_cmsCIExyY, cmsCIExyY, Y);
SAME(sizeof(plh_cmsCIExyYTRIPLE), sizeof(cmsCIExyYTRIPLE));
SAME_MEMBER(plh_cmsCIExyYTRIPLE, cmsCIExyYTRIPLE, Red);
SAME_MEMBER(plh_cmsCIExyYTRIPLE, cmsCIExyYTRIPLE, Green);
SAME_MEMBER(plh_cmsCIExyYTRIPLE, cmsCIExyYTRIPLE, Blue);

// the leading members infer_clut_size reads
SAME_MEMBER(plh_cmsInterpParams, cmsInterpParams, ContextID);
SAME_MEMBER(plh_cmsInterpParams, cmsInterpParams, dwFlags);
SAME_MEMBER(plh_cmsInterpParams, cmsInterpParams, nInputs);
SAME_MEMBER(plh_cmsInterpParams, cmsInterpParams, nOutputs);
SAME_MEMBER(plh_cmsInterpParams, cmsInterpParams, nSamples);
SAME_MEMBER(plh_cmsStageCLutData, _cmsStageCLutData, Tab);
SAME_MEMBER(plh_cmsStageCLutData, _cmsStageCLutData, Params);

int main(void)
{
    // the header that was compiled against has every entry point on the list ...
#define DECLARED(ret, name, args) (void) &name;
    PLH_LCMS_ENTRY_POINTS(DECLARED)
#undef DECLARED

    // ... and so has the library the loader finds, where it finds one
    void *dl = dlopen("liblcms2.so.2", RTLD_NOW | RTLD_LOCAL);
    if (!dl) {
        printf("lcms_api_check: ok (constants and layouts; no liblcms2.so.2 to look into)\n");
        return 0;
    }
    int missing = 0;
#define EXPORTED(ret, name, args)                                   \
    if (!dlsym(dl, #name)) {                                        \
        printf("lcms_api_check: liblcms2.so.2 lacks %s\n", #name);  \
        missing++;                                                  \
    }
    PLH_LCMS_ENTRY_POINTS(EXPORTED)
#undef EXPORTED
    dlclose(dl);
    if (missing)
        return 1;
    printf("lcms_api_check: ok\n");
    return 0;
}
