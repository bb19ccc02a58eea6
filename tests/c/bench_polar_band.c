/*
 * Time of ONE polar (EWA-Lanczos) downscaling pass out of a 3840 x 2160 rgba16 texture, through the
 * shader interface: the pass alone, no renderer around it. For a kernel trace
 * (profiles/polar_band.md); PL_HIP_POLAR_BAND=1 puts a pass k_polar would take on k_polar_band.
 *
 * usage: bench_polar_band out_w out_h [passes]
 * prints the pass's own description (filter radius, taps, LDS geometry) and the time per pass by the
 * host clock around a device synchronise
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <libplacebo/dispatch.h>
#include <libplacebo/hip.h>
#include <libplacebo/shaders/sampling.h>

#define SW 3840
#define SH 2160

static double now_us(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

static void die(const char *what)
{
    fprintf(stderr, "bench_polar_band: %s\n", what);
    exit(1);
}

int main(int argc, char **argv)
{
    if (argc < 3)
        die("usage: bench_polar_band out_w out_h [passes]");
    const int dw = atoi(argv[1]), dh = atoi(argv[2]);
    const int passes = argc > 3 ? atoi(argv[3]) : 20;
    if (dw < 1 || dh < 1 || passes < 1)
        die("bad arguments");

    pl_log log = pl_log_create(PL_API_VER, pl_log_params(.log_cb = pl_log_simple, .log_level = PL_LOG_WARN));
    pl_hip hip = pl_hip_create(log, pl_hip_params(.device = 0));
    if (!hip)
        die("no HIP device");
    pl_gpu gpu = hip->gpu;
    pl_dispatch dp = pl_dispatch_create(log, gpu);
    pl_fmt fmt = pl_find_named_fmt(gpu, "rgba16");

    // white noise from a fixed seed: no texel is like its neighbour
    uint16_t *pixels = malloc((size_t) SW * SH * 4 * sizeof(uint16_t));
    uint32_t x = 1;
    for (size_t i = 0; i < (size_t) SW * SH * 4; i++) {
        x = x * 1664525u + 1013904223u;
        pixels[i] = x >> 16;
    }
    pl_tex src = pl_tex_create(gpu, pl_tex_params(.w = SW, .h = SH, .format = fmt, .sampleable = true,
                                                  .host_writable = true, .initial_data = pixels));
    pl_tex dst = pl_tex_create(gpu, pl_tex_params(.w = dw, .h = dh, .format = fmt, .renderable = true,
                                                  .storable = true, .host_readable = true));
    if (!src || !dst)
        die("texture creation failed");

    pl_shader_obj lut = NULL;
    double t0 = 0;
    for (int f = -3; f < passes; f++) {
        if (f == 0) {
            pl_gpu_finish(gpu);
            t0 = now_us();
        }
        pl_shader sh = pl_dispatch_begin(dp);
        if (!pl_shader_sample_polar(sh, pl_sample_src(.tex = src, .new_w = dw, .new_h = dh),
                                    pl_sample_filter_params(.filter = pl_filter_ewa_lanczos, .lut = &lut)))
            die("pl_shader_sample_polar failed");
        if (f == -3) {
            const struct pl_shader_res *res = pl_shader_finalize(sh);
            printf("%s", res && res->glsl ? res->glsl : "(no description)\n");
        }
        if (!pl_dispatch_finish(dp, pl_dispatch_params(.shader = &sh, .target = dst)))
            die("pl_dispatch_finish failed");
    }
    pl_gpu_finish(gpu);
    const double us = (now_us() - t0) / passes;
    printf("polar %dx%d -> %dx%d (%.2fx): %.1f us per pass, %d passes\n", SW, SH, dw, dh,
           (double) SW / dw, us, passes);

    pl_shader_obj_destroy(&lut);
    pl_tex_destroy(gpu, &src);
    pl_tex_destroy(gpu, &dst);
    free(pixels);
    pl_dispatch_destroy(&dp);
    pl_hip_destroy(&hip);
    pl_log_destroy(&log);
    return 0;
}
