/*
 * The presentation loop every libplacebo application is written around, in plain C against the
 * public headers: start_frame -> pl_frame_from_swapchain -> pl_render_image -> submit_frame ->
 * swap_buffers, with pl_swapchain_colorspace_hint, _resize and _latency around it, and -- on this
 * backend -- a consumer that takes the submitted images and gives them back.
 *
 * It is compiled two ways:
 *   against include/ (tests/c/swapchain.mk, built by build()): the whole program;
 *   against the REFERENCE's headers, with -DSWAPCHAIN_LOOP_REFERENCE and compile-only
 *   (tests/test_swapchain_abi.py): the same loop with only the backend include swapped -- the
 *   swapchain then comes from `app_create_swapchain`, which an application would write with its
 *   backend's constructor. That the loop compiles unchanged is the point.
 *
 * usage: swapchain_loop [frames]      prints one line per consumed frame and a summary
 */
#include <stdio.h>
#include <stdlib.h>

#include <libplacebo/renderer.h>
#include <libplacebo/swapchain.h>

#ifdef SWAPCHAIN_LOOP_REFERENCE
#include <libplacebo/dummy.h>
extern pl_gpu app_create_gpu(pl_log log);
extern pl_swapchain app_create_swapchain(pl_gpu gpu, int w, int h);
#else
#include <libplacebo/hip.h>
#include <libplacebo/hip_swapchain.h>
#endif

enum { W = 70, H = 46 };

// the consumer's turn: the `pending` images that have been submitted and not yet taken
static int consume(pl_swapchain sw, int pending)
{
    int n = 0;
#ifndef SWAPCHAIN_LOOP_REFERENCE
    struct pl_hip_presented img;
    while (n < pending && pl_hip_swapchain_acquire(sw, &img, 1000000000ull)) {  // 1 s at most
        const uint32_t *row = img.host_ptr;
        printf("frame %llu: %dx%d %s, %d bit, first word 0x%08x\n", (unsigned long long) img.seq,
               img.tex->params.w, img.tex->params.h, img.tex->params.format->name,
               img.color_repr.bits.color_depth, row ? (unsigned) row[0] : 0u);
        pl_hip_swapchain_release(sw, img.tex, NULL);
        n++;
    }
#else
    (void) sw;
    n = pending;
#endif
    return n;
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 5;
    pl_log log = pl_log_create(PL_API_VER, pl_log_params(
        .log_cb = pl_log_simple,
        .log_level = PL_LOG_WARN,
    ));

#ifdef SWAPCHAIN_LOOP_REFERENCE
    pl_gpu gpu = app_create_gpu(log);
    pl_swapchain sw = gpu ? app_create_swapchain(gpu, W, H) : NULL;
#else
    pl_hip hip = pl_hip_create(log, pl_hip_params(.device = 0));
    pl_gpu gpu = hip ? hip->gpu : NULL;
    pl_swapchain sw = hip ? pl_hip_create_swapchain(hip, pl_hip_swapchain_params(
        .width = W,
        .height = H,
        .alpha = PL_ALPHA_NONE,
        .host_readback = true,
    )) : NULL;
#endif
    if (!sw) {
        fprintf(stderr, "swapchain_loop: no swapchain\n");
        return 1;
    }

    // an HDR10 source: a horizontal PQ ramp
    uint16_t *pixels = malloc((size_t) W * H * 4 * sizeof(uint16_t));
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            uint16_t *px = &pixels[4 * (y * W + x)];
            px[0] = px[1] = px[2] = (uint16_t) (65535u * x / (W - 1));
            px[3] = 65535;
        }
    }
    pl_tex src = pl_tex_create(gpu, pl_tex_params(
        .w = W,
        .h = H,
        .format = pl_find_named_fmt(gpu, "rgba16"),
        .sampleable = true,
        .host_writable = true,
        .initial_data = pixels,
    ));
    free(pixels);
    pl_renderer rr = pl_renderer_create(log, gpu);
    if (!src || !rr) {
        fprintf(stderr, "swapchain_loop: no source texture / renderer\n");
        return 1;
    }
    struct pl_frame image = {
        .num_planes = 1,
        .planes = {{
            .texture = src,
            .components = 4,
            .component_mapping = { 0, 1, 2, 3 },
        }},
        .repr = { .sys = PL_COLOR_SYSTEM_RGB, .levels = PL_COLOR_LEVELS_FULL },
        .color = pl_color_space_hdr10,
    };

    printf("latency %d\n", pl_swapchain_latency(sw));
    int rendered = 0, consumed = 0, skipped = 0;
    for (int i = 0; i < frames; i++) {
        // odd frames are presented as they are (PQ), even frames tone-mapped to sRGB; the last
        // one at half the size
        pl_swapchain_colorspace_hint(sw, i & 1 ? &image.color : NULL);
        if (i == frames - 1) {
            int w = W / 2, h = H / 2;
            if (!pl_swapchain_resize(sw, &w, &h))
                break;
        }

        struct pl_swapchain_frame frame;
        bool ok = pl_swapchain_start_frame(sw, &frame);
        if (!ok) {
            // no image free: let the consumer catch up, then go on
            consumed += consume(sw, rendered - consumed);
            skipped++;
            if (skipped > frames)
                break;
            i--;
            continue;
        }

        struct pl_frame target;
        pl_frame_from_swapchain(&target, &frame);
        if (!pl_render_image(rr, &image, &target, &pl_render_fast_params))
            fprintf(stderr, "swapchain_loop: pl_render_image failed\n");

        ok = pl_swapchain_submit_frame(sw);
        if (!ok)
            break;
        rendered++;

        pl_swapchain_swap_buffers(sw);
    }
    consumed += consume(sw, rendered - consumed);
    printf("rendered %d, consumed %d, start_frame refused %d times\n", rendered, consumed, skipped);

    pl_renderer_destroy(&rr);
    pl_tex_destroy(gpu, &src);
    pl_swapchain_destroy(&sw);
#ifndef SWAPCHAIN_LOOP_REFERENCE
    pl_hip_destroy(&hip);
#endif
    pl_log_destroy(&log);
    return rendered == frames && consumed == frames ? 0 : 1;
}
