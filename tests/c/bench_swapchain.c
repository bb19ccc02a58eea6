/*
 * Frames per second of a 4K rgb10a2 readback loop, two ways (profiles/swapchain_readback.md):
 *
 *   sync leg: pl_render_image into a plain texture, then one synchronous pl_tex_download into
 *             host memory per frame, then the host touches the frame. Uses nothing of
 *             swapchain.h, so it also builds against (and measures) a library without it:
 *             compile with -DBENCH_SYNC_ONLY.
 *   ring leg: the presentation loop (start_frame -> pl_frame_from_swapchain -> pl_render_image
 *             -> submit_frame -> swap_buffers) on a `host_readback` swapchain, with a consumer
 *             thread that acquires every image, touches its host copy and releases it.
 *
 * "Touches": reads one word of every 4 KiB of the frame. The source is a 4K HDR10 rgba16 frame,
 * the target has the same colour space (no tone mapping: the I/O is what is measured).
 *
 * usage: bench_swapchain [frames [warmup [sync|ring|both]]]      (default 200 20 both)
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <libplacebo/hip.h>
#include <libplacebo/renderer.h>
#ifndef BENCH_SYNC_ONLY
#include <libplacebo/hip_swapchain.h>
#endif

enum { W = 3840, H = 2160 };

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static void die(const char *what)
{
    fprintf(stderr, "bench_swapchain: %s\n", what);
    exit(1);
}

static uint64_t touch(const void *frame, size_t pitch, int rows)
{
    uint64_t sum = 0;
    const uint8_t *p = frame;
    for (size_t off = 0; off + 8 <= pitch * (size_t) rows; off += 4096)
        sum += *(const uint64_t *) (p + off);
    return sum;
}

#ifndef BENCH_SYNC_ONLY
struct consumer {
    pl_swapchain sw;
    int frames;
    int taken;
    uint64_t sum;
};

static void *consume(void *arg)
{
    struct consumer *c = arg;
    struct pl_hip_presented img;
    while (c->taken < c->frames && pl_hip_swapchain_acquire(c->sw, &img, 2000000000ull)) {
        c->sum += touch(img.host_ptr, img.host_pitch, img.tex->params.h);
        pl_hip_swapchain_release(c->sw, img.tex, NULL);
        c->taken++;
    }
    return NULL;
}
#endif

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 200;
    const int warmup = argc > 2 ? atoi(argv[2]) : 20;
    const char *legs = argc > 3 ? argv[3] : "both";
    const bool do_sync = strcmp(legs, "ring") != 0, do_ring = strcmp(legs, "sync") != 0;

    pl_log log = pl_log_create(PL_API_VER, pl_log_params(
        .log_cb = pl_log_simple,
        .log_level = PL_LOG_WARN,
    ));
    pl_hip hip = pl_hip_create(log, pl_hip_params(.device = 0));
    if (!hip)
        die("no HIP device");
    pl_gpu gpu = hip->gpu;
    pl_fmt rgb10a2 = pl_find_named_fmt(gpu, "rgb10a2");
    if (!rgb10a2)
        die("no rgb10a2");

    uint16_t *pixels = malloc((size_t) W * H * 4 * sizeof(uint16_t));
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) {
            uint16_t *px = &pixels[4 * ((size_t) y * W + x)];
            px[0] = (uint16_t) (x * 13 + y * 7);
            px[1] = (uint16_t) (x * 5 + y * 11);
            px[2] = (uint16_t) (x * 3 + y * 17);
            px[3] = 65535;
        }
    }
    pl_tex src = pl_tex_create(gpu, pl_tex_params(
        .w = W, .h = H, .format = pl_find_named_fmt(gpu, "rgba16"),
        .sampleable = true, .host_writable = true, .initial_data = pixels,
    ));
    free(pixels);
    pl_renderer rr = pl_renderer_create(log, gpu);
    if (!src || !rr)
        die("no source / renderer");
    const struct pl_color_repr repr = {
        .sys = PL_COLOR_SYSTEM_RGB, .levels = PL_COLOR_LEVELS_FULL, .alpha = PL_ALPHA_NONE,
        .bits = { .sample_depth = 10, .color_depth = 10 },
    };
    struct pl_frame image = {
        .num_planes = 1,
        .planes = {{ .texture = src, .components = 3, .component_mapping = { 0, 1, 2, -1 } }},
        .repr = { .sys = PL_COLOR_SYSTEM_RGB, .levels = PL_COLOR_LEVELS_FULL },
        .color = pl_color_space_hdr10,
    };
    uint64_t check = 0;

    if (do_sync) {
        pl_tex dst = pl_tex_create(gpu, pl_tex_params(
            .w = W, .h = H, .format = rgb10a2, .sampleable = true, .renderable = true,
            .storable = true, .blit_dst = true, .host_readable = true,
        ));
        const size_t pitch = (size_t) W * 4;
        void *host = malloc(pitch * H);
        if (!dst || !host)
            die("no target");
        struct pl_frame target = {
            .num_planes = 1,
            .planes = {{ .texture = dst, .components = 3, .component_mapping = { 0, 1, 2, 3 } }},
            .repr = repr,
            .color = pl_color_space_hdr10,
        };
        double t0 = 0;
        for (int i = 0; i < warmup + frames; i++) {
            if (i == warmup)
                t0 = now_ms();
            if (!pl_render_image(rr, &image, &target, &pl_render_fast_params))
                die("render failed");
            if (!pl_tex_download(gpu, pl_tex_transfer_params(.tex = dst, .ptr = host)))
                die("download failed");
            check += touch(host, pitch, H);
        }
        const double ms = (now_ms() - t0) / frames;
        printf("sync  %8.3f ms/frame  %8.1f fps\n", ms, 1e3 / ms);
        free(host);
        pl_tex_destroy(gpu, &dst);
    }

#ifndef BENCH_SYNC_ONLY
    if (do_ring) {
        pl_swapchain sw = pl_hip_create_swapchain(hip, pl_hip_swapchain_params(
            .width = W, .height = H, .format = rgb10a2, .alpha = PL_ALPHA_NONE,
            .host_readback = true,
        ));
        if (!sw)
            die("no swapchain");
        pl_swapchain_colorspace_hint(sw, &pl_color_space_hdr10);
        struct consumer c = { .sw = sw, .frames = warmup + frames };
        pthread_t thread;
        pthread_create(&thread, NULL, consume, &c);
        double t0 = 0;
        int refused = 0;
        for (int i = 0; i < warmup + frames; i++) {
            if (i == warmup)
                t0 = now_ms();
            struct pl_swapchain_frame frame;
            const double wait0 = now_ms();
            while (!pl_swapchain_start_frame(sw, &frame)) {
                refused++;
                if (now_ms() - wait0 > 2000)
                    die("no image came free in 2 s");
            }
            struct pl_frame target;
            pl_frame_from_swapchain(&target, &frame);
            if (!pl_render_image(rr, &image, &target, &pl_render_fast_params))
                die("render failed");
            if (!pl_swapchain_submit_frame(sw))
                die("submit failed");
            pl_swapchain_swap_buffers(sw);
        }
        pthread_join(thread, NULL);     // (the last frame counts once the consumer has it)
        const double ms = (now_ms() - t0) / frames;
        printf("ring  %8.3f ms/frame  %8.1f fps   (consumer took %d of %d, start_frame polled "
               "%d times in vain)\n", ms, 1e3 / ms, c.taken, warmup + frames, refused);
        check += c.sum;
        pl_swapchain_destroy(&sw);
    }
#else
    (void) do_ring;
    (void) repr;
#endif

    printf("checksum %016llx\n", (unsigned long long) check);
    pl_renderer_destroy(&rr);
    pl_tex_destroy(gpu, &src);
    pl_hip_destroy(&hip);
    pl_log_destroy(&log);
    return 0;
}
