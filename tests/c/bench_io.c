/*
 * The frame loop of a caller that owns its frames in host memory: upload, render, download, per
 * frame. 1080p rgba16 in, bilinear to 4K rgba16 out (pl_render_fast_params), so that the I/O --
 * 17 MB in, 66 MB out -- dominates the 0.1 ms the render takes.
 *
 *   sync leg: `ptr` transfers from / into pageable memory; every transfer returns when the
 *             memory may be reused / is filled, i.e. drains the stream.
 *   ring leg: 3 source and 3 destination buffers imported from page-aligned host memory
 *             (PL_HANDLE_HOST_PTR), transfers with callbacks; before a slot is reused the loop
 *             polls that slot's buffers, nothing else. No call drains the stream.
 *
 * usage: bench_io [frames [warmup [sync|ring|both]]]      (default 200 20 both)
 * prints per leg: ms per frame; for the ring leg also the whole-stream drains per frame
 * (plh_test_stream_syncs, looked up at run time) and the callbacks that ran.
 */
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <libplacebo/hip.h>
#include <libplacebo/renderer.h>

#define SW 1920
#define SH 1080
#define DW 3840
#define DH 2160
#define RING 3
#define SRC_BYTES ((size_t) SW * SH * 8)
#define DST_BYTES ((size_t) DW * DH * 8)

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static void die(const char *what)
{
    fprintf(stderr, "bench_io: %s\n", what);
    exit(1);
}

static void fill(uint16_t *px, int seed)
{
    uint32_t s = 0x9e3779b9u * (uint32_t) (seed + 1);
    for (size_t i = 0; i < (size_t) SW * SH * 4; i++) {
        s = s * 1664525u + 1013904223u;
        px[i] = (i & 3) == 3 ? 65535 : (uint16_t) (s >> 16);
    }
}

static void count_cb(void *priv)
{
    ++*(int *) priv;
}

static pl_tex src_tex[RING], dst_tex[RING];
static struct pl_frame image, target;

static void render(pl_renderer rr, int slot)
{
    image.planes[0].texture = src_tex[slot];
    target.planes[0].texture = dst_tex[slot];
    if (!pl_render_image(rr, &image, &target, &pl_render_fast_params))
        die("pl_render_image failed");
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 200;
    const int warmup = argc > 2 ? atoi(argv[2]) : 20;
    const char *legs = argc > 3 ? argv[3] : "both";
    const int do_sync = strcmp(legs, "ring") != 0, do_ring = strcmp(legs, "sync") != 0;

    pl_log log = pl_log_create(PL_API_VER, pl_log_params(.log_cb = pl_log_simple, .log_level = PL_LOG_WARN));
    pl_hip hip = pl_hip_create(log, pl_hip_params(.device = 0));
    if (!hip)
        die("no HIP device");
    pl_gpu gpu = hip->gpu;
    pl_fmt fmt = pl_find_named_fmt(gpu, "rgba16");
    for (int i = 0; i < RING; i++) {
        src_tex[i] = pl_tex_create(gpu, pl_tex_params(.w = SW, .h = SH, .format = fmt, .sampleable = true,
                                                      .host_writable = true));
        dst_tex[i] = pl_tex_create(gpu, pl_tex_params(.w = DW, .h = DH, .format = fmt, .renderable = true,
                                                      .storable = true, .host_readable = true));
        if (!src_tex[i] || !dst_tex[i])
            die("texture creation failed");
    }
    const struct pl_color_repr full16 = {
        .sys = PL_COLOR_SYSTEM_RGB, .levels = PL_COLOR_LEVELS_FULL,
        .bits = { .sample_depth = 16, .color_depth = 16 },
    };
    image = (struct pl_frame) {
        .num_planes = 1, .planes = {{ .components = 3, .component_mapping = {0, 1, 2} }},
        .repr = full16, .color = pl_color_space_srgb,
    };
    target = (struct pl_frame) {
        .num_planes = 1, .planes = {{ .components = 4, .component_mapping = {0, 1, 2, 3} }},
        .repr = full16, .color = pl_color_space_srgb,
    };
    pl_renderer rr = pl_renderer_create(log, gpu);

    const long page = 4096 > gpu->limits.align_host_ptr ? 4096 : (long) gpu->limits.align_host_ptr;
    uint8_t *src_mem[RING], *dst_mem[RING];
    for (int i = 0; i < RING; i++) {
        if (posix_memalign((void **) &src_mem[i], page, SRC_BYTES) ||
            posix_memalign((void **) &dst_mem[i], page, DST_BYTES))
            die("out of host memory");
        fill((uint16_t *) src_mem[i], i);
        memset(dst_mem[i], 0, DST_BYTES);
    }
    uint64_t check[2] = {0, 0};

    if (do_sync) {
        double t0 = 0;
        for (int f = -warmup; f < frames; f++) {
            if (f == 0) {
                pl_gpu_finish(gpu);
                t0 = now_ms();
            }
            const int slot = (f + warmup) % RING;
            if (!pl_tex_upload(gpu, pl_tex_transfer_params(.tex = src_tex[slot], .ptr = src_mem[slot])))
                die("pl_tex_upload failed");
            render(rr, slot);
            if (!pl_tex_download(gpu, pl_tex_transfer_params(.tex = dst_tex[slot], .ptr = dst_mem[slot])))
                die("pl_tex_download failed");
        }
        pl_gpu_finish(gpu);
        printf("sync  %8.3f ms/frame\n", (now_ms() - t0) / frames);
        for (int i = 0; i < RING; i++)
            check[0] += ((uint64_t *) dst_mem[i])[DST_BYTES / 16 + i];
    }

    if (do_ring) {
        if (!(gpu->import_caps.buf & PL_HANDLE_HOST_PTR) || !gpu->limits.callbacks)
            die("this library imports no host pointers (ring leg)");
        uint64_t (*syncs)(pl_gpu) = (uint64_t (*)(pl_gpu)) dlsym(RTLD_DEFAULT, "plh_test_stream_syncs");
        pl_buf sbuf[RING], dbuf[RING];
        for (int i = 0; i < RING; i++) {
            memset(dst_mem[i], 0, DST_BYTES);
            sbuf[i] = pl_buf_create(gpu, pl_buf_params(.size = SRC_BYTES, .host_writable = true,
                .import_handle = PL_HANDLE_HOST_PTR, .shared_mem = { .handle.ptr = src_mem[i], .size = SRC_BYTES }));
            dbuf[i] = pl_buf_create(gpu, pl_buf_params(.size = DST_BYTES, .host_readable = true,
                .import_handle = PL_HANDLE_HOST_PTR, .shared_mem = { .handle.ptr = dst_mem[i], .size = DST_BYTES }));
            if (!sbuf[i] || !dbuf[i])
                die("import failed");
        }
        int uploaded = 0, downloaded = 0;
        uint64_t drains0 = 0;
        double t0 = 0;
        for (int f = -warmup; f < frames; f++) {
            if (f == 0) {
                pl_gpu_finish(gpu);
                uploaded = downloaded = 0;
                drains0 = syncs ? syncs(gpu) : 0;
                t0 = now_ms();
            }
            const int slot = (f + warmup) % RING;
            // the oldest frame in flight lives in this slot: wait for it alone, then the slot's
            // memory is the caller's again (here: a decoder would write the next picture)
            while (pl_buf_poll(gpu, dbuf[slot], UINT64_MAX))
                ;
            while (pl_buf_poll(gpu, sbuf[slot], UINT64_MAX))
                ;
            ((uint16_t *) src_mem[slot])[0] = (uint16_t) f;
            if (!pl_tex_upload(gpu, pl_tex_transfer_params(.tex = src_tex[slot], .buf = sbuf[slot],
                                                           .callback = count_cb, .priv = &uploaded)))
                die("pl_tex_upload failed");
            render(rr, slot);
            if (!pl_tex_download(gpu, pl_tex_transfer_params(.tex = dst_tex[slot], .buf = dbuf[slot],
                                                             .callback = count_cb, .priv = &downloaded)))
                die("pl_tex_download failed");
        }
        for (int i = 0; i < RING; i++) {
            while (pl_buf_poll(gpu, dbuf[i], UINT64_MAX))
                ;
        }
        const double ms = (now_ms() - t0) / frames;
        const uint64_t drains = syncs ? syncs(gpu) - drains0 : 0;
        pl_gpu_finish(gpu);     // (runs the callbacks still queued)
        printf("ring  %8.3f ms/frame   drains/frame %.3f%s   callbacks %d + %d of %d\n", ms,
               (double) drains / frames, syncs ? "" : " (no hook)", uploaded, downloaded, frames);
        for (int i = 0; i < RING; i++)
            check[1] += ((uint64_t *) dst_mem[i])[DST_BYTES / 16 + i];
        for (int i = 0; i < RING; i++) {
            pl_buf_destroy(gpu, &sbuf[i]);
            pl_buf_destroy(gpu, &dbuf[i]);
        }
    }
    // (the last frames of both legs render the same pictures but for one texel: a cheap look at
    // whether the downloads carried data at all)
    printf("check %016llx %016llx\n", (unsigned long long) check[0], (unsigned long long) check[1]);

    pl_renderer_destroy(&rr);
    for (int i = 0; i < RING; i++) {
        pl_tex_destroy(gpu, &src_tex[i]);
        pl_tex_destroy(gpu, &dst_tex[i]);
        free(src_mem[i]);
        free(dst_mem[i]);
    }
    pl_hip_destroy(&hip);
    pl_log_destroy(&log);
    return 0;
}
