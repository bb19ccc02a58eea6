/*
 * libplacebo-hip -- the headless swapchain (hip_swapchain.h): a ring of target textures between
 * one producer (the reference's start_frame / submit_frame / swap_buffers loop) and one consumer
 * (acquire / release). The contract is written out in the header; how it is kept:
 *
 *   * Every ring slot owns two events for its whole life: `ready`, recorded by submit_frame on the
 *     main stream behind everything that wrote the image, and `released`, recorded by release on
 *     the consumer's stream. Textures (and host buffers) come and go with resize and format
 *     changes, the events stay, so swap_buffers and a late consumer never hold a dead handle.
 *   * The pl_gpu is not thread-safe (limits.thread_safe is false), so only the producer side
 *     calls into it. The consumer side touches the slot table under the mutex and otherwise only
 *     waits for, or records, events -- which the HIP runtime allows from any thread. What the
 *     consumer's release asks of the main stream (wait for `released`) is noted in the slot and
 *     done by the producer's next start_frame on that slot.
 *   * Nothing waits for a GPU with the mutex held: neither side can stall the other that way.
 *   * host_readback goes through the public transfer path: pl_tex_download into a buffer imported
 *     from page-aligned memory of the slot's own (pinned by the import), which runs the copy --
 *     for rgb10a2 the packing kernel -- on the copy stream, beside the next frame. The buffer's
 *     fence is the event behind that copy; the consumer waits for it after `ready`. The texture
 *     remembers the copy (io_ev, gpu_hip.c), so the next render into the slot waits for it.
 */
#include <errno.h>
#include <pthread.h>
#include <sched.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <libplacebo/hip_swapchain.h>

#include "gpu_priv.h"
#include "swapchain_priv.h"

enum img_state { IMG_FREE = 0, IMG_RENDERING, IMG_PRESENTED, IMG_HELD };

struct sw_image {
    enum img_state state;
    pl_tex tex;
    uint64_t seq;
    struct pl_color_repr repr;
    struct pl_color_space csp;
    plh_event ready;        // submit_frame, main stream
    plh_event released;     // release, consumer's stream
    bool wait_released;     // the next render into the slot goes behind `released`
    // host_readback
    void *host_mem;         // whole pages, imported as `host_buf`
    size_t host_size, host_pitch;
    pl_buf host_buf;
    plh_event host_done;    // (borrowed: host_buf's fence) behind the latest copy
};

struct sw_priv {
    struct plh_swapchain base;
    pthread_mutex_t lock;
    pthread_cond_t cond;    // an image was submitted
    struct pl_hip_swapchain_params params;
    int num_images, latency;
    int w, h;               // in force from the next start_frame on
    pl_fmt fmt;             // of images created from now on
    struct pl_color_space hint;     // inferred
    struct sw_image *img;
    int *fifo, fifo_head, fifo_n;   // presented slots, oldest first
    int *hist;              // slot of submit `seq % num_images`
    int cur;                // the slot being rendered, or -1
    int next_slot;          // where the search for a free slot starts (round robin)
    uint64_t next_seq;
};

#define SW_PRIV(sw) ((struct sw_priv *) (sw))

static uint64_t now_ns(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t) ts.tv_sec * 1000000000ull + (uint64_t) ts.tv_nsec;
}

// `timeout` 0 asks once, otherwise polls until `deadline` -- the runtime has no timed wait for an
// event: a few polls a yield apart (a frame that is nearly done), then 50 us apart so that a long
// wait does not keep a core busy. A failed event counts as complete: waiting will not mend it,
// and pl_gpu_is_failed tells.
static bool event_reached(plh_event ev, uint64_t timeout, uint64_t deadline)
{
    for (int polls = 0; ; polls++) {
        if (plh_event_query(ev) != 0)
            return true;
        if (!timeout || now_ns() >= deadline)
            return false;
        if (polls < 16)
            sched_yield();
        else
            nanosleep(&(struct timespec) { .tv_nsec = 50000 }, NULL);
    }
}

static pl_fmt fmt_for_hint(const struct sw_priv *p)
{
    if (p->params.format)
        return p->params.format;
    const bool hdr = p->hint.transfer == PL_COLOR_TRC_PQ || p->hint.transfer == PL_COLOR_TRC_HLG;
    return pl_find_named_fmt(p->base.pub.gpu, hdr ? "rgb10a2" : "rgba8");
}

static void image_free(struct sw_priv *p, struct sw_image *im)
{
    pl_gpu gpu = p->base.pub.gpu;
    pl_tex_destroy(gpu, &im->tex);
    pl_buf_destroy(gpu, &im->host_buf);     // (waits for its own last copy, undoes the pinning)
    free(im->host_mem);
    im->host_mem = NULL;
    im->host_done = NULL;
    im->host_size = im->host_pitch = 0;
}

// The slot's texture (and host buffer) in the size and format in force; producer side, slot owned.
// `*wait_released`: the consumer released the image with a stream of its own, whose work may still
// read it. An image that stays is ordered behind that on the device by the caller; one that has
// to go is not freed before the consumer's event has completed (pl_tex_destroy drains the
// pl_gpu's own streams, not the consumer's), which settles the wait.
static bool image_ensure(struct sw_priv *p, struct sw_image *im, int w, int h, pl_fmt fmt,
                         bool *wait_released)
{
    pl_gpu gpu = p->base.pub.gpu;
    if (im->tex && im->tex->params.w == w && im->tex->params.h == h && im->tex->params.format == fmt)
        return true;
    if (*wait_released) {
        plh_event_sync(im->released);
        *wait_released = false;
    }
    image_free(p, im);
    im->tex = pl_tex_create(gpu, &(struct pl_tex_params) {
        .w = w, .h = h, .format = fmt,
        .sampleable = true, .renderable = true, .storable = true,
        .blit_src = true, .blit_dst = true, .host_writable = true, .host_readable = true,
    });
    if (!im->tex)
        return false;
    if (!p->params.host_readback)
        return true;

    // rows on the transfer pitch alignment, whole pages (the import registers pages)
    const size_t align = PL_DEF(gpu->limits.align_tex_xfer_pitch, 1);
    const size_t page = PL_DEF(gpu->limits.align_host_ptr, 4096);
    im->host_pitch = PL_ALIGN((size_t) w * fmt->texel_size, align);
    im->host_size = PL_ALIGN(im->host_pitch * (size_t) h, page);
    if (posix_memalign(&im->host_mem, page, im->host_size)) {
        im->host_mem = NULL;
        pl_msg(gpu->log, PL_LOG_ERR, "pl_hip swapchain: no host memory for a %zu byte frame",
               im->host_size);
        image_free(p, im);
        return false;
    }
    memset(im->host_mem, 0, im->host_size);
    im->host_buf = pl_buf_create(gpu, &(struct pl_buf_params) {
        .size = im->host_size,
        .host_readable = true,
        .import_handle = PL_HANDLE_HOST_PTR,
        .shared_mem = { .handle.ptr = im->host_mem, .size = im->host_size },
    });
    if (!im->host_buf) {
        image_free(p, im);
        return false;
    }
    return true;
}

static void hip_sw_destroy(pl_swapchain sw)
{
    struct sw_priv *p = SW_PRIV(sw);
    pl_gpu gpu = sw->gpu;
    pl_gpu_finish(gpu);
    int held = 0;
    for (int i = 0; i < p->num_images; i++)
        held += p->img[i].state == IMG_HELD;
    if (held) {
        pl_msg(sw->log, PL_LOG_WARN, "pl_swapchain_destroy: %d image%s still held by the consumer "
               "(acquired, not released): freed with the rest", held, held == 1 ? " is" : "s are");
    }
    for (int i = 0; i < p->num_images; i++) {
        struct sw_image *im = &p->img[i];
        if (im->wait_released)
            plh_event_sync(im->released);   // (a consumer's copy may still read the image)
        image_free(p, im);
        plh_event_destroy(im->ready);
        plh_event_destroy(im->released);
    }
    pthread_cond_destroy(&p->cond);
    pthread_mutex_destroy(&p->lock);
    free(p->img);
    free(p->fifo);
    free(p->hist);
    free(p);
}

static int hip_sw_latency(pl_swapchain sw)
{
    return SW_PRIV(sw)->latency;
}

static bool hip_sw_resize(pl_swapchain sw, int *width, int *height)
{
    struct sw_priv *p = SW_PRIV(sw);
    const int max = (int) PL_MIN(sw->gpu->limits.max_tex_2d_dim, (uint32_t) INT32_MAX);
    pthread_mutex_lock(&p->lock);
    if (*width > 0 && *height > 0) {
        const int w = PL_MIN(*width, max), h = PL_MIN(*height, max);
        if (w != *width || h != *height) {
            pl_msg(sw->log, PL_LOG_WARN, "pl_swapchain_resize: %dx%d exceeds max_tex_2d_dim (%d): "
                   "clamped to %dx%d", *width, *height, max, w, h);
        }
        p->w = w;
        p->h = h;
    }
    *width = p->w;
    *height = p->h;
    pthread_mutex_unlock(&p->lock);
    return true;
}

static void hip_sw_colorspace_hint(pl_swapchain sw, const struct pl_color_space *csp)
{
    struct sw_priv *p = SW_PRIV(sw);
    struct pl_color_space hint = *csp;
    pl_color_space_infer(&hint);
    pthread_mutex_lock(&p->lock);
    p->hint = hint;
    pthread_mutex_unlock(&p->lock);
}

static bool hip_sw_start_frame(pl_swapchain sw, struct pl_swapchain_frame *out_frame)
{
    struct sw_priv *p = SW_PRIV(sw);
    pl_gpu gpu = sw->gpu;

    pthread_mutex_lock(&p->lock);
    if (p->cur >= 0) {
        pthread_mutex_unlock(&p->lock);
        pl_msg(sw->log, PL_LOG_ERR, "pl_swapchain_start_frame: the previous frame has not been "
               "submitted");
        return false;
    }
    const int w = p->w, h = p->h;
    if (!w || !h) {
        pthread_mutex_unlock(&p->lock);
        pl_msg(sw->log, PL_LOG_DEBUG, "pl_swapchain_start_frame: the swapchain has no size (%dx%d)",
               w, h);
        return false;
    }
    int slot = -1, busy = 0;
    for (int n = 0; n < p->num_images; n++) {
        const int i = (p->next_slot + n) % p->num_images;
        if (p->img[i].state == IMG_FREE) {
            if (slot < 0)
                slot = i;
        } else {
            busy += p->img[i].state != IMG_RENDERING;
        }
    }
    if (slot < 0) {
        pthread_mutex_unlock(&p->lock);
        pl_msg(sw->log, PL_LOG_DEBUG, "pl_swapchain_start_frame: all %d images are presented or "
               "held: none free until the consumer releases one", p->num_images);
        return false;
    }
    // (a format the hint selects replaces the ring's only as a whole)
    pl_fmt want = fmt_for_hint(p);
    if (want && want != p->fmt && !busy)
        p->fmt = want;
    pl_fmt fmt = p->fmt;
    struct sw_image *im = &p->img[slot];
    im->state = IMG_RENDERING;
    p->cur = slot;
    p->next_slot = (slot + 1) % p->num_images;
    const struct pl_color_space csp = p->hint;
    bool wait_released = im->wait_released;
    im->wait_released = false;
    pthread_mutex_unlock(&p->lock);

    // from here on the slot is the producer's own
    bool ok = image_ensure(p, im, w, h, fmt, &wait_released);
    if (ok && wait_released && plh_stream_wait_event(plh_gpu_stream(gpu), im->released))
        ok = !plh_event_sync(im->released);
    if (!ok) {
        pl_msg(sw->log, PL_LOG_ERR, "pl_swapchain_start_frame: no %dx%d '%s' image", w, h,
               fmt->name);
        pthread_mutex_lock(&p->lock);
        im->state = IMG_FREE;
        p->cur = -1;
        pthread_mutex_unlock(&p->lock);
        return false;
    }
    // the image counts as written at this point of the main stream -- behind the consumer's
    // event and the slot's last host copy: whatever either stream does with it next is ordered
    // behind that
    plh_tex_order(gpu, 0, NULL, im->tex);

    const int depth = fmt->component_depth[0];
    im->repr = (struct pl_color_repr) {
        .sys = PL_COLOR_SYSTEM_RGB,
        .levels = PL_COLOR_LEVELS_FULL,
        .alpha = p->params.alpha,
        .bits = { .sample_depth = depth, .color_depth = depth },
    };
    im->csp = csp;
    *out_frame = (struct pl_swapchain_frame) {
        .fbo = im->tex,
        .flipped = false,
        .color_repr = im->repr,
        .color_space = im->csp,
    };
    return true;
}

static bool hip_sw_submit_frame(pl_swapchain sw)
{
    struct sw_priv *p = SW_PRIV(sw);
    pl_gpu gpu = sw->gpu;
    const int slot = p->cur;    // (only the producer writes it)
    if (slot < 0) {
        pl_msg(sw->log, PL_LOG_ERR, "pl_swapchain_submit_frame: no frame was started");
        return false;
    }
    struct sw_image *im = &p->img[slot];

    // the main stream behind what the measuring stream still does with the image, then the event
    plh_tex_order(gpu, 0, im->tex, NULL);
    int err = plh_event_record(im->ready, plh_gpu_stream(gpu));
    if (err)
        pl_msg(sw->log, PL_LOG_ERR, "pl_swapchain_submit_frame: %s", plh_strerror(err));
    bool ok = !err;
    if (ok && im->host_buf) {
        ok = pl_tex_download(gpu, &(struct pl_tex_transfer_params) {
            .tex = im->tex,
            .row_pitch = im->host_pitch,
            .buf = im->host_buf,
        });
        im->host_done = BUF_PRIV(im->host_buf)->fence;
    }
    ok = ok && !pl_gpu_is_failed(gpu);

    pthread_mutex_lock(&p->lock);
    p->cur = -1;
    if (ok) {
        im->seq = p->next_seq++;
        im->state = IMG_PRESENTED;
        p->hist[im->seq % p->num_images] = slot;
        p->fifo[(p->fifo_head + p->fifo_n++) % p->num_images] = slot;
        pthread_cond_broadcast(&p->cond);
    } else {
        im->state = IMG_FREE;   // the started frame is used up either way
    }
    pthread_mutex_unlock(&p->lock);
    return ok;
}

static void hip_sw_swap_buffers(pl_swapchain sw)
{
    struct sw_priv *p = SW_PRIV(sw);
    pthread_mutex_lock(&p->lock);
    plh_event ev = NULL;
    if (p->next_seq >= (uint64_t) p->latency) {
        // (a slot submitted again since then carries a later recording: waiting longer is safe)
        const uint64_t target = p->next_seq - p->latency;
        ev = p->img[p->hist[target % p->num_images]].ready;
    }
    pthread_mutex_unlock(&p->lock);
    if (ev && plh_event_sync(ev))
        pl_msg(sw->log, PL_LOG_ERR, "pl_swapchain_swap_buffers: waiting for the GPU failed");
}

static const struct plh_sw_fns hip_sw_fns = {
    .destroy = hip_sw_destroy,
    .latency = hip_sw_latency,
    .resize = hip_sw_resize,
    .colorspace_hint = hip_sw_colorspace_hint,
    .start_frame = hip_sw_start_frame,
    .submit_frame = hip_sw_submit_frame,
    .swap_buffers = hip_sw_swap_buffers,
};

pl_swapchain pl_hip_create_swapchain(pl_hip hip, const struct pl_hip_swapchain_params *params)
{
    if (!hip || !params)
        return NULL;
    pl_gpu gpu = hip->gpu;
    const int num = PL_DEF(params->num_images, 3);
    const int latency = PL_DEF(params->latency, num - 1);
    if (num < 2 || num > 64 || latency < 1 || latency > num || params->width < 0 ||
        params->height < 0 || !params->width != !params->height) {
        pl_msg(gpu->log, PL_LOG_ERR, "pl_hip_create_swapchain: invalid parameters (%dx%d, "
               "num_images %d: 0 or 2..64, latency %d: 0 or 1..num_images)", params->width,
               params->height, params->num_images, params->latency);
        return NULL;
    }
    if (params->format && (!(params->format->caps & PL_FMT_CAP_RENDERABLE) ||
                           params->format->num_components < 3)) {
        pl_msg(gpu->log, PL_LOG_ERR, "pl_hip_create_swapchain: '%s' is no renderable format of "
               "three or four components", params->format->name);
        return NULL;
    }

    struct sw_priv *p = calloc(1, sizeof(*p));
    if (!p)
        return NULL;
    p->img = calloc(num, sizeof(*p->img));
    p->fifo = calloc(num, sizeof(*p->fifo));
    p->hist = calloc(num, sizeof(*p->hist));
    pthread_condattr_t ca;
    pthread_condattr_init(&ca);
    pthread_condattr_setclock(&ca, CLOCK_MONOTONIC);
    pthread_mutex_init(&p->lock, NULL);
    pthread_cond_init(&p->cond, &ca);
    pthread_condattr_destroy(&ca);
    p->base.pub.log = gpu->log;
    p->base.pub.gpu = gpu;
    p->base.fns = &hip_sw_fns;
    p->params = *params;
    p->num_images = num;
    p->latency = latency;
    p->cur = -1;
    p->hint = pl_color_space_srgb;
    pl_color_space_infer(&p->hint);
    p->fmt = p->img && p->fifo && p->hist ? fmt_for_hint(p) : NULL;

    bool ok = !!p->fmt;
    for (int i = 0; ok && i < num; i++) {
        ok = !plh_fence_create(plh_gpu_device(gpu), &p->img[i].ready) &&
             !plh_fence_create(plh_gpu_device(gpu), &p->img[i].released);
    }
    if (ok) {
        p->num_images = num;
        int w = params->width, h = params->height;
        hip_sw_resize(&p->base.pub, &w, &h);
        for (int i = 0; ok && w && i < num; i++)
            ok = image_ensure(p, &p->img[i], w, h, p->fmt, &(bool) { false });
    }
    if (!ok) {
        pl_msg(gpu->log, PL_LOG_ERR, "pl_hip_create_swapchain: creating the ring failed");
        if (!p->img)
            p->num_images = 0;  // (no slots to go through)
        hip_sw_destroy(&p->base.pub);
        return NULL;
    }
    return &p->base.pub;
}

bool pl_hip_swapchain_acquire(pl_swapchain sw, struct pl_hip_presented *out, uint64_t timeout_ns)
{
    struct sw_priv *p = SW_PRIV(sw);
    const uint64_t deadline = now_ns() + PL_MIN(timeout_ns, (uint64_t) INT64_MAX / 2);
    const struct timespec until = { .tv_sec = deadline / 1000000000ull,
                                    .tv_nsec = deadline % 1000000000ull };
    pthread_mutex_lock(&p->lock);
    while (!p->fifo_n) {
        if (!timeout_ns || pthread_cond_timedwait(&p->cond, &p->lock, &until) == ETIMEDOUT) {
            if (p->fifo_n)
                break;
            pthread_mutex_unlock(&p->lock);
            return false;
        }
    }
    const int slot = p->fifo[p->fifo_head];
    struct sw_image *im = &p->img[slot];
    plh_event ready = im->ready, host_done = im->host_done;
    pthread_mutex_unlock(&p->lock);

    // (a presented slot is nobody else's: the producer takes free ones, there is one consumer)
    if (!event_reached(ready, timeout_ns, deadline) ||
        (host_done && !event_reached(host_done, timeout_ns, deadline)))
        return false;

    pthread_mutex_lock(&p->lock);
    p->fifo_head = (p->fifo_head + 1) % p->num_images;
    p->fifo_n--;
    im->state = IMG_HELD;
    *out = (struct pl_hip_presented) {
        .tex = im->tex,
        .seq = im->seq,
        .color_repr = im->repr,
        .color_space = im->csp,
        .ready_event = im->ready,
        .host_ptr = im->host_buf ? im->host_mem : NULL,
        .host_pitch = im->host_buf ? im->host_pitch : 0,
    };
    pthread_mutex_unlock(&p->lock);
    return true;
}

void pl_hip_swapchain_release(pl_swapchain sw, pl_tex tex, void *consumer_stream)
{
    struct sw_priv *p = SW_PRIV(sw);
    pthread_mutex_lock(&p->lock);
    struct sw_image *im = NULL;
    for (int i = 0; tex && i < p->num_images; i++) {
        // (state first: `tex` of a slot being rendered is the producer's to rewrite)
        if (p->img[i].state == IMG_HELD && p->img[i].tex == tex)
            im = &p->img[i];
    }
    if (!im) {
        pl_msg(sw->log, PL_LOG_ERR, "pl_hip_swapchain_release: %p is not an image held by the "
               "consumer (not of this swapchain, not acquired, or released already)", (void *) tex);
        pthread_mutex_unlock(&p->lock);
        return;
    }
    bool drain = false;
    if (consumer_stream) {
        if (plh_event_record(im->released, consumer_stream))
            drain = true;   // (no event to be had: the blunt way, below)
        else
            im->wait_released = true;
    }
    if (!drain)
        im->state = IMG_FREE;
    pthread_mutex_unlock(&p->lock);
    if (drain) {
        plh_stream_sync(consumer_stream);
        pthread_mutex_lock(&p->lock);
        im->state = IMG_FREE;
        pthread_mutex_unlock(&p->lock);
    }
}
