/*
 * libplacebo-hip: a headless swapchain -- a ring of target images with a consumer side.
 *
 * The counterpart of pl_vulkan_create_swapchain / pl_opengl_create_swapchain on a device without a
 * display: "present" means "hand the finished image to a consumer". The producer runs the
 * reference's loop (swapchain.h); the consumer takes the submitted images in order with
 * pl_hip_swapchain_acquire and gives each back with pl_hip_swapchain_release.
 *
 * Image states. Every image of the ring is in one of four states:
 *     free       nobody uses it; pl_swapchain_start_frame may hand it out
 *     rendering  between pl_swapchain_start_frame and pl_swapchain_submit_frame
 *     presented  submitted, not yet acquired
 *     held       acquired, not yet released
 *
 * pl_swapchain_start_frame  takes a free image. It returns false, with one debug message, when no
 *     image is free or the size is 0x0. It never waits for the consumer: a caller that produces and
 *     consumes on one thread cannot deadlock in it. `flipped` is always false.
 * pl_swapchain_submit_frame  records the image's `ready_event` on the backend's stream -- with
 *     pl_hip_params.async_measure after making that stream wait for whatever the second stream
 *     still has to do with the image (what pl_hip_tex_access(gpu, tex, false) does) -- and, with
 *     `host_readback`, queues the download into the image's pinned host buffer behind it. It does
 *     not wait.
 * pl_swapchain_swap_buffers  waits until the GPU has finished the frame submitted `latency`
 *     submits ago, counting the one just submitted as the first (pl_swapchain_latency returns the
 *     value; 1 = wait for the frame just submitted). It never waits for the consumer.
 * pl_swapchain_colorspace_hint  takes effect at the next pl_swapchain_start_frame. The frame's
 *     `color_space` is the hint after pl_color_space_infer, with the HDR metadata it carries; NULL
 *     (or an all-zero struct) returns to pl_color_space_srgb. The defaults swapchain.h documents
 *     for every swapchain come first: an HDR transfer without metadata gets pl_hdr_metadata_hdr10
 *     (its primaries and luminance range, where inference alone would only fill in what is
 *     missing), metadata without a transfer gets PQ. Without a fixed `format` the ring is recreated in the format the hint
 *     selects (rgb10a2 for PQ / HLG, rgba8 otherwise) once no image is presented or held; until
 *     then frames keep the old format. `color_repr` is full-range
 *     RGB with the parameters' alpha mode, and its `bits.sample_depth` and `bits.color_depth` are
 *     the component depth of the image's format, so the renderer dithers to that depth by itself.
 * pl_swapchain_resize  takes effect at the next pl_swapchain_start_frame and writes back the size
 *     in force from then on. A request above limits.max_tex_2d_dim is clamped (and the clamped size
 *     reported). Images are recreated one by one as they come free: a presented or held image
 *     keeps its size until it has been released. An image released with a stream is not freed
 *     before that stream's work on it has completed (the one case in which start_frame waits).
 * pl_swapchain_destroy  waits for all queued work, then frees every image -- held ones too, which
 *     it says in a warning.
 *
 * Threads: one producer thread (everything in swapchain.h, and all other use of the pl_gpu) and
 * one consumer thread (acquire, release) may run at the same time; the swapchain keeps one mutex
 * and one condition variable. The consumer side touches nothing of the pl_gpu.
 */
#ifndef LIBPLACEBO_HIP_SWAPCHAIN_H_
#define LIBPLACEBO_HIP_SWAPCHAIN_H_

#include <libplacebo/hip.h>
#include <libplacebo/swapchain.h>

PL_API_BEGIN

struct pl_hip_swapchain_params {
    int width, height;      // initial size (0x0: no frames until pl_swapchain_resize)
    pl_fmt format;          // NULL = chosen from the hint: rgb10a2 for PQ / HLG, rgba8 otherwise
    int num_images;         // ring size, 0 = 3, at least 2
    int latency;            // frames the GPU may be behind swap_buffers, 0 = num_images - 1
    enum pl_alpha_mode alpha;
    bool host_readback;     // also copy every submitted image into a pinned host ring
};

#define pl_hip_swapchain_params(...) (&(struct pl_hip_swapchain_params) { __VA_ARGS__ })

// NULL (and an error message) on invalid parameters or when the first images cannot be created.
// The swapchain must be destroyed before the pl_hip it was created on.
PL_API pl_swapchain pl_hip_create_swapchain(pl_hip hip, const struct pl_hip_swapchain_params *params);

// One submitted image. Images arrive oldest first; `seq` counts the submits from 0.
struct pl_hip_presented {
    pl_tex tex;
    uint64_t seq;
    struct pl_color_repr color_repr;
    struct pl_color_space color_space;
    // hipEvent_t recorded behind all work that wrote `tex`. It has completed when acquire returns;
    // a consumer that polls ahead, or orders a stream of its own, may hipStreamWaitEvent on it.
    void *ready_event;
    // `host_readback` only, valid from the return of acquire until release: the image in the
    // format's host layout (for rgb10a2 the packed 32-bit words), rows `host_pitch` bytes apart.
    // The pointer of a ring slot stays the same for as long as the slot keeps its size and format.
    const void *host_ptr;
    size_t host_pitch;
};

// Takes the oldest presented image, which becomes held. `timeout_ns` 0 asks once; otherwise the
// call waits up to that long for an image to be submitted (on the condition variable) and for its
// GPU work to complete (on the event -- by polling it, the runtime having no timed wait: a few
// polls a yield apart, then every 50 us). True: `*out` is filled, the device work that wrote the
// image is complete and, with `host_readback`, so is the host copy. False: nothing was taken.
PL_API bool pl_hip_swapchain_acquire(pl_swapchain sw, struct pl_hip_presented *out, uint64_t timeout_ns);

// Gives a held image back; it becomes free. With a `consumer_stream` (hipStream_t) an event is
// recorded on that stream now, and the backend's stream waits for it before the image is rendered
// into again: work the consumer has queued there so far may still read the image. With NULL the
// caller states that it is done with the image. A texture that is not held is an error message and
// nothing else.
PL_API void pl_hip_swapchain_release(pl_swapchain sw, pl_tex tex, void *consumer_stream);

PL_API_END

#endif // LIBPLACEBO_HIP_SWAPCHAIN_H_
