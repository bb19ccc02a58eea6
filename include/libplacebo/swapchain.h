/*
 * libplacebo-hip: the presentation interface (libplacebo's swapchain.h).
 *
 * Source- and layout-compatible with the reference's header: the same two structs, the same seven
 * functions. A CDNA accelerator has no display, so the one implementation on this backend
 * (hip_swapchain.h) "presents" by handing the finished image to a consumer -- an encoder, another
 * stream, host memory. The render loop is the reference's:
 *
 *     struct pl_swapchain_frame frame;
 *     while (rendering) {
 *         if (!pl_swapchain_start_frame(sw, &frame))
 *             continue;                       // no image free: let the consumer catch up
 *         struct pl_frame target;
 *         pl_frame_from_swapchain(&target, &frame);
 *         pl_render_image(renderer, &image, &target, params);
 *         if (!pl_swapchain_submit_frame(sw))
 *             break;
 *         pl_swapchain_swap_buffers(sw);
 *     }
 */
#ifndef LIBPLACEBO_SWAPCHAIN_H_
#define LIBPLACEBO_SWAPCHAIN_H_

#include <libplacebo/common.h>
#include <libplacebo/colorspace.h>
#include <libplacebo/gpu.h>

PL_API_BEGIN

// A ring of target images on one pl_gpu. One producer thread (start_frame .. swap_buffers, resize,
// colorspace_hint) and, on this backend, one consumer thread (hip_swapchain.h) may use it at the
// same time.
typedef const struct pl_swapchain_t {
    pl_log log;
    pl_gpu gpu;
} *pl_swapchain;

// Waits for the work queued on the images, then frees them and the swapchain, and sets `*sw` to
// NULL. Nothing obtained from the swapchain may be used afterwards. NULL and a pointer to NULL are
// accepted.
PL_API void pl_swapchain_destroy(pl_swapchain *sw);

// How many submitted frames pl_swapchain_swap_buffers lets the GPU work on: with 1 it returns once
// the frame just submitted has finished, with 2 once the one before it has, and so on. 0 = unknown.
PL_API int pl_swapchain_latency(pl_swapchain sw);

// Sets and reports the size of the images. A non-zero `*width` / `*height` is a request, 0 only
// asks; on return both hold the size in force (which may differ from the request, and may be 0
// while there is none). False only when the swapchain is unusable.
PL_API bool pl_swapchain_resize(pl_swapchain sw, int *width, int *height);

// (older name of the struct)
#define pl_swapchain_colors pl_color_space

// Tells the swapchain what colour space the content is in. No answer comes back: what the
// swapchain makes of it shows in `pl_swapchain_frame.color_space` of the frames started afterwards,
// which is what rendering has to go by. Each call replaces the previous hint; NULL or an all-zero
// struct returns to the swapchain's own default. An HDR transfer without metadata gets
// pl_hdr_metadata_hdr10, metadata without a transfer gets PL_COLOR_TRC_PQ (pl_color_space_infer).
PL_API void pl_swapchain_colorspace_hint(pl_swapchain sw, const struct pl_color_space *csp);

// What pl_swapchain_start_frame hands out
struct pl_swapchain_frame {
    // The image to render into: `renderable` and `blit_dst`, nothing else is promised.
    pl_tex fbo;

    // The image will be shown upside down (row 0 at the bottom): render it mirrored. Never set on
    // this backend.
    bool flipped;

    // How the consumer of the image will interpret its samples: encoding, bit depth and alpha
    // mode, and the colour space.
    struct pl_color_repr color_repr;
    struct pl_color_space color_space;
};

// Starts a frame. False when there is no image to be had right now (for a benign reason, such as
// a size of 0x0 or a consumer that has not given one back yet): try again later. Whether the call
// waits for an image is up to the implementation; do not pace rendering by it.
PL_API bool pl_swapchain_start_frame(pl_swapchain sw, struct pl_swapchain_frame *out_frame);

// Submits the frame started last; does not wait. Frames are started and submitted strictly in
// turn, and reach the consumer in the order of submission. False on a lost device; the started
// frame is used up either way.
PL_API bool pl_swapchain_submit_frame(pl_swapchain sw);

// Waits until the GPU is no more than the swapchain's latency behind (pl_swapchain_latency), so
// that a render loop cannot queue work without bound. How long that takes varies from call to
// call: it is no clock.
PL_API void pl_swapchain_swap_buffers(pl_swapchain sw);

PL_API_END

#endif // LIBPLACEBO_SWAPCHAIN_H_
