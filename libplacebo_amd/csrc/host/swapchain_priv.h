/*
 * libplacebo-hip -- the backend half of a pl_swapchain, after the reference's
 * `struct pl_sw_fns` (src/swapchain.h): swapchain.c holds the public entry points and calls
 * through this table; swapchain_hip.c is the one implementation. The table pointer comes right
 * behind the public struct in the implementation's object.
 */
#ifndef PLH_SWAPCHAIN_PRIV_H_
#define PLH_SWAPCHAIN_PRIV_H_

#include <libplacebo/swapchain.h>

struct plh_sw_fns {
    void (*destroy)(pl_swapchain sw);
    int (*latency)(pl_swapchain sw);                                // optional
    bool (*resize)(pl_swapchain sw, int *width, int *height);       // optional
    // `csp`: never NULL, transfer and HDR metadata already defaulted
    void (*colorspace_hint)(pl_swapchain sw, const struct pl_color_space *csp);  // optional
    bool (*start_frame)(pl_swapchain sw, struct pl_swapchain_frame *out_frame);
    bool (*submit_frame)(pl_swapchain sw);
    void (*swap_buffers)(pl_swapchain sw);
};

struct plh_swapchain {
    struct pl_swapchain_t pub;
    const struct plh_sw_fns *fns;
};

#define SW_FNS(sw) (((const struct plh_swapchain *) (sw))->fns)

#endif // PLH_SWAPCHAIN_PRIV_H_
