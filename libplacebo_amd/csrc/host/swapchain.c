/*
 * libplacebo-hip -- the public pl_swapchain_* entry points (swapchain.h). They complete the
 * arguments the way the interface documents them and call through the implementation's table
 * (swapchain_priv.h), as gpu.c does for pl_gpu.
 */
#include <string.h>

#include "host_common.h"
#include "swapchain_priv.h"

void pl_swapchain_destroy(pl_swapchain *sw)
{
    if (!sw || !*sw)
        return;
    SW_FNS(*sw)->destroy(*sw);
    *sw = NULL;
}

int pl_swapchain_latency(pl_swapchain sw)
{
    return SW_FNS(sw)->latency ? SW_FNS(sw)->latency(sw) : 0;
}

bool pl_swapchain_resize(pl_swapchain sw, int *width, int *height)
{
    int none = 0;
    width = PL_DEF(width, &none);
    height = PL_DEF(height, &none);
    if (!SW_FNS(sw)->resize) {
        *width = *height = 0;
        return true;
    }
    return SW_FNS(sw)->resize(sw, width, height);
}

void pl_swapchain_colorspace_hint(pl_swapchain sw, const struct pl_color_space *csp)
{
    if (!SW_FNS(sw)->colorspace_hint)
        return;
    // NULL and {0} both mean "no hint"; metadata without a transfer means PQ, an HDR transfer
    // without metadata means HDR10's (swapchain.h)
    struct pl_color_space fix = pl_color_space_srgb;
    const struct pl_color_space none = {0};
    if (csp && !pl_color_space_equal(csp, &none)) {
        fix = *csp;
        const struct pl_hdr_metadata empty = {0};
        const bool has_metadata = !pl_hdr_metadata_equal(&fix.hdr, &empty);
        if (has_metadata && !fix.transfer)
            fix.transfer = PL_COLOR_TRC_PQ;
        else if (!has_metadata && pl_color_transfer_is_hdr(fix.transfer))
            fix.hdr = pl_hdr_metadata_hdr10;
    }
    SW_FNS(sw)->colorspace_hint(sw, &fix);
}

bool pl_swapchain_start_frame(pl_swapchain sw, struct pl_swapchain_frame *out_frame)
{
    memset(out_frame, 0, sizeof(*out_frame));   // (nothing stale on failure)
    return SW_FNS(sw)->start_frame(sw, out_frame);
}

bool pl_swapchain_submit_frame(pl_swapchain sw)
{
    return SW_FNS(sw)->submit_frame(sw);
}

void pl_swapchain_swap_buffers(pl_swapchain sw)
{
    SW_FNS(sw)->swap_buffers(sw);
}
