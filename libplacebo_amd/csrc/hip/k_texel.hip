/*
 * libplacebo-hip -- the transfer kernels of the emulated texture formats (bgra8, rgb10a2,
 * bgr10a2): what the reference does in pl_tex_upload_texel / pl_tex_download_texel
 * (src/gpu/utils.c:700-850, a compute pass between the caller's buffer and the texture). `unpack`
 * reads packed 32-bit words in host layout and writes the texture's storage (ordered rgba8 /
 * rgba16); `pack` is the way back. The arithmetic is plh_texel.h's.
 *
 * Pure streaming, one pass over the rect. Main path (VEC): a lane takes four consecutive texels,
 * one 16-byte access on the packed side and one (bgra8) or two (10-bit) on the storage side; the
 * last w % 4 texels of a row go one by one through the lane behind. Where a base address or a
 * pitch is not a multiple of 16 the launcher takes the per-texel instance instead (one texel per
 * lane, 4-byte packed accesses): decided once per launch, on the host.
 */
#include <hip/hip_runtime.h>

#include "backend.h"
#include "devmath.hiph"     // (plh_launch_status)
#include "plh_texel.h"

template <int FMT>
static __device__ inline void unpack_one(const uint8_t *prow, uint8_t *srow, int x)
{
    const uint32_t w = ((const uint32_t *) prow)[x];
    if (FMT == PLH_TEXEL_BGRA8) {
        ((uint32_t *) srow)[x] = plh_texel_swap_rb8(w);
    } else {
        uint2 t;
        plh_texel_unpack10(w, FMT == PLH_TEXEL_BGR10A2, &t.x, &t.y);
        ((uint2 *) srow)[x] = t;
    }
}

template <int FMT>
static __device__ inline void pack_one(const uint8_t *srow, uint8_t *prow, int x)
{
    if (FMT == PLH_TEXEL_BGRA8) {
        ((uint32_t *) prow)[x] = plh_texel_swap_rb8(((const uint32_t *) srow)[x]);
    } else {
        const uint2 t = ((const uint2 *) srow)[x];
        ((uint32_t *) prow)[x] = plh_texel_pack10(t.x, t.y, FMT == PLH_TEXEL_BGR10A2);
    }
}

// packed: w x h words at `packed`, rows `ppitch` bytes apart; storage likewise at `store` / `spitch`
template <int FMT, bool VEC>
__global__ void k_texel_unpack(const uint8_t *packed, size_t ppitch, uint8_t *store, size_t spitch,
                               int w, int h)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (y >= h)
        return;
    const uint8_t *prow = packed + (size_t) y * ppitch;
    uint8_t *srow = store + (size_t) y * spitch;
    if (!VEC) {
        if (i < w)
            unpack_one<FMT>(prow, srow, i);
        return;
    }
    const int x = 4 * i;
    if (x + 4 <= w) {
        const uint4 p = ((const uint4 *) prow)[i];
        if (FMT == PLH_TEXEL_BGRA8) {
            const uint4 o = { plh_texel_swap_rb8(p.x), plh_texel_swap_rb8(p.y),
                              plh_texel_swap_rb8(p.z), plh_texel_swap_rb8(p.w) };
            ((uint4 *) srow)[i] = o;
        } else {
            const int bgr = FMT == PLH_TEXEL_BGR10A2;
            uint4 a, b;
            plh_texel_unpack10(p.x, bgr, &a.x, &a.y);
            plh_texel_unpack10(p.y, bgr, &a.z, &a.w);
            plh_texel_unpack10(p.z, bgr, &b.x, &b.y);
            plh_texel_unpack10(p.w, bgr, &b.z, &b.w);
            ((uint4 *) srow)[2 * i] = a;
            ((uint4 *) srow)[2 * i + 1] = b;
        }
    } else {
        for (int k = x; k < w; k++)     // the row's tail: at most three texels
            unpack_one<FMT>(prow, srow, k);
    }
}

template <int FMT, bool VEC>
__global__ void k_texel_pack(const uint8_t *store, size_t spitch, uint8_t *packed, size_t ppitch,
                             int w, int h)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (y >= h)
        return;
    const uint8_t *srow = store + (size_t) y * spitch;
    uint8_t *prow = packed + (size_t) y * ppitch;
    if (!VEC) {
        if (i < w)
            pack_one<FMT>(srow, prow, i);
        return;
    }
    const int x = 4 * i;
    if (x + 4 <= w) {
        uint4 o;
        if (FMT == PLH_TEXEL_BGRA8) {
            const uint4 p = ((const uint4 *) srow)[i];
            o = { plh_texel_swap_rb8(p.x), plh_texel_swap_rb8(p.y),
                  plh_texel_swap_rb8(p.z), plh_texel_swap_rb8(p.w) };
        } else {
            const int bgr = FMT == PLH_TEXEL_BGR10A2;
            const uint4 a = ((const uint4 *) srow)[2 * i], b = ((const uint4 *) srow)[2 * i + 1];
            o = { plh_texel_pack10(a.x, a.y, bgr), plh_texel_pack10(a.z, a.w, bgr),
                  plh_texel_pack10(b.x, b.y, bgr), plh_texel_pack10(b.z, b.w, bgr) };
        }
        ((uint4 *) prow)[i] = o;
    } else {
        for (int k = x; k < w; k++)
            pack_one<FMT>(srow, prow, k);
    }
}

template <int FMT, bool VEC>
static void launch(hipStream_t s, int pack, const uint8_t *src, size_t src_pitch, uint8_t *dst,
                   size_t dst_pitch, int w, int h)
{
    const int lanes = VEC ? (w + 3) / 4 : w;
    const dim3 block(64, 4), grid((lanes + 63) / 64, (h + 3) / 4);
    if (pack) {
        hipLaunchKernelGGL((k_texel_pack<FMT, VEC>), grid, block, 0, s, src, src_pitch, dst,
                           dst_pitch, w, h);
    } else {
        hipLaunchKernelGGL((k_texel_unpack<FMT, VEC>), grid, block, 0, s, src, src_pitch, dst,
                           dst_pitch, w, h);
    }
}

template <int FMT>
static void launch_fmt(hipStream_t s, int pack, const uint8_t *src, size_t src_pitch, uint8_t *dst,
                       size_t dst_pitch, int w, int h)
{
    // the 16-byte path needs every row of both sides to start on a 16-byte boundary
    const bool vec = !(((uintptr_t) src | (uintptr_t) dst | src_pitch | dst_pitch) & 15);
    if (vec)
        launch<FMT, true>(s, pack, src, src_pitch, dst, dst_pitch, w, h);
    else
        launch<FMT, false>(s, pack, src, src_pitch, dst, dst_pitch, w, h);
}

extern "C" int plh_launch_texel_convert(plh_stream s, int texel_fmt, int pack, const void *src,
                                        size_t src_pitch, void *dst, size_t dst_pitch, int w, int h)
{
    if (w <= 0 || h <= 0)
        return 0;
    const uint8_t *sp = (const uint8_t *) src;
    uint8_t *dp = (uint8_t *) dst;
    switch (texel_fmt) {
    case PLH_TEXEL_BGRA8:   launch_fmt<PLH_TEXEL_BGRA8>((hipStream_t) s, pack, sp, src_pitch, dp, dst_pitch, w, h); break;
    case PLH_TEXEL_RGB10A2: launch_fmt<PLH_TEXEL_RGB10A2>((hipStream_t) s, pack, sp, src_pitch, dp, dst_pitch, w, h); break;
    case PLH_TEXEL_BGR10A2: launch_fmt<PLH_TEXEL_BGR10A2>((hipStream_t) s, pack, sp, src_pitch, dp, dst_pitch, w, h); break;
    default: return -(int) hipErrorInvalidValue;
    }
    return plh_launch_status();
}
