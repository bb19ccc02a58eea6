// The kernels a test hook launches itself on the stage texture (tests/hooks/testhooks.c): what a
// caller's own processing looks like to the renderer. Both work on rgba16hf textures given as
// pointer / pitch (bytes) / size, one thread per output texel, the ragged edge guarded, one 8-byte
// vector store per texel.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

struct texel { _Float16 r, g, b, a; };
static_assert(sizeof(texel) == 8, "rgba16hf texel");

__device__ inline const texel *at(const void *base, size_t pitch, int x, int y)
{
    return (const texel *) ((const char *) base + (size_t) y * pitch) + x;
}

__device__ inline texel *at(void *base, size_t pitch, int x, int y)
{
    return (texel *) ((char *) base + (size_t) y * pitch) + x;
}

// rgb -> 1 - x in fp32, rounded to nearest f16; alpha copied
__global__ void k_invert(const void *src, size_t src_pitch, void *dst, size_t dst_pitch, int w, int h)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h)
        return;
    const texel in = *at(src, src_pitch, x, y);
    texel out;
    out.r = (_Float16) (1.0f - (float) in.r);
    out.g = (_Float16) (1.0f - (float) in.g);
    out.b = (_Float16) (1.0f - (float) in.b);
    out.a = in.a;
    *at(dst, dst_pitch, x, y) = out;
}

// every source texel to a 2 x 2 block: dst is 2w x 2h
__global__ void k_double_nearest(const void *src, size_t src_pitch, void *dst, size_t dst_pitch,
                                 int w, int h)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= 2 * w || y >= 2 * h)
        return;
    *at(dst, dst_pitch, x, y) = *at(src, src_pitch, x >> 1, y >> 1);
}

dim3 grid_for(int w, int h, dim3 block)
{
    return dim3((w + block.x - 1) / block.x, (h + block.y - 1) / block.y);
}

} // namespace

extern "C" int th_launch_invert(void *stream, const void *src, size_t src_pitch, void *dst,
                                size_t dst_pitch, int w, int h)
{
    if (!src || !dst || w <= 0 || h <= 0 || src_pitch < (size_t) w * 8 || dst_pitch < (size_t) w * 8)
        return -1;
    const dim3 block(32, 8);
    k_invert<<<grid_for(w, h, block), block, 0, (hipStream_t) stream>>>(src, src_pitch, dst,
                                                                        dst_pitch, w, h);
    return (int) hipGetLastError();
}

extern "C" int th_launch_double_nearest(void *stream, const void *src, size_t src_pitch, void *dst,
                                        size_t dst_pitch, int w, int h)
{
    if (!src || !dst || w <= 0 || h <= 0 || src_pitch < (size_t) w * 8 ||
        dst_pitch < (size_t) w * 16)
        return -1;
    const dim3 block(32, 8);
    k_double_nearest<<<grid_for(2 * w, 2 * h, block), block, 0, (hipStream_t) stream>>>(
        src, src_pitch, dst, dst_pitch, w, h);
    return (int) hipGetLastError();
}
