/*
 * libplacebo-hip — the blurred border's pyramid (pl_render_params.border = PL_CLEAR_BLUR):
 * one launch per level of the reference's pass_blur (src/renderer.c:2345-2465), see
 * struct plh_blur_args (plh_device.h) for what a pass computes.
 *
 * Read directly, the taps cost 20 (down) or 32 (up) texel fetches per output pixel. A workgroup
 * owns a PLH_BLUR_TILE^2 tile of outputs and first stages the input texels its taps reach, the
 * footprint, in LDS (decoded to fp32, MIRROR addressing resolved at load time); every tap then
 * reads LDS. The footprint is the bounding box of the tile's actual tap positions (odd level
 * sizes are no exact 2 : 1, so it is not derived from the ratio). A footprint larger than
 * PLH_BLUR_LDS (offsets far beyond the pyramid's usual 1 .. 1.8 texels) reads the taps from
 * memory instead: the same arithmetic either way.
 *
 * Numerics: the taps are tex_linear's exact-fp32 bilinear (samplers.hiph), summed in the GLSL's
 * order (products by 2 and 4 are exact), divided once (plh_div); the level is stored through
 * plh_store like every other intermediate.
 */
#include <climits>

#include "transfer.hiph"     // (plh_expf, which samplers.hiph uses)
#include "samplers.hiph"

template <bool UP>
struct blur_taps {
    static constexpr int N = UP ? 8 : 5;
};

// the tap positions of the output at (px, py), in the order the GLSL sums them
template <bool UP>
DEV void blur_positions(const plh_blur_args &a, float px, float py, float (&tx)[blur_taps<UP>::N],
                        float (&ty)[blur_taps<UP>::N])
{
    const float sx = a.step[0], sy = a.step[1];
    if constexpr (!UP) {
        tx[0] = px;      ty[0] = py;
        tx[1] = px - sx; ty[1] = py - sy;
        tx[2] = px + sx; ty[2] = py + sy;
        tx[3] = px - sx; ty[3] = py - (-sy);
        tx[4] = px + sx; ty[4] = py + (-sy);
    } else {
        const float s2x = sx + sx, s2y = sy + sy;
        tx[0] = px - s2x;  ty[0] = py - 0.0f;
        tx[1] = px + s2x;  ty[1] = py + 0.0f;
        tx[2] = px - 0.0f; ty[2] = py - s2y;
        tx[3] = px + 0.0f; ty[3] = py + s2y;
        tx[4] = px + -sx;  ty[4] = py + -sy;
        tx[5] = px + sx;   ty[5] = py + -sy;
        tx[6] = px + -sx;  ty[6] = py + sy;
        tx[7] = px + sx;   ty[7] = py + sy;
    }
}

// tex_linear against the staged footprint: `t` holds texels [ox, ox + fw) x [oy, ...)
DEV float4_t blur_tap_lds(const float4_t *t, int fw, int ox, int oy, const plh_view &v, float px,
                          float py)
{
    const float u = px * (float) v.w - 0.5f, w = py * (float) v.h - 0.5f;
    const float fu = __builtin_floorf(u), fv = __builtin_floorf(w);
    const float ax = u - fu, ay = w - fv;
    const float4_t *r0 = t + ((int) fv - oy) * fw + ((int) fu - ox);
    const float4_t *r1 = r0 + fw;
    return mix4(mix4(r0[0], r0[1], ax), mix4(r1[0], r1[1], ax), ay);
}

DEV void add4(float4_t &c, const float4_t &t)
{
    c.x = c.x + t.x; c.y = c.y + t.y; c.z = c.z + t.z; c.w = c.w + t.w;
}

template <bool UP>
__global__ __launch_bounds__(PLH_BLUR_TILE * PLH_BLUR_TILE)
void k_blur(plh_blur_args a)
{
    constexpr int N = blur_taps<UP>::N;
    __shared__ float4_t tile[PLH_BLUR_LDS];
    __shared__ int box[4];

    const int x = blockIdx.x * PLH_BLUR_TILE + (int) (threadIdx.x % PLH_BLUR_TILE);
    const int y = blockIdx.y * PLH_BLUR_TILE + (int) (threadIdx.x / PLH_BLUR_TILE);
    const bool in = x < a.dst.w && y < a.dst.h;

    const float mx = a.out_scale[0] * ((float) x + 0.5f);
    const float my = a.out_scale[1] * ((float) y + 0.5f);
    const float px = plh_attr(a.pos, 0, mx, my), py = plh_attr(a.pos, 1, mx, my);
    float tx[N], ty[N];
    blur_positions<UP>(a, px, py, tx, ty);

    // the footprint: the first texel of every tap's bilinear quad, over the tile
    if (threadIdx.x == 0) {
        box[0] = box[1] = INT_MAX;
        box[2] = box[3] = INT_MIN;
    }
    __syncthreads();
    if (in) {
        int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int ix = (int) __builtin_floorf(tx[i] * (float) a.src.w - 0.5f);
            const int iy = (int) __builtin_floorf(ty[i] * (float) a.src.h - 0.5f);
            x0 = min(x0, ix); x1 = max(x1, ix);
            y0 = min(y0, iy); y1 = max(y1, iy);
        }
        atomicMin(&box[0], x0); atomicMin(&box[1], y0);
        atomicMax(&box[2], x1); atomicMax(&box[3], y1);
    }
    __syncthreads();
    const int ox = box[0], oy = box[1];
    // (+1: the quad's second texel; 64-bit: a degenerate step may spread the taps arbitrarily)
    const long long fw = (long long) box[2] - ox + 2, fh = (long long) box[3] - oy + 2;
    const bool staged = fw * fh <= PLH_BLUR_LDS;    // uniform over the workgroup

    float4_t c;
    if (staged) {
        const int n = (int) (fw * fh), w = (int) fw;
        for (int i = threadIdx.x; i < n; i += PLH_BLUR_TILE * PLH_BLUR_TILE) {
            const int lx = i % w, ly = i / w;
            tile[i] = plh_fetch(a.src, plh_wrap(ox + lx, a.src.w, PLH_ADDRESS_MIRROR),
                                plh_wrap(oy + ly, a.src.h, PLH_ADDRESS_MIRROR));
        }
        __syncthreads();
        if (!in)
            return;
        float4_t t[N];
#pragma unroll
        for (int i = 0; i < N; i++)
            t[i] = blur_tap_lds(tile, w, ox, oy, a.src, tx[i], ty[i]);
        if (!UP) {
            c = scale4(t[0], 4.0f);
#pragma unroll
            for (int i = 1; i < N; i++)
                add4(c, t[i]);
        } else {
            c = t[0];
#pragma unroll
            for (int i = 1; i < N; i++)
                add4(c, i < 4 ? t[i] : scale4(t[i], 2.0f));
        }
    } else {
        if (!in)
            return;
        if (!UP) {
            c = scale4(tex_linear(a.src, PLH_ADDRESS_MIRROR, tx[0], ty[0]), 4.0f);
            for (int i = 1; i < N; i++)
                add4(c, tex_linear(a.src, PLH_ADDRESS_MIRROR, tx[i], ty[i]));
        } else {
            c = tex_linear(a.src, PLH_ADDRESS_MIRROR, tx[0], ty[0]);
            for (int i = 1; i < N; i++) {
                const float4_t t = tex_linear(a.src, PLH_ADDRESS_MIRROR, tx[i], ty[i]);
                add4(c, i < 4 ? t : scale4(t, 2.0f));
            }
        }
    }
    const float d = UP ? 12.0f : 8.0f;
    c.x = plh_div(c.x, d); c.y = plh_div(c.y, d); c.z = plh_div(c.z, d); c.w = plh_div(c.w, d);
    plh_store(a.dst, x, y, c);
}

extern "C" int plh_launch_blur(plh_stream stream, const plh_blur_args *args, int up)
{
    const dim3 grid((args->dst.w + PLH_BLUR_TILE - 1) / PLH_BLUR_TILE,
                    (args->dst.h + PLH_BLUR_TILE - 1) / PLH_BLUR_TILE);
    const dim3 block(PLH_BLUR_TILE * PLH_BLUR_TILE);
    if (up)
        PLH_LAUNCH_LAST(k_blur<true>, grid, block, 0, (hipStream_t) stream, *args);
    else
        PLH_LAUNCH_LAST(k_blur<false>, grid, block, 0, (hipStream_t) stream, *args);
    return plh_launch_status();
}
