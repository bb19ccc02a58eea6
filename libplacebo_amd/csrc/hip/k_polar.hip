/*
 * libplacebo-hip — polar (EWA) resampling kernel (K2/K3).
 *
 * Device half of pl_shader_sample_polar (src/shaders/sampling.c:587-912) and
 * polar_sample (:503-558), compute-shader formulation (:723-783):
 *
 *   fcoord = fract(pos*size - 0.5);  base texel = floor(pos*size - 0.5)
 *   for every tap (x, y) of the statically pruned list (host: tap order and
 *   flags are produced exactly like the reference's generation-time loops):
 *       d = length(vec2(x, y) - fcoord);   [if skippable: if (d < R)]
 *       w = LUT(d / R);  wsum += w;  color += w * texel(base + (x, y))
 *       [anti-ringing: weighted soft-min/max of taps with d <= radius_zero]
 *   color = scale / wsum * color;  [AR clamp];  alpha = 1 if not sampled
 *
 * MI355X mapping: a 256-thread workgroup (4 waves, 32x8 lanes) produces a
 * 32 x 8*rows output tile (rows = 4 unless the footprint would not fit). The source footprint of the tile
 * (ceil(32/ratio) + 2*ceil(R) texels square) is staged once in LDS as half4
 * (exactly the precision of the reference's rgba16hf FBO) or float4, together
 * with the 256-entry weight LUT stored as {L[i], L[i+1]} pairs so a tap costs
 * two ds_read_b64. Source texels are read from HBM once per tile with
 * row-contiguous lanes; the optional `pre-ops` (the reference's separate
 * "PASS A": normalise / decode / linearize / sigmoidize / FBO rounding) run on
 * the texels while they are being staged, which removes a full-frame FBO
 * write+read from the frame.
 */
#include "polar_common.hiph"

struct ar_state {
    float ar[4][2], wwsum[4][2];
};

template <typename T, uint32_t MASK, bool USE_AR>
__global__ __launch_bounds__(POLAR_BW * POLAR_BH)
void k_polar(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *lut = (float2 *) smem;                              // 256 pairs = 2 KiB
    tile_px<T> *tile = (tile_px<T> *) (smem + 256 * sizeof(float2));

    const plh_sampler_args &s = p.s;
    const int tid = threadIdx.y * POLAR_BW + threadIdx.x;
    const float sw = (float) s.src.w, sh = (float) s.src.h;

    // ---- workgroup footprint: base texel of the four corner lanes ----------
    const int rows = s.tile_rows;
    const int gx0 = blockIdx.x * POLAR_BW, gy0 = blockIdx.y * POLAR_BH * rows;
    int ox, oy;
    {
        int bx[2], by[2];
        for (int k = 0; k < 2; k++) {
            const float mx = p.out_scale[0] * ((float) (gx0 + k * (POLAR_BW - 1)) + 0.5f);
            const float my = p.out_scale[1] *
                ((float) (gy0 + k * (POLAR_BH * rows - 1)) + 0.5f);
            // pos.x only depends on (mx) when the quad is axis aligned, but we
            // evaluate the full bilinear attribute like every lane does
            const float cx = plh_attr(s.pos, 0, mx, p.out_scale[1] * ((float) gy0 + 0.5f));
            const float cy = plh_attr(s.pos, 1, p.out_scale[0] * ((float) gx0 + 0.5f), my);
            bx[k] = (int) __builtin_floorf(cx * sw - 0.5f);
            by[k] = (int) __builtin_floorf(cy * sh - 0.5f);
        }
        // one texel of slack on the low side (the host adds two to the tile
        // size): the corner estimate may be off by one when pos*size - 0.5
        // lands within rounding noise of an integer
        const int off = s.bound - 1;
        ox = min(bx[0], bx[1]) - off - 1;
        oy = min(by[0], by[1]) - off - 1;
    }

    // ---- stage LUT pairs + source tile in LDS ----------------------------------
    for (int i = tid; i < 256; i += POLAR_BW * POLAR_BH)
        lut[i] = ((const float2 *) s.lut)[i];

    const int tw = s.tile_w, th = s.tile_h;
    // an rgba16hf source without pre-ops is copied bit for bit (the f16 -> f32 -> f16 round
    // trip of the generic path is the identity)
    const bool raw16 = sizeof(tile_px<T>) == 8 && s.src.fmt == PLH_FMT_RGBA16F && !p.num_pre_ops;
    const float rcp_tw = 1.0f / (float) tw;
    for (int i = tid; i < tw * th; i += POLAR_BW * POLAR_BH) {
        const int ty = (int) (((float) i + 0.5f) * rcp_tw), tx = i - ty * tw;  // exact: i < 2^22
        const int sx = plh_wrap(ox + tx, s.src.w, s.address_mode);
        const int sy = plh_wrap(oy + ty, s.src.h, s.address_mode);
        if (raw16) {
            *(uint2 *) &tile[i] = *(const uint2 *) ((const char *) s.src.ptr +
                                                    (size_t) sy * s.src.pitch + (size_t) sx * 8);
            continue;
        }
        float4_t c = plh_fetch(s.src, sx, sy);
        if (p.num_pre_ops) {
            const frag_t fc = { (float) sx + 0.5f, (float) sy + 0.5f };
            apply_ops(c, p.ops, 0, p.num_pre_ops, fc);
        }
        tile_put(tile[i], c);
    }
    __syncthreads();

    // ---- taps -----------------------------------------------------------------------
    const int idx = gx0 + threadIdx.x;
    const float mx = p.out_scale[0] * ((float) idx + 0.5f);

#pragma unroll 1
    for (int r = 0; r < rows; r++) {
        const int idy = gy0 + threadIdx.y + r * POLAR_BH;
        const float my = p.out_scale[1] * ((float) idy + 0.5f);
        const float px = plh_attr(s.pos, 0, mx, my);
        const float py = plh_attr(s.pos, 1, mx, my);

        const float tx = px * sw - 0.5f, ty = py * sh - 0.5f;
        const float flx = __builtin_floorf(tx), fly = __builtin_floorf(ty);
        const float fcx = tx - flx, fcy = ty - fly;         // fcoord
        // tile index of tap (0,0); lanes outside the image footprint (padding
        // lanes of edge groups) are clamped so their LDS reads stay in range
        int relx = (int) flx - ox, rely = (int) fly - oy;
        relx = min(max(relx, s.bound - 1), tw - s.bound - 1);
        rely = min(max(rely, s.bound - 1), th - s.bound - 1);
        const tile_px<T> *tp = tile + rely * tw + relx;

        float col[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float wsum = 0.0f;
        ar_state ars;
        if (USE_AR) {
            for (int c = 0; c < 4; c++)
                ars.ar[c][0] = ars.ar[c][1] = ars.wwsum[c][0] = ars.wwsum[c][1] = 0.0f;
        }

        for (int t = 0; t < s.num_taps; t++) {
            const uint32_t tap = s.taps[t];
            const int x = (int8_t) (tap & 0xff), y = (int8_t) ((tap >> 8) & 0xff);
            const uint32_t fl = tap >> 16;

            float d;
            bool live;
            const float w = polar_weight(s, lut, tap, fcx, fcy, d, live);
            wsum += w;

            const float4_t c = tile_get(tp[y * tw + x]);
            const float cv[4] = { c.x, c.y, c.z, c.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (MASK & (1u << k))
                    col[k] = __builtin_fmaf(w, cv[k], col[k]);
            }

            if (USE_AR) {
                if ((fl & PLH_TAP_AR) && live && d <= s.radius_zero) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (!(MASK & (1u << k)))
                            continue;
                        float cc[2] = { 1.0f - s.scale * cv[k], s.scale * cv[k] };
                        for (int j = 0; j < 2; j++) {
                            float ww = cc[j] + 0.10f;
                            ww = ww * ww; ww = ww * ww; ww = ww * ww; ww = ww * ww; ww = ww * ww;
                            ww = w * ww;
                            ars.ar[k][j] = __builtin_fmaf(ww, cc[j], ars.ar[k][j]);
                            ars.wwsum[k][j] += ww;
                        }
                    }
                }
            }
        }

        // color = scale / wsum * color                               sampling.c:897
        const float norm = s.scale / wsum;
        float4_t out;
        float *o[4] = { &out.x, &out.y, &out.z, &out.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float v = norm * col[k];
            if (USE_AR && (MASK & (1u << k))) {
                float lo = ars.ar[k][0] / ars.wwsum[k][0];
                const float hi = ars.ar[k][1] / ars.wwsum[k][1];
                lo = 1.0f - lo;
                float w = fminf(fmaxf(v, lo), hi);
                w = lo > hi ? (lo * 0.5f + hi * 0.5f) : w;
                v = plh_mix(v, w, s.antiring);
            }
            *o[k] = v;
        }
        if (!(MASK & 8u))
            out.w = 1.0f;

        const frag_t fc = { (float) (idx + p.frag_x0) + 0.5f, (float) (idy + p.frag_y0) + 0.5f,
                            0.0f, 0, p.out_scale[0] * ((float) idx + 0.5f),
                            p.out_scale[1] * ((float) idy + 0.5f) };
        apply_ops(out, p.ops, p.num_pre_ops, p.num_ops, fc);

        // guarded store (dispatch.c:1126-1142)
        const float gx = p.out_scale[0] * (float) idx, gy = p.out_scale[1] * (float) idy;
        if (gx < 1.0f && gy < 1.0f) {
            const int oxp = p.base_x + p.dir_x * (p.transpose ? idy : idx);
            const int oyp = p.base_y + p.dir_y * (p.transpose ? idx : idy);
            if (oxp >= 0 && oyp >= 0 && oxp < p.dst.w && oyp < p.dst.h)
                plh_store(p.dst, oxp, oyp, out);
        }
    }
}


/* ------------------------------------------------------------------------------------
 * Phase-class formulation (struct plh_polar_pp, plh_device.h)
 *
 * The per-pixel path above spends ~35 VALU instructions per tap on the weight
 * (IEEE sqrt, LUT address, lerp) and 5 on the accumulation, which makes it
 * ALU-bound at ~3 % of the HBM roofline. But the weight of a tap is a pure
 * function of fcoord, fcoord.x only depends on the output column and fcoord.y
 * on the row, and only a few dozen distinct fp32 values of each occur per
 * frame. So the weights are tabulated once per (class pair, tap) — by
 * k_polar_weights, with the *same* device arithmetic (polar_weight) — and the
 * frame kernel keeps only the FMAs: a lane owns an n x n block of output pixels
 * that share one base texel (n = 2 for a 2x upscale), reads each source texel of
 * the footprint once from LDS and feeds it to the n*n accumulators with weights
 * fetched from an LDS copy of the tile's slice of the table.
 *
 * Exactness: every lane still evaluates its own fcoord/base (polar_coord) and
 * compares them with the tables; a pixel that disagrees (a rounding tie in the
 * degenerate bilinear attribute interpolation) takes the per-pixel path
 * inline. Summation order, fma usage and the final `scale / wsum` are those of
 * k_polar, so results are bit-identical to it.
 */
__global__ void k_polar_classify(const plh_pass p_, float *out)
{
    const plh_pass &p = plh_kernarg_pass();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float *colfc = out;
    int *colbase = (int *) (out + p.width);
    float *rowfc = out + 2 * p.width;
    int *rowbase = (int *) (out + 2 * p.width + p.height);
    float fcx, fcy;
    int bx, by;
    if (i < p.width) {
        polar_coord(p, i, 0, fcx, fcy, bx, by);
        colfc[i] = fcx;
        colbase[i] = bx;
    }
    if (i < p.height) {
        polar_coord(p, 0, i, fcx, fcy, bx, by);
        rowfc[i] = fcy;
        rowbase[i] = by;
    }
}

__global__ void k_polar_weights(const plh_pass p_, const float *clsx, int ncx,
                                const float *clsy, int ncy, float *weights)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncx * ncy)
        return;
    const int cy = i / ncx, cx = i - cy * ncx;
    const float fcx = clsx[cx], fcy = clsy[cy];
    float *w = weights + (size_t) i * (s.num_taps + 1);
    float wsum = 0.0f;
    for (int t = 0; t < s.num_taps; t++) {
        float d;
        bool live;
        const float wt = polar_weight(s, (const float2 *) s.lut, s.taps[t], fcx, fcy, d, live);
        wsum += wt;
        w[t] = wt;
    }
    w[s.num_taps] = s.scale / wsum;     // color = scale / wsum * color, sampling.c:897
}

int plh_launch_polar_classify(plh_stream stream, const plh_pass *pass, void *out)
{
    const int n = pass->width > pass->height ? pass->width : pass->height;
    hipLaunchKernelGGL(k_polar_classify, dim3((n + 255) / 256), dim3(256), 0,
                       (hipStream_t) stream, *pass, (float *) out);
    return plh_launch_status();
}

int plh_launch_polar_weights(plh_stream stream, const plh_pass *pass, const float *clsx, int ncx,
                             const float *clsy, int ncy, float *weights)
{
    hipLaunchKernelGGL(k_polar_weights, dim3((ncx * ncy + 63) / 64), dim3(64), 0,
                       (hipStream_t) stream, *pass, clsx, ncx, clsy, ncy, weights);
    return plh_launch_status();
}

// The two candidates that live here (polar_common.hiph: the contract).
// k_polar_pp: a geometry with phase-class tables; RGB / RGBA tiles or one- and two-component planes
static bool plh_polar_pp_applies(plh_pass *pass)
{
    const uint32_t cm = pass->s.comp_mask & 0xf;
    if (!pass->s.pp || (cm != 0x7 && cm != 0xf && cm != 0x1 && cm != 0x3))
        return false;
    // (the kernel has a CHAIN variant for RGB / RGBA tiles, k_polar_pp.hiph)
    if (cm == 0x7 || cm == 0xf)
        plh_match_map_chain(pass);
    if (!pass->chain.enabled)
        plh_match_fast_epilogue(pass);
    return true;
}

static int plh_launch_polar_pp(hipStream_t stream, const plh_pass *pass)
{
    const plh_sampler_args &s = pass->s;
    const int cth = POLAR_BH * s.tile_rows;
    const dim3 grid((s.pp_cells_w + POLAR_BW - 1) / POLAR_BW, (s.pp_cells_h + cth - 1) / cth);
    const dim3 block(POLAR_BW, POLAR_BH);
    const size_t px = s.tile_fp32 ? sizeof(float4) : sizeof(uint2);
    const size_t shmem = PP_LDS_FIXED + s.pp_lds_weights + (size_t) s.tile_w * s.tile_h * px;
    // (not reached: polar_tables.c sizes the tile and the weights' slice to 64 KiB together -- its
    // `max_lds` loop -- or builds no tables, and then s.pp is NULL)
    if (shmem > 160 * 1024)
        return -1000;
    const bool planes = (s.comp_mask & 0xf) == 0x1 || (s.comp_mask & 0xf) == 0x3;
    if (s.tile_fp32)
        return planes ? plh_launch_polar_pp_f32_c12(stream, pass, grid, block, shmem, s.pp_n)
                      : plh_launch_polar_pp_f32(stream, pass, grid, block, shmem, s.pp_n);
    return planes ? plh_launch_polar_pp_f16_c12(stream, pass, grid, block, shmem, s.pp_n)
                  : plh_launch_polar_pp_f16(stream, pass, grid, block, shmem, s.pp_n);
}

// k_polar: per-pixel weights, the recorded ops interpreted -- any polar pass

// k_polar's instance for the tile's texels T, the component mask and anti-ringing
template <typename T>
static plh_pass_launch_fn *px_instance(const plh_pass *pass)
{
#define PX(MASK) return pass->s.antiring > 0.0f ? plh_launch_last_lds<k_polar<T, MASK, true>> \
                                                : plh_launch_last_lds<k_polar<T, MASK, false>>
    switch (pass->s.comp_mask & 0xf) {
    case 0x1: PX(0x1);
    case 0x3: PX(0x3);
    case 0x7: PX(0x7);
    default:  PX(0xf);
    }
#undef PX
}

static int plh_launch_polar_px(hipStream_t stream, const plh_pass *pass)
{
    const plh_sampler_args &s = pass->s;
    const int th = POLAR_BH * s.tile_rows;
    const dim3 grid((pass->width + POLAR_BW - 1) / POLAR_BW, (pass->height + th - 1) / th);
    const size_t px = s.tile_fp32 ? sizeof(float4) : sizeof(uint2);
    const size_t shmem = 256 * sizeof(float2) + (size_t) s.tile_w * s.tile_h * px;
    // (not reached: pl_shader_sample_polar, shader_sampling.c, plans the band walk for a pass whose
    // tile -- this sum -- is above 160 KiB. It does size tiles of steep downscales above 64 KiB:
    // plh_launch_last_lds asks)
    if (shmem > 160 * 1024)
        return -1000;
    plh_pass_launch_fn *launch = s.tile_fp32 ? px_instance<float>(pass) : px_instance<__half>(pass);
    return launch(grid, dim3(POLAR_BW, POLAR_BH), shmem, stream, *pass);
}

// The kernels for a polar pass, in the order they are tried; each on a copy of the pass of its own
int plh_launch_polar(hipStream_t stream, const plh_pass *pass)
{
    static const plh_candidate candidates[] = {
        { "k_polar_mxd", plh_polar_mxd_applies, plh_launch_polar_mxd },   // matrix pipe: the 2 : 1 downscale
        { "k_polar_mxr", plh_polar_mxr_applies, plh_launch_polar_mxr },   // ... the 3x, 4x, 3 : 2 upscales
        { "k_polar_mxp", plh_polar_mxp_applies, plh_launch_polar_mxp },   // ... the 2x upscale, persistent, commonest op shapes
        { "k_polar_mx",  plh_polar_mx_applies,  plh_launch_polar_mx },    // ... the 2x upscale, every op shape
        { "k_polar_pp",  plh_polar_pp_applies,  plh_launch_polar_pp },    // phase classes: every geometry with tables
        { "k_polar_band", plh_polar_band_applies, plh_launch_polar_band }, // a pass with a band plan: no whole tile fits
        { "k_polar",     plh_applies_always,    plh_launch_polar_px },    // every other pass
    };
    return plh_launch_first(candidates, stream, pass);
}
