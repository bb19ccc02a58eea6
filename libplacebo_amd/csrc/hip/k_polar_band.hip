/*
 * libplacebo-hip — polar (EWA) resampling with a footprint that is never resident as a whole.
 *
 * The contract of k_polar (k_polar.hip: fcoord, the tap list with its flags, the weight from the
 * LUT pairs, the accumulators of one pixel in ONE lane in the list's order, scale / wsum, the
 * anti-ringing clamp, the post-ops and the guarded store), for the downscales whose whole footprint
 * k_polar cannot stage: at 6x the filter reaches 19 texels each way and a 32 x 8 output tile reads
 * 232 x 88 source texels.
 *
 * The tap list is ordered by rows. The host emits it from a loop over y = 1 - bound .. bound, and
 * the taps of one turn lie on rows y and y + 1 (gather order: a 2 x 2 quad, sampling.c:798-893) or
 * on row y alone (compute order, :776-783). So while the list is walked the rows in use only move
 * up, one per turn, and a workgroup keeps, per turn, only the source rows some lane needs:
 *
 *   v = (lane's base row - lowest base row of the tile) + (tap row + bound - 1)     "virtual row"
 *   turn t reads v in [t, t + span], span = number of base rows the tile's lanes can have
 *
 * in an LDS ring of span + 2 rows (slot = v mod rows). During turn t the one new row of turn t + 1
 * (v = t + span + 1) is written over the slot of v = t - 1, which no lane has read since the
 * barrier that ended turn t - 1; ONE barrier per turn publishes it. A ring row is as wide as
 * k_polar's tile (the columns are all resident), which is what sizes the ring: 32 outputs at 6x
 * with 19 texels of support each way are 232 texels. The host narrows the output tile until ring
 * and LUT fit the LDS (polar_band_plan, shader_sampling.c: 32 x 8 lanes down to 16 x 1 at 16x).
 *
 * No pre-ops: a fused "PASS A" would have to run once per staged texel AND per visit of the ring;
 * the host records none for a pass with a band plan (shader_sampling.c).
 */
#include "polar_common.hiph"

// One output pixel of k_polar_band, statement for statement what k_polar's loop body does (that
// kernel keeps its own copy: moving it here changed its instruction schedule, and its code is
// pinned): the accumulators of polar_sample (sampling.c:503-558), fed one tap at a time in the tap
// list's order by ONE lane, and what follows the taps (sampling.c:897-910, then the recorded
// post-ops and the guarded store).
template <bool USE_AR>
struct polar_acc {
    float col[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float wsum = 0.0f;
    float ar[4][2], wwsum[4][2];

    DEV polar_acc()
    {
        if (USE_AR) {
            for (int c = 0; c < 4; c++)
                ar[c][0] = ar[c][1] = wwsum[c][0] = wwsum[c][1] = 0.0f;
        }
    }
};

// tap with weight `w` (polar_weight: d, live) and flags `fl` on texel `c`
template <uint32_t MASK, bool USE_AR>
DEV void polar_acc_tap(const plh_sampler_args &s, polar_acc<USE_AR> &a, uint32_t fl, float w, float d,
                       bool live, const float4_t &c)
{
    a.wsum += w;
    const float cv[4] = { c.x, c.y, c.z, c.w };
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (MASK & (1u << k))
            a.col[k] = __builtin_fmaf(w, cv[k], a.col[k]);
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
                    a.ar[k][j] = __builtin_fmaf(ww, cc[j], a.ar[k][j]);
                    a.wwsum[k][j] += ww;
                }
            }
        }
    }
}

// behind the last tap of output pixel (idx, idy): normalise, anti-ringing clamp, post-ops, store
template <uint32_t MASK, bool USE_AR>
DEV void polar_acc_store(const plh_pass &p, const polar_acc<USE_AR> &a, int idx, int idy)
{
    const plh_sampler_args &s = p.s;
    // color = scale / wsum * color                               sampling.c:897
    const float norm = s.scale / a.wsum;
    float4_t out;
    float *o[4] = { &out.x, &out.y, &out.z, &out.w };
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = norm * a.col[k];
        if (USE_AR && (MASK & (1u << k))) {
            float lo = a.ar[k][0] / a.wwsum[k][0];
            const float hi = a.ar[k][1] / a.wwsum[k][1];
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

// rows [v0, v0 + n) of the tile's virtual footprint into their ring slots
template <typename T>
DEV void band_stage(const plh_sampler_args &s, tile_px<T> *ring, int ox, int oy, int v0, int n,
                    int vmax, int tid, int nthreads, bool raw16)
{
    const int tw = s.band_w, rows = s.band_rows;
    const float rcp_tw = 1.0f / (float) tw;
    for (int i = tid; i < tw * n; i += nthreads) {
        const int ty = (int) (((float) i + 0.5f) * rcp_tw), tx = i - ty * tw;   // exact: i < 2^22
        const int v = v0 + ty;
        if (v >= vmax)
            break;      // (beyond the last row any tap reads)
        tile_px<T> *dst = ring + (v % rows) * tw + tx;
        const int sx = plh_wrap(ox + tx, s.src.w, s.address_mode);
        const int sy = plh_wrap(oy + v, s.src.h, s.address_mode);
        if (raw16) {
            *(uint2 *) dst = *(const uint2 *) ((const char *) s.src.ptr +
                                               (size_t) sy * s.src.pitch + (size_t) sx * 8);
            continue;
        }
        tile_put(*dst, plh_fetch(s.src, sx, sy));
    }
}

template <typename T, uint32_t MASK, bool USE_AR>
__global__ __launch_bounds__(POLAR_BW * POLAR_BH)
void k_polar_band(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *lut = (float2 *) smem;                              // 256 pairs = 2 KiB
    tile_px<T> *ring = (tile_px<T> *) (smem + 256 * sizeof(float2));

    const plh_sampler_args &s = p.s;
    const int bw = s.band_out_w, bh = s.band_out_h, nthreads = bw * bh;     // = blockDim
    const int tid = threadIdx.y * bw + threadIdx.x;
    const float sw = (float) s.src.w, sh = (float) s.src.h;
    const int tw = s.band_w, rows = s.band_rows, span = rows - 2;
    const int vmax = span + 2 * s.bound - 1;    // virtual rows in all: k_polar's tile height

    // ---- workgroup footprint: base texel of the four corner lanes, as k_polar ----------------
    const int gx0 = blockIdx.x * bw, gy0 = blockIdx.y * bh;
    int ox, oy;     // source texel of ring column 0 / of virtual row 0
    {
        int bx[2], by[2];
        for (int k = 0; k < 2; k++) {
            const float mx = p.out_scale[0] * ((float) (gx0 + k * (bw - 1)) + 0.5f);
            const float my = p.out_scale[1] * ((float) (gy0 + k * (bh - 1)) + 0.5f);
            const float cx = plh_attr(s.pos, 0, mx, p.out_scale[1] * ((float) gy0 + 0.5f));
            const float cy = plh_attr(s.pos, 1, p.out_scale[0] * ((float) gx0 + 0.5f), my);
            bx[k] = (int) __builtin_floorf(cx * sw - 0.5f);
            by[k] = (int) __builtin_floorf(cy * sh - 0.5f);
        }
        // one texel of slack on the low side, one on the high side (the host's + 2)
        const int off = s.bound - 1;
        ox = min(bx[0], bx[1]) - off - 1;
        oy = min(by[0], by[1]) - off - 1;
    }

    // ---- LUT pairs + the rows of turn 0 -----------------------------------------------------
    for (int i = tid; i < 256; i += nthreads)
        lut[i] = ((const float2 *) s.lut)[i];
    const bool raw16 = sizeof(tile_px<T>) == 8 && s.src.fmt == PLH_FMT_RGBA16F;
    band_stage<T>(s, ring, ox, oy, 0, span + 1, vmax, tid, nthreads, raw16);
    __syncthreads();

    // ---- this lane's pixel ------------------------------------------------------------------
    const int idx = gx0 + threadIdx.x, idy = gy0 + threadIdx.y;
    float fcx, fcy;
    int relx, rely;
    {
        const float mx = p.out_scale[0] * ((float) idx + 0.5f);
        const float my = p.out_scale[1] * ((float) idy + 0.5f);
        const float px = plh_attr(s.pos, 0, mx, my);
        const float py = plh_attr(s.pos, 1, mx, my);
        const float tx = px * sw - 0.5f, ty = py * sh - 0.5f;
        const float flx = __builtin_floorf(tx), fly = __builtin_floorf(ty);
        fcx = tx - flx;
        fcy = ty - fly;
        // ring column of tap (0, 0) and base row above the tile's lowest; lanes outside the image
        // (padding lanes of edge groups) are clamped so their LDS reads stay in range
        relx = min(max((int) flx - ox, s.bound - 1), tw - s.bound - 1);
        rely = min(max((int) fly - oy - (s.bound - 1), 0), span - 1);
    }
    const tile_px<T> *tp = ring + relx;

    polar_acc<USE_AR> acc;
    int t = 0, slot0 = 0;
#pragma unroll 1
    for (int turn = 0; turn < 2 * s.bound; turn++) {
        // the new row of the next turn, over the slot the last turn has left
        if (turn + 1 < 2 * s.bound)
            band_stage<T>(s, ring, ox, oy, turn + span + 1, 1, vmax, tid, nthreads, raw16);

        // the taps of rows y0, y0 + 1: virtual rows turn + rely (+ 1), slot = v mod rows
        const int y0 = 1 - s.bound + turn;
        for (; t < s.num_taps; t++) {
            const uint32_t tap = s.taps[t];
            const int x = (int8_t) (tap & 0xff), y = (int8_t) ((tap >> 8) & 0xff);
            if (y > y0 + 1)
                break;
            const uint32_t fl = tap >> 16;

            float d;
            bool live;
            const float w = polar_weight(s, lut, tap, fcx, fcy, d, live);

            int slot = slot0 + (y - y0) + rely;
            slot = slot >= rows ? slot - rows : slot;
            polar_acc_tap<MASK, USE_AR>(s, acc, fl, w, d, live, tile_get(tp[slot * tw + x]));
        }
        slot0 = slot0 + 1 == rows ? 0 : slot0 + 1;
        __syncthreads();
    }

    polar_acc_store<MASK, USE_AR>(p, acc, idx, idy);
}

// k_polar_band's instance for the ring's texels T, the component mask and anti-ringing
template <typename T>
static plh_pass_launch_fn *band_instance(const plh_pass *pass)
{
#define BAND(MASK) return pass->s.antiring > 0.0f ? plh_launch_last_lds<k_polar_band<T, MASK, true>> \
                                                  : plh_launch_last_lds<k_polar_band<T, MASK, false>>
    switch (pass->s.comp_mask & 0xf) {
    case 0x1: BAND(0x1);
    case 0x3: BAND(0x3);
    case 0x7: BAND(0x7);
    default:  BAND(0xf);
    }
#undef BAND
}

// a pass that carries a band plan (pl_shader_sample_polar: nothing else fits, or PL_HIP_POLAR_BAND)
bool plh_polar_band_applies(plh_pass *pass)
{
    return pass->s.band_rows > 0 && !pass->num_pre_ops;
}

int plh_launch_polar_band(hipStream_t stream, const plh_pass *pass)
{
    const plh_sampler_args &s = pass->s;
    const dim3 grid((pass->width + s.band_out_w - 1) / s.band_out_w,
                    (pass->height + s.band_out_h - 1) / s.band_out_h);
    const size_t px = s.tile_fp32 ? sizeof(float4) : sizeof(uint2);
    const size_t shmem = 256 * sizeof(float2) + (size_t) s.band_w * s.band_rows * px;
    plh_pass_launch_fn *launch = s.tile_fp32 ? band_instance<float>(pass) : band_instance<__half>(pass);
    return launch(grid, dim3(s.band_out_w, s.band_out_h), shmem, stream, *pass);
}
