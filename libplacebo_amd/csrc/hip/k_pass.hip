/*
 * libplacebo-hip — generic fused pass kernel (K1, K5, K7-K9, K13, K15, K16).
 *
 * One launch = one reference pass for every sampler that needs no workgroup
 * cooperation: direct/nearest/bilinear (sampling.c:277-316), the fast
 * bicubic/hermite/gaussian/oversample samplers (:318-471), or no sampler at
 * all. The sampled colour then runs through the recorded colour-op chain and
 * is stored with the target format's conversion.
 *
 * Memory-bound: every source texel and every target texel crosses HBM once.
 */
#include <stdio.h>

#include <string.h>
#include "colorops.hiph"
#include "backend.h"
#include "samplers.hiph"
#include "fastepi.hiph"
#include "launch_ladder.hiph"

#include "k_pass_generic.hiph"


/* ------------------------------------------------------------------------ */
/*
 * k_bilinear_fast: the renderer's commonest final pass as one small kernel --
 * bilinear sample of an 8-byte texel source (rgba16 / rgba16hf), the fused epilogue
 * (fastepi.hiph: [dither] [uniform scale]) and an rgba16 store. Same arithmetic as
 * k_pass_generic's BILINEAR case + apply_ops_n (bit-identical; tests/test_gpu_renderer.py
 * runs both), without the op interpreter: ~1/2 of the instructions and of the registers.
 *
 * A lane owns ITERS 2x2 output cells, BF_BH cell rows apart, software-pipelined: the four
 * texel loads (and the dither fetches) of cell k+1 are in flight while cell k is blended,
 * encoded and stored. The attribute interpolation is split into its per-column halves
 * (computed once per lane) and the per-pixel fy blend -- the same fma sequence as plh_attr.
 */
#define BF_BW 64
#define BF_BH 4

// The kernels below pin their uniforms in SGPRs with an empty asm; a pointer that went through
// one is a generic pointer to the compiler afterwards, and every access through it a flat_
// instruction (which also ties up the LDS counter). These are device allocations: say so.
#define BF_GLOBAL __attribute__((address_space(1)))

DEV uint2 bf_load(const char *base, int pitch, int x, int y)
{
    const BF_GLOBAL char *g = (const BF_GLOBAL char *) (uintptr_t) base;
    const plh_u32x2 v = *(const BF_GLOBAL plh_u32x2 *) (g + (size_t) y * pitch + (size_t) x * 8);
    return make_uint2(v.x, v.y);
}

DEV float bf_bias(const float *matrix, int i)
{
    return ((const BF_GLOBAL float *) (uintptr_t) matrix)[i];
}

template <bool F16SRC>
DEV float4_t bf_decode(const uint2 v)
{
    float4_t c;
    if (F16SRC) {
        c = { plh_h2f(v.x & 0xffff), plh_h2f(v.x >> 16), plh_h2f(v.y & 0xffff), plh_h2f(v.y >> 16) };
    } else {
        c = { plh_un16(v.x & 0xffff), plh_un16(v.x >> 16), plh_un16(v.y & 0xffff), plh_un16(v.y >> 16) };
    }
    return c;
}

struct bf_cell {
    uint2 raw[4];       // the shared 2x2 footprint: (x0,y0) (x1,y0) (x0,y1) (x1,y1)
    float ax[4], ay[4]; // blend factors of the cell's four pixels
    float bias[4];      // dither matrix values
    int idy0;
    bool shared;
};

// RGB: the epilogue overwrites alpha (p.epi.has_alpha: video without an alpha plane), so the
// fourth channel is neither decoded nor blended.
template <bool F16SRC, int ITERS, bool RGB>
__global__ __launch_bounds__(BF_BW * BF_BH)
void k_bilinear_fast(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    const int cx = blockIdx.x * BF_BW + threadIdx.x;
    const int idx0 = 2 * cx - p.cell_padx;
    const float sw = (float) s.src.w, sh = (float) s.src.h;
    // Uniforms used under control flow, pinned in SGPRs: left alone the compiler re-loads them
    // from the kernel arguments at every use, each load followed by a full scalar wait.
    const char *sp = (const char *) s.src.ptr;
    const float *dmat = p.epi.matrix;
    int spitch = s.src.pitch, srcw = s.src.w, srch = s.src.h;
    int dmask = p.epi.mask, dsize = p.epi.size, has_dither = p.epi.has_dither;
    int fx0 = p.frag_x0, fy0 = p.frag_y0;
    asm volatile("" : "+s"(sp), "+s"(dmat), "+s"(spitch), "+s"(srcw), "+s"(srch), "+s"(dmask),
                      "+s"(dsize), "+s"(has_dither), "+s"(fx0), "+s"(fy0));

    // per-column state: fx halves of the attributes, store guard, target column
    float a0[2], a1[2], b0[2], b1[2];
    int sx[2];
    bool cok[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int idx = idx0 + i;
        const float mx = p.out_scale[0] * ((float) idx + 0.5f);
        a0[i] = plh_mix(s.pos[0][0], s.pos[1][0], mx);
        a1[i] = plh_mix(s.pos[2][0], s.pos[3][0], mx);
        b0[i] = plh_mix(s.pos[0][1], s.pos[1][1], mx);
        b1[i] = plh_mix(s.pos[2][1], s.pos[3][1], mx);
        sx[i] = p.base_x + p.dir_x * idx;
        cok[i] = idx >= 0 && p.out_scale[0] * (float) idx < 1.0f && sx[i] >= 0 && sx[i] < p.dst.w;
    }

    // stage A: coordinates, footprint, loads
    auto stage_a = [&](int it, bf_cell &c) {
        const int cy = (blockIdx.y * ITERS + it) * BF_BH + threadIdx.y;
        c.idy0 = 2 * cy - p.cell_pady;
        float fu0 = 0.0f, fw0 = 0.0f;
        bool shared = true;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = q & 1, j = q >> 1;
            const float my = p.out_scale[1] * ((float) (c.idy0 + j) + 0.5f);
            const float px = plh_mix(a0[i], a1[i], my), py = plh_mix(b0[i], b1[i], my);
            const float u = px * sw - 0.5f, w = py * sh - 0.5f;
            const float fu = __builtin_floorf(u), fw = __builtin_floorf(w);
            c.ax[q] = u - fu;
            c.ay[q] = w - fw;
            if (q == 0) {
                fu0 = fu; fw0 = fw;
            } else {
                shared = shared && fu == fu0 && fw == fw0;
            }
            c.bias[q] = 0.0f;
            if (has_dither) {
                const int ix = (idx0 + i + fx0) & dmask;
                const int iy = (c.idy0 + j + fy0) & dmask;
                c.bias[q] = bf_bias(dmat, iy * dsize + ix);
            }
        }
        c.shared = shared;
        // (clamp addressing only; the other modes take the generic kernel)
        const int x0 = min(max((int) fu0, 0), srcw - 1), x1 = min(max((int) fu0 + 1, 0), srcw - 1);
        const int y0 = min(max((int) fw0, 0), srch - 1), y1 = min(max((int) fw0 + 1, 0), srch - 1);
        c.raw[0] = bf_load(sp, spitch, x0, y0);
        c.raw[1] = bf_load(sp, spitch, x1, y0);
        c.raw[2] = bf_load(sp, spitch, x0, y1);
        c.raw[3] = bf_load(sp, spitch, x1, y1);
    };

    // stage B: decode, blend, epilogue, store
    auto stage_b = [&](const bf_cell &c) {
        constexpr int NCH = RGB ? 3 : 4;
        float t[4][NCH];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t w[4] = { c.raw[k].x & 0xffff, c.raw[k].x >> 16, c.raw[k].y & 0xffff,
                                    c.raw[k].y >> 16 };
#pragma unroll
            for (int ch = 0; ch < NCH; ch++)
                t[k][ch] = F16SRC ? plh_h2f(w[ch]) : plh_un16(w[ch]);
        }
        float4_t o[4];
        // The blend factors are per column (ax) and per row (ay) up to the rounding of the
        // attribute interpolation; when they are -- bit for bit, checked here -- the two
        // horizontal blends of a column serve both of its pixels: 8 mixes per channel, not 12.
        const bool separable = c.ax[0] == c.ax[2] && c.ax[1] == c.ax[3] &&
                               c.ay[0] == c.ay[1] && c.ay[2] == c.ay[3];
        float ov[4][4];
        if (separable) {
#pragma unroll
            for (int ch = 0; ch < NCH; ch++) {
                float top[2], bot[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    top[i] = plh_mix(t[0][ch], t[1][ch], c.ax[i]);
                    bot[i] = plh_mix(t[2][ch], t[3][ch], c.ax[i]);
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
                    ov[q][ch] = s.scale * plh_mix(top[q & 1], bot[q & 1], c.ay[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
#pragma unroll
                for (int ch = 0; ch < NCH; ch++) {
                    ov[q][ch] = s.scale * plh_mix(plh_mix(t[0][ch], t[1][ch], c.ax[q]),
                                                  plh_mix(t[2][ch], t[3][ch], c.ax[q]), c.ay[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            o[q] = { ov[q][0], ov[q][1], ov[q][2], RGB ? 0.0f : ov[q][NCH - 1] };
        if (!c.shared) {
            // pixels of this cell straddle a texel boundary (not a 2x upscale on the cell
            // phase): every pixel fetches its own footprint
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = q & 1, j = q >> 1;
                const float my = p.out_scale[1] * ((float) (c.idy0 + j) + 0.5f);
                const float px = plh_mix(a0[i], a1[i], my), py = plh_mix(b0[i], b1[i], my);
                const lin_fp f = lin_footprint(s.src, s.address_mode, px, py);
                const uint2 r0 = bf_load(sp, spitch, f.x0, f.y0), r1 = bf_load(sp, spitch, f.x1, f.y0);
                const uint2 r2 = bf_load(sp, spitch, f.x0, f.y1), r3 = bf_load(sp, spitch, f.x1, f.y1);
                o[q] = scale4(mix4(mix4(bf_decode<F16SRC>(r0), bf_decode<F16SRC>(r1), f.ax),
                                   mix4(bf_decode<F16SRC>(r2), bf_decode<F16SRC>(r3), f.ax), f.ay),
                              s.scale);
            }
        }
        int ox[4], oy[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = q & 1, j = q >> 1;
            const int idy = c.idy0 + j;
            if (p.epi.has_alpha)
                o[q].w = p.epi.alpha;
            // op_dither (non-gamma path) and the SCALE op (colorops.hiph)
            if (p.epi.has_dither) {
                const float b = c.bias[q], ds = p.epi.dscale, di = p.epi.dinv;
                o[q].x = __builtin_floorf(ds * o[q].x + b) * di;
                o[q].y = __builtin_floorf(ds * o[q].y + b) * di;
                o[q].z = __builtin_floorf(ds * o[q].z + b) * di;
                o[q].w = __builtin_floorf(ds * o[q].w + b) * di;
            }
            if (p.epi.has_scale)
                o[q] = scale4(o[q], p.epi.scale);
            ox[q] = sx[i];
            oy[q] = p.base_y + p.dir_y * idy;
            ok[q] = cok[i] && idy >= 0 && p.out_scale[1] * (float) idy < 1.0f &&
                    oy[q] >= 0 && oy[q] < p.dst.h;
        }
        plh_store_rgba16_n<4>(p.dst, ox, oy, ok, o, p.nt_store);
    };

    if constexpr (ITERS == 1) {
        bf_cell c;
        stage_a(0, c);
        stage_b(c);
    } else {
        bf_cell c[2];
        stage_a(0, c[0]);
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            if (it + 1 < ITERS)
                stage_a(it + 1, c[(it + 1) & 1]);
            stage_b(c[it & 1]);
        }
    }
}

/*
 * k_nearest_fast: nearest-neighbour fetch of an 8-byte RGBA source + the fused epilogue
 * ([alpha] [dither] [scale] -> rgba16 store). The output pass of a single cached frame
 * (pl_render_image_mix between two source frames, frame-cache hits) and plain format
 * conversions are this pass: k_pass_generic's NEAREST case + apply_ops_n, bit-identical, without
 * the interpreter. A lane owns two adjacent pixels in NF_ROWS rows (one 16-byte store each), all
 * loads requested before the first use.
 */
#define NF_ROWS 2

template <bool F16SRC>
__global__ __launch_bounds__(BF_BW * BF_BH)
void k_nearest_fast(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    const int cx = blockIdx.x * BF_BW + threadIdx.x;
    const int idx0 = 2 * cx - p.cell_padx;
    const float sw = (float) s.src.w, sh = (float) s.src.h;
    const char *sp = (const char *) s.src.ptr;
    const float *dmat = p.epi.matrix;
    int spitch = s.src.pitch, srcw = s.src.w, srch = s.src.h;
    int dmask = p.epi.mask, dsize = p.epi.size, has_dither = p.epi.has_dither;
    int fx0 = p.frag_x0, fy0 = p.frag_y0;
    asm volatile("" : "+s"(sp), "+s"(dmat), "+s"(spitch), "+s"(srcw), "+s"(srch), "+s"(dmask),
                      "+s"(dsize), "+s"(has_dither), "+s"(fx0), "+s"(fy0));

    uint2 raw[NF_ROWS][2];
    float bias[NF_ROWS][2];
    int idys[NF_ROWS];
#pragma unroll
    for (int r = 0; r < NF_ROWS; r++) {
        const int idy = (blockIdx.y * NF_ROWS + r) * BF_BH + threadIdx.y;
        idys[r] = idy;
        const float my = p.out_scale[1] * ((float) idy + 0.5f);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int idx = idx0 + i;
            const float mx = p.out_scale[0] * ((float) idx + 0.5f);
            const float px = plh_attr(s.pos, 0, mx, my), py = plh_attr(s.pos, 1, mx, my);
            // (clamp addressing only; the other modes take the generic kernel)
            const int ix = min(max((int) __builtin_floorf(px * sw), 0), srcw - 1);
            const int iy = min(max((int) __builtin_floorf(py * sh), 0), srch - 1);
            raw[r][i] = bf_load(sp, spitch, ix, iy);
            bias[r][i] = 0.0f;
            if (has_dither)
                bias[r][i] = bf_bias(dmat, ((idy + fy0) & dmask) * dsize + ((idx + fx0) & dmask));
        }
    }

#pragma unroll
    for (int r = 0; r < NF_ROWS; r++) {
        float4_t o[2];
        int ox[2], oy[2];
        bool ok[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int idx = idx0 + i, idy = idys[r];
            o[i] = scale4(bf_decode<F16SRC>(raw[r][i]), s.scale);
            if (p.epi.has_alpha)
                o[i].w = p.epi.alpha;
            if (p.epi.has_dither) {
                const float b = bias[r][i], ds = p.epi.dscale, di = p.epi.dinv;
                o[i].x = __builtin_floorf(ds * o[i].x + b) * di;
                o[i].y = __builtin_floorf(ds * o[i].y + b) * di;
                o[i].z = __builtin_floorf(ds * o[i].z + b) * di;
                o[i].w = __builtin_floorf(ds * o[i].w + b) * di;
            }
            if (p.epi.has_scale)
                o[i] = scale4(o[i], p.epi.scale);
            ox[i] = p.base_x + p.dir_x * idx;
            oy[i] = p.base_y + p.dir_y * idy;
            ok[i] = idx >= 0 && p.out_scale[0] * (float) idx < 1.0f && ox[i] >= 0 && ox[i] < p.dst.w &&
                    idy >= 0 && p.out_scale[1] * (float) idy < 1.0f && oy[i] >= 0 && oy[i] < p.dst.h;
        }
        plh_store_rgba16_n<2>(p.dst, ox, oy, ok, o, p.nt_store);
    }
}

/* ------------------------------------------------------------------------ */
/*
 * k_pass_native: a pass that reads its source texel for texel (identity rect, nearest) -- the
 * colour-map pass behind an intermediate, a plane decode -- with the op interpreter of
 * k_pass_generic but none of its geometry: no attribute interpolation, no texel-coordinate
 * arithmetic, no format switches; a lane owns two horizontally adjacent pixels (one 16-byte
 * load, one 16-byte store). Same ops, same values: the source coordinate of output pixel
 * (x, y) IS (x, y) there (k_pass_generic computes floor(((x + 0.5) / w) * w) = x).
 */
template <bool LITE, bool F16SRC, bool F16DST>
__global__ __launch_bounds__(PASS_BW * PASS_BH)
void k_pass_native(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    const int cx = blockIdx.x * PASS_BW + threadIdx.x;
    const int w = p.width, h = p.height;
    const int x0 = 2 * cx;
#pragma unroll 1
    for (int it = 0; it < PASS_ITERS; it++) {
        const int y = (blockIdx.y * PASS_ITERS + it) * PASS_BH + threadIdx.y;
        if (x0 >= w || y >= h)
            continue;
        const bool two = x0 + 1 < w;
        const char *row = (const char *) s.src.ptr + (size_t) y * s.src.pitch + (size_t) x0 * 8;
        uint4 v;
        if (two) {
            v = *(const uint4 *) row;
        } else {
            const uint2 e = *(const uint2 *) row;
            v = make_uint4(e.x, e.y, e.x, e.y);
        }
        float4_t c[2];
        frag_t fcs[2];
        const uint32_t q[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t lo = q[2 * i], hi = q[2 * i + 1];
            if (F16SRC)
                c[i] = { plh_h2f(lo & 0xffff), plh_h2f(lo >> 16), plh_h2f(hi & 0xffff), plh_h2f(hi >> 16) };
            else
                c[i] = { plh_un16(lo & 0xffff), plh_un16(lo >> 16), plh_un16(hi & 0xffff), plh_un16(hi >> 16) };
            if (s.scale != 1.0f)
                c[i] = scale4(c[i], s.scale);
            const int idx = x0 + i;
            fcs[i] = { (float) (idx + p.frag_x0) + 0.5f, (float) (y + p.frag_y0) + 0.5f, 0.0f, 0,
                       p.out_scale[0] * ((float) idx + 0.5f), p.out_scale[1] * ((float) y + 0.5f) };
        }
        apply_ops_n<2, false, LITE>(c, p.ops, 0, p.num_ops, fcs);
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (F16DST) {
                o[2 * i] = (uint32_t) plh_f2h(c[i].x) | ((uint32_t) plh_f2h(c[i].y) << 16);
                o[2 * i + 1] = (uint32_t) plh_f2h(c[i].z) | ((uint32_t) plh_f2h(c[i].w) << 16);
            } else {
                o[2 * i] = plh_unorm16x2(c[i].x, c[i].y);
                o[2 * i + 1] = plh_unorm16x2(c[i].z, c[i].w);
            }
        }
        char *d = (char *) p.dst.ptr + (size_t) y * p.dst.pitch + (size_t) x0 * 8;
        if (two) {
            const plh_u32x4 pk = { o[0], o[1], o[2], o[3] };
            // (an rgba16 target is a final frame: streamed; an rgba16hf one is the intermediate the next
            // pass reads: cached. At compile time: `if (nt) non-temporal else plain` is folded into one
            // plain store, devmath.hiph)
            if constexpr (F16DST)
                *(plh_u32x4 *) d = pk;
            else
                __builtin_nontemporal_store(pk, (plh_u32x4 *) d);
        } else {
            *(uint2 *) d = make_uint2(o[0], o[1]);
        }
    }
}

/*
 * k_pass_chain: k_pass_native for the one op list an HDR map pass records (struct plh_map_chain,
 * plh_device.h) behind an rgba16 target -- no interpreter at all: decode, the chain's device
 * functions, the fused epilogue (op_dither's plain path and the SCALE op, fastepi.hiph), store.
 * Bit-identical to k_pass_native / k_pass_generic on such a pass; NP pixels per lane.
 */
#ifndef CHAIN_NP
#define CHAIN_NP 1      // (one pixel per lane: 101.5 us against 104.0 with two on configs[3]'s map pass)
#endif
template <bool F16SRC, int NP, bool CR, bool F16DST = false>
__global__ __launch_bounds__(PASS_BW * PASS_BH)
void k_pass_chain(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    const int x0 = NP * (blockIdx.x * PASS_BW + threadIdx.x);
    const int y = blockIdx.y * PASS_BH + threadIdx.y;
    const int w = p.width, h = p.height;
    // (final frames) the tone curve's table in LDS: the launcher asks for the room when the chain has
    // a tone op with a table of at most PQSEG_TONE_MAX entries -- one gather per pixel less on the
    // texture path, which is what bounds this pass (TD busy 84 % under the gamut LUT's four
    // gathers). Same entries, same blend: same bits.
    extern __shared__ __attribute__((aligned(16))) unsigned char chain_smem[];
    pq_seg seg = pq_seg_view(chain_smem, 0, 0, false);     // (no PQ pieces here: the closed forms)
    if constexpr (!F16DST) {
        int tone_n = p.chain.tone_lds;
        asm volatile("" : "+s"(tone_n));
        if (tone_n) {
            typedef __attribute__((address_space(1))) const float gfl;
            gfl *g = (gfl *) (uintptr_t) p.ops[p.chain.tone].ptr;
            for (int i = threadIdx.y * PASS_BW + threadIdx.x; i < tone_n; i += PASS_BW * PASS_BH)
                ((float *) chain_smem)[i] = g[i];
            __syncthreads();
            seg.tone = (const float *) chain_smem;
        }
    }
    if (x0 >= w || y >= h)
        return;
    const bool all = x0 + NP - 1 < w;
    const char *row = (const char *) s.src.ptr + (size_t) y * s.src.pitch + (size_t) x0 * 8;
    uint32_t q[2 * NP];
    if (NP == 2 && all) {
        const uint4 v = *(const uint4 *) row;
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    } else {
        const uint2 e = *(const uint2 *) row;
#pragma unroll
        for (int i = 0; i < NP; i++) {
            q[2 * i] = e.x;
            q[2 * i + 1] = e.y;
        }
    }
    // the dither values, asked for before the arithmetic that hides their latency
    const plh_fast_epi &e = p.epi;
    float bias[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int ix = (x0 + i + p.frag_x0) & e.mask, iy = (y + p.frag_y0) & e.mask;
        bias[i] = e.has_dither ? e.matrix[iy * e.size + ix] : 0.0f;
    }
    float4_t c[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const uint32_t lo = q[2 * i], hi = q[2 * i + 1];
        if (F16SRC)
            c[i] = { plh_h2f(lo & 0xffff), plh_h2f(lo >> 16), plh_h2f(hi & 0xffff), plh_h2f(hi >> 16) };
        else
            c[i] = { plh_un16(lo & 0xffff), plh_un16(lo >> 16), plh_un16(hi & 0xffff), plh_un16(hi >> 16) };
        if (s.scale != 1.0f)
            c[i] = scale4(c[i], s.scale);
    }
    float pos[NP][2];
    if (CR) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            pos[i][0] = p.out_scale[0] * ((float) (x0 + i) + 0.5f);
            pos[i][1] = p.out_scale[1] * ((float) y + 0.5f);
        }
    }
    if constexpr (F16DST)
        run_map_chain<NP, CR>(c, p, pos);
    else
        run_map_chain<NP, CR, true, true>(c, p, pos, &seg);     // (seg.on == false: only the tone table)
    uint32_t o[2 * NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if (F16DST) {
            // an rgba16hf intermediate: no epilogue (plh_match_map_chain)
            o[2 * i] = (uint32_t) plh_f2h(c[i].x) | ((uint32_t) plh_f2h(c[i].y) << 16);
            o[2 * i + 1] = (uint32_t) plh_f2h(c[i].z) | ((uint32_t) plh_f2h(c[i].w) << 16);
            continue;
        }
        if (e.has_dither) {
            const float b = bias[i], ds = e.dscale, di = e.dinv;
            c[i] = { __builtin_floorf(ds * c[i].x + b) * di, __builtin_floorf(ds * c[i].y + b) * di,
                     __builtin_floorf(ds * c[i].z + b) * di, __builtin_floorf(ds * c[i].w + b) * di };
        }
        if (e.has_scale)
            c[i] = scale4(c[i], e.scale);
        o[2 * i] = plh_unorm16x2(c[i].x, c[i].y);
        o[2 * i + 1] = plh_unorm16x2(c[i].z, c[i].w);
    }
    char *d = (char *) p.dst.ptr + (size_t) y * p.dst.pitch + (size_t) x0 * 8;
    if (NP == 2 && all) {
        const plh_u32x4 pk = { o[0], o[1], o[2], o[3] };
        // (an rgba16 target is a final frame: streamed; an rgba16hf one is the intermediate the next
        // pass reads: cached. At compile time: `if (nt) non-temporal else plain` is folded into one
        // plain store, devmath.hiph)
        if constexpr (F16DST)
            *(plh_u32x4 *) d = pk;
        else
            __builtin_nontemporal_store(pk, (plh_u32x4 *) d);
    } else {
        const plh_u32x2 one = { o[0], o[1] };
        if constexpr (F16DST)
            *(plh_u32x2 *) d = one;
        else
            __builtin_nontemporal_store(one, (plh_u32x2 *) d);
    }
}

/*
 * k_pass_features: pl_shader_extract_features as its own pass (renderer.c:1404-1440: the
 * contrast-recovery feature map, one FEATURES op from the linear-light intermediate into an r16hf
 * plane) without the interpreter: two pixels per lane, 16 bytes in, 4 bytes out. op_features
 * itself, so bit-identical to k_pass_generic.
 */
template <bool F16SRC>
__global__ __launch_bounds__(PASS_BW * PASS_BH)
void k_pass_features(const plh_pass p_)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    const int x0 = 2 * (blockIdx.x * PASS_BW + threadIdx.x);
    const int y = blockIdx.y * PASS_BH + threadIdx.y;
    if (x0 >= p.width || y >= p.height)
        return;
    const bool two = x0 + 1 < p.width;
    const char *row = (const char *) s.src.ptr + (size_t) y * s.src.pitch + (size_t) x0 * 8;
    uint32_t q[4];
    if (two) {
        const uint4 v = *(const uint4 *) row;
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    } else {
        const uint2 e = *(const uint2 *) row;
        q[0] = q[2] = e.x; q[1] = q[3] = e.y;
    }
    uint32_t o[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t lo = q[2 * i], hi = q[2 * i + 1];
        float4_t c;
        if (F16SRC)
            c = { plh_h2f(lo & 0xffff), plh_h2f(lo >> 16), plh_h2f(hi & 0xffff), plh_h2f(hi >> 16) };
        else
            c = { plh_un16(lo & 0xffff), plh_un16(lo >> 16), plh_un16(hi & 0xffff), plh_un16(hi >> 16) };
        if (s.scale != 1.0f)
            c = scale4(c, s.scale);
        op_features(c, p.ops[0]);
        o[i] = plh_f2h(c.x);
    }
    char *d = (char *) p.dst.ptr + (size_t) y * p.dst.pitch + (size_t) x0 * 2;
    if (two)
        *(uint32_t *) d = o[0] | (o[1] << 16);
    else
        *(uint16_t *) d = (uint16_t) o[0];
}

/*
 * k_pass_merge: the pass that assembles a planar frame (renderer.c:1874-1920: the reference plane
 * sampled texel for texel, the other planes -- already scaled to its size -- fetched at the same
 * position, YCbCr -> RGB, and whatever colour management follows) without the interpreter:
 *   PLANE_MAP, one or two PLANE_FETCH, [AFFINE], [the map chain], then the fused epilogue into
 *   rgba16 or a plain store into an rgba16hf intermediate.
 * The device functions of the interpreter's cases, in its order: bit-identical. Any source format
 * (plh_fetch); two horizontally adjacent pixels per lane.
 */
struct plh_merge { int32_t pmap, fetch0, fetch1, affine; };

template <bool F16DST>
__global__ __launch_bounds__(PASS_BW * PASS_BH)
void k_pass_merge(const plh_pass p_, const plh_merge m)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    constexpr int NP = 2;
    const int x0 = NP * (blockIdx.x * PASS_BW + threadIdx.x);
    const int y = blockIdx.y * PASS_BH + threadIdx.y;
    if (x0 >= p.width || y >= p.height)
        return;
    const bool all = x0 + 1 < p.width;
    const plh_fast_epi &e = p.epi;
    float bias[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int ix = (x0 + i + p.frag_x0) & e.mask, iy = (y + p.frag_y0) & e.mask;
        bias[i] = !F16DST && e.has_dither ? e.matrix[iy * e.size + ix] : 0.0f;
    }
    float4_t c[NP];
    const float my = p.out_scale[1] * ((float) y + 0.5f);
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int x = all ? x0 + i : x0;
        c[i] = plh_fetch(s.src, x, y);
        if (s.scale != 1.0f)
            c[i] = scale4(c[i], s.scale);
        const float mx = p.out_scale[0] * ((float) x + 0.5f);
        if (m.pmap >= 0)
            op_plane_map(c[i], p.ops[m.pmap]);
        op_plane_fetch(c[i], p.ops[m.fetch0], mx, my);
        if (m.fetch1 >= 0)
            op_plane_fetch(c[i], p.ops[m.fetch1], mx, my);
        if (m.affine >= 0)
            op_affine(c[i], p.ops[m.affine].f);
    }
    if (p.chain.enabled)
        run_map_chain<NP>(c, p);
    uint32_t o[2 * NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if (F16DST) {
            o[2 * i] = (uint32_t) plh_f2h(c[i].x) | ((uint32_t) plh_f2h(c[i].y) << 16);
            o[2 * i + 1] = (uint32_t) plh_f2h(c[i].z) | ((uint32_t) plh_f2h(c[i].w) << 16);
            continue;
        }
        if (e.has_dither) {
            const float b = bias[i], ds = e.dscale, di = e.dinv;
            c[i] = { __builtin_floorf(ds * c[i].x + b) * di, __builtin_floorf(ds * c[i].y + b) * di,
                     __builtin_floorf(ds * c[i].z + b) * di, __builtin_floorf(ds * c[i].w + b) * di };
        }
        if (e.has_scale)
            c[i] = scale4(c[i], e.scale);
        o[2 * i] = plh_unorm16x2(c[i].x, c[i].y);
        o[2 * i + 1] = plh_unorm16x2(c[i].z, c[i].w);
    }
    char *d = (char *) p.dst.ptr + (size_t) y * p.dst.pitch + (size_t) x0 * 8;
    if (all) {
        const plh_u32x4 pk = { o[0], o[1], o[2], o[3] };
        // (an rgba16 target is a final frame: streamed; an rgba16hf one is the intermediate the next
        // pass reads: cached. At compile time: `if (nt) non-temporal else plain` is folded into one
        // plain store, devmath.hiph)
        if constexpr (F16DST)
            *(plh_u32x4 *) d = pk;
        else
            __builtin_nontemporal_store(pk, (plh_u32x4 *) d);
    } else {
        const plh_u32x2 one = { o[0], o[1] };
        if constexpr (F16DST)
            *(plh_u32x2 *) d = one;
        else
            __builtin_nontemporal_store(one, (plh_u32x2 *) d);
    }
}

// The head of the merge pass k_pass_merge is written for, as `m`: the index of the first op behind
// it, or -1 where the pass is none (k_pass_merge's plan: its test and its launch both ask here)
static int pass_merge_plan(const plh_pass *pass, plh_merge *m)
{
    const plh_sampler_args &s = pass->s;
    if (!plh_switch(PLH_SW_PASS_NATIVE))
        return -1;
    if (!plh_pass_covers_source(pass) || s.type != PLH_SAMPLE_NEAREST ||
        s.address_mode != PLH_ADDRESS_CLAMP || pass->transpose || pass->num_pre_ops ||
        !plh_pass_plain_target(pass) ||
        (pass->dst.fmt != PLH_FMT_RGBA16 && pass->dst.fmt != PLH_FMT_RGBA16F))
        return -1;
    const int n = pass->num_ops;
    int i = 0;
    *m = plh_merge{ -1, -1, -1, -1 };
    if (i < n && pass->ops[i].kind == PLH_OP_PLANE_MAP)
        m->pmap = i++;
    if (!(i < n && pass->ops[i].kind == PLH_OP_PLANE_FETCH))
        return -1;
    m->fetch0 = i++;
    if (i < n && pass->ops[i].kind == PLH_OP_PLANE_FETCH)
        m->fetch1 = i++;
    if (i < n && pass->ops[i].kind == PLH_OP_AFFINE)
        m->affine = i++;
    return i;
}

// Is this the merge pass k_pass_merge is written for? Fills pass->chain and pass->epi.
static bool pass_merge_applies(plh_pass *pass)
{
    plh_merge m;
    const int i = pass_merge_plan(pass, &m), n = pass->num_ops;
    if (i < 0)
        return false;
    pass->chain = plh_map_chain{ 0, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, 0 };
    pass->epi = plh_fast_epi{};
    if (i == n)
        return pass->dst.fmt == PLH_FMT_RGBA16F;    // (an rgba16 target stores through the epilogue)
    plh_match_map_chain(pass, false, false, true, i);
    if (pass->chain.enabled)
        return true;
    if (pass->dst.fmt != PLH_FMT_RGBA16)
        return false;
    plh_match_fast_epilogue(pass, false, i);
    return pass->epi.enabled;
}

/*
 * k_pass_mix: the blending pass of pl_render_image_mix (src/renderer.c:3612-4052 -- the cached,
 * already scaled frames of a vsync, each linearised and weighted: color = sum_i w_i * linear(F_i),
 * then back to the target's curve, dither, store) without the interpreter:
 *   [LINEARIZE] MIX_ADD { PLANE_FETCH [LINEARIZE] MIX_ADD }* MIX_END [DELINEARIZE], then the fused
 *   epilogue into rgba16 or a plain store into rgba16hf.
 * Through k_pass_generic<.., MIX> that pass took 146 us at 4K for two frames (three waves' worth of
 * interpreter registers, nine transfer curves per pixel as serial per-channel switches); here the
 * same device functions in the same order -- bit-identical -- with the curves of a lane's two
 * pixels as independent chains (transfer.hiph). Two horizontally adjacent pixels per lane.
 */
#define PLH_MIX_MAX 8
struct plh_mixplan { int32_t n, delin; int32_t lin[PLH_MIX_MAX], add[PLH_MIX_MAX], fetch[PLH_MIX_MAX]; };

template <bool F16DST>
__global__ __launch_bounds__(PASS_BW * PASS_BH)
void k_pass_mix(const plh_pass p_, const plh_mixplan m)
{
    const plh_pass &p = plh_kernarg_pass();
    const plh_sampler_args &s = p.s;
    constexpr int NP = 2;
    const int x0 = NP * (blockIdx.x * PASS_BW + threadIdx.x);
    const int y = blockIdx.y * PASS_BH + threadIdx.y;
    if (x0 >= p.width || y >= p.height)
        return;
    const bool all = x0 + 1 < p.width;
    const plh_fast_epi &e = p.epi;
    float bias[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int ix = (x0 + i + p.frag_x0) & e.mask, iy = (y + p.frag_y0) & e.mask;
        bias[i] = !F16DST && e.has_dither ? e.matrix[iy * e.size + ix] : 0.0f;
    }
    float4_t c[NP], mix[NP];
    float mx[NP];
    const float my = p.out_scale[1] * ((float) y + 0.5f);
#pragma unroll
    for (int i = 0; i < NP; i++) {
        const int x = all ? x0 + i : x0;
        c[i] = plh_fetch(s.src, x, y);
        if (s.scale != 1.0f)
            c[i] = scale4(c[i], s.scale);
        mx[i] = p.out_scale[0] * ((float) x + 0.5f);
        mix[i] = { 0.0f, 0.0f, 0.0f, 0.0f };
    }
#pragma unroll 1
    for (int f = 0; f < m.n; f++) {
        if (f > 0) {
#pragma unroll
            for (int i = 0; i < NP; i++)
                op_plane_fetch(c[i], p.ops[m.fetch[f]], mx[i], my);
        }
        if (m.lin[f] >= 0)
            op_linearize_px(c, p.ops[m.lin[f]]);
        const float w = p.ops[m.add[f]].f[0];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            // mix_color += vec4(weight) * color (the interpreter's MIX_ADD: product, then sum)
            mix[i].x += w * c[i].x; mix[i].y += w * c[i].y; mix[i].z += w * c[i].z; mix[i].w += w * c[i].w;
        }
    }
#pragma unroll
    for (int i = 0; i < NP; i++)
        c[i] = mix[i];
    if (m.delin >= 0)
        op_delinearize_px(c, p.ops[m.delin]);
    uint32_t o[2 * NP];
#pragma unroll
    for (int i = 0; i < NP; i++) {
        if (F16DST) {
            o[2 * i] = (uint32_t) plh_f2h(c[i].x) | ((uint32_t) plh_f2h(c[i].y) << 16);
            o[2 * i + 1] = (uint32_t) plh_f2h(c[i].z) | ((uint32_t) plh_f2h(c[i].w) << 16);
            continue;
        }
        if (e.has_dither) {
            const float b = bias[i], ds = e.dscale, di = e.dinv;
            c[i] = { __builtin_floorf(ds * c[i].x + b) * di, __builtin_floorf(ds * c[i].y + b) * di,
                     __builtin_floorf(ds * c[i].z + b) * di, __builtin_floorf(ds * c[i].w + b) * di };
        }
        if (e.has_scale)
            c[i] = scale4(c[i], e.scale);
        o[2 * i] = plh_unorm16x2(c[i].x, c[i].y);
        o[2 * i + 1] = plh_unorm16x2(c[i].z, c[i].w);
    }
    char *d = (char *) p.dst.ptr + (size_t) y * p.dst.pitch + (size_t) x0 * 8;
    if (all) {
        const plh_u32x4 pk = { o[0], o[1], o[2], o[3] };
        // (an rgba16 target is a final frame: streamed; an rgba16hf one is the intermediate the next
        // pass reads: cached. At compile time: `if (nt) non-temporal else plain` is folded into one
        // plain store, devmath.hiph)
        if constexpr (F16DST)
            *(plh_u32x4 *) d = pk;
        else
            __builtin_nontemporal_store(pk, (plh_u32x4 *) d);
    } else {
        const plh_u32x2 one = { o[0], o[1] };
        if constexpr (F16DST)
            *(plh_u32x2 *) d = one;
        else
            __builtin_nontemporal_store(one, (plh_u32x2 *) d);
    }
}

// The blending pass k_pass_mix is written for, as `m`: the index of the first op behind the blend,
// or -1 where the pass is none (k_pass_mix's plan: its test and its launch both ask here)
static int pass_mix_plan(const plh_pass *pass, plh_mixplan *m)
{
    const plh_sampler_args &s = pass->s;
    if (!plh_switch(PLH_SW_PASS_NATIVE))
        return -1;
    if (!plh_pass_covers_source(pass) || s.type != PLH_SAMPLE_NEAREST ||
        s.address_mode != PLH_ADDRESS_CLAMP || pass->transpose || pass->num_pre_ops ||
        !plh_pass_plain_target(pass) ||
        (pass->dst.fmt != PLH_FMT_RGBA16 && pass->dst.fmt != PLH_FMT_RGBA16F))
        return -1;
    const int n = pass->num_ops;
    int i = 0;
    *m = plh_mixplan{};
    m->delin = -1;
    for (;;) {
        if (m->n == PLH_MIX_MAX)
            return -1;
        const int f = m->n;
        m->fetch[f] = m->lin[f] = -1;
        if (f > 0) {
            if (!(i < n && pass->ops[i].kind == PLH_OP_PLANE_FETCH))
                return -1;
            m->fetch[f] = i++;
        }
        if (i < n && pass->ops[i].kind == PLH_OP_LINEARIZE)
            m->lin[f] = i++;
        if (!(i < n && pass->ops[i].kind == PLH_OP_MIX_ADD))
            return -1;
        m->add[f] = i++;
        m->n++;
        if (i < n && pass->ops[i].kind == PLH_OP_MIX_END) {
            i++;
            break;
        }
    }
    if (m->n < 2)
        return -1;
    if (i < n && pass->ops[i].kind == PLH_OP_DELINEARIZE)
        m->delin = i++;
    return i;
}

// Is this the blending pass k_pass_mix is written for? Fills pass->epi.
static bool pass_mix_applies(plh_pass *pass)
{
    plh_mixplan m;
    const int i = pass_mix_plan(pass, &m), n = pass->num_ops;
    if (i < 0)
        return false;
    pass->chain = plh_map_chain{ 0, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, 0 };
    pass->epi = plh_fast_epi{};
    if (pass->dst.fmt == PLH_FMT_RGBA16F)
        return i == n;
    plh_match_fast_epilogue(pass, false, i);
    return pass->epi.enabled;
}

// lut3d_tricubic: the gamut LUT op with its cubic flag set
static bool pass_has_tricubic(const plh_pass *pass)
{
    for (int i = 0; i < pass->num_ops; i++) {
        if (pass->ops[i].kind == PLH_OP_GAMUT_LUT && pass->ops[i].f[3] != 0.0f)
            return true;
    }
    return false;
}

// the shape k_pass_native is written for (and, with `features`, k_pass_features)
static bool pass_native_shape(const plh_pass *pass, bool features = false)
{
    const plh_sampler_args &s = pass->s;
    if (!plh_switch(PLH_SW_PASS_NATIVE))
        return false;
    if (!plh_pass_covers_source(pass) || s.type != PLH_SAMPLE_NEAREST ||
        s.address_mode != PLH_ADDRESS_CLAMP || pass->transpose || pass->num_pre_ops ||
        !plh_pass_plain_target(pass) ||
        (s.src.fmt != PLH_FMT_RGBA16 && s.src.fmt != PLH_FMT_RGBA16F))
        return false;
    if (features)   // (k_pass_features: the one op into an r16hf plane)
        return pass->dst.fmt == PLH_FMT_R16F && pass->num_ops == 1 && pass->ops[0].kind == PLH_OP_FEATURES;
    if (pass->dst.fmt != PLH_FMT_RGBA16 && pass->dst.fmt != PLH_FMT_RGBA16F)
        return false;
    // (frame mixing, the measurement and the tricubic lookup have their own kernels)
    return !plh_pass_has_op(pass, PLH_OP_MIX_ADD) && !plh_pass_has_op(pass, PLH_OP_MIX_END) &&
           !plh_pass_has_op(pass, PLH_OP_PEAK_DETECT) && !pass_has_tricubic(pass);
}

/* ------------------------------------------------------------------------ */

int plh_launch_polar(hipStream_t stream, const plh_pass *pass);
int plh_launch_ortho(hipStream_t stream, const plh_pass *pass);
int plh_launch_deband(hipStream_t stream, const plh_pass *pass);
int plh_launch_peak(hipStream_t stream, const plh_pass *pass);
extern "C" int plh_launch_deinterlace(plh_stream stream, const struct plh_pass *pass);

// k_pass_viz.hip: the variant with the colour map's diagnostics (and the Dolby Vision ops)
int plh_launch_generic_viz(hipStream_t stream, const plh_pass *pass, bool cubic);

// no sampler, or one texel / one hardware-bilinear footprint per pixel
static bool pass_simple_sampler(const plh_pass *pass)
{
    return pass->s.type == PLH_SAMPLE_NONE || pass->s.type == PLH_SAMPLE_NEAREST ||
           pass->s.type == PLH_SAMPLE_BILINEAR;
}

// the generic kernel (any sampler without a kernel of its own, any op list)
static int plh_launch_generic(hipStream_t stream, const plh_pass *pass, bool cubic, bool dovi)
{
    const dim3 block(PASS_BW, PASS_BH);
    const bool lite = plh_ops_lite(pass, 0, pass->num_ops);
    const bool simple = pass_simple_sampler(pass);
    // 2x2 cells share the bilinear footprint; everything else prefers the lighter 2x1 cells
    // (measured: 4K colour map 193 -> 168 us, plane copy 20.4 -> 18.8 us)
    int ch = pass->s.type == PLH_SAMPLE_BILINEAR && lite ? 2 : 1;
    const bool mixing = plh_pass_has_op(pass, PLH_OP_MIX_ADD);
    if (mixing || cubic || dovi)
        ch = 1;
    const int cells_w = (pass->width + pass->cell_padx + 1) / 2;
    const int cells_h = ch == 2 ? (pass->height + pass->cell_pady + 1) / 2 : pass->height;
    const int bh = PASS_BH * PASS_ITERS;
    const dim3 grid((cells_w + PASS_BW - 1) / PASS_BW, (cells_h + bh - 1) / bh);
#define LAUNCH(L, S, C) PLH_LAUNCH_LAST((k_pass_generic<L, S, C>), grid, block, 0, stream, *pass)
    if (dovi) {
        if (cubic || mixing)
            return -1004;
        PLH_LAUNCH_LAST((k_pass_generic<false, false, 1, false, false, true>), grid, block, 0, stream, *pass);
    } else if (cubic) {
        PLH_LAUNCH_LAST((k_pass_generic<false, true, 1, false, true>), grid, block, 0, stream, *pass);
    } else if (mixing) {
        // frame mixing: the one variant that carries the second colour register
        if (!simple)
            return -1003;
        PLH_LAUNCH_LAST((k_pass_generic<false, true, 1, true>), grid, block, 0, stream, *pass);
    } else if (ch == 2) {
        if (lite && simple) LAUNCH(true, true, 2);
        else if (lite)      LAUNCH(true, false, 2);
        else if (simple)    LAUNCH(false, true, 2);
        else                LAUNCH(false, false, 2);
    } else {
        if (lite && simple) LAUNCH(true, true, 1);
        else if (lite)      LAUNCH(true, false, 1);
        else if (simple)    LAUNCH(false, true, 1);
        else                LAUNCH(false, false, 1);
    }
#undef LAUNCH
    return plh_launch_status();
}

/* ---- the candidates for a 1:1 pass (launch_ladder.hiph), in the order of plh_launch_pass's table ---- */

// A kernel with a <true> / <false> pair of instances: launch the one `which` picks as the pass's
// last kernel (the kernel's arguments follow `stream`)
#define PASS_LAUNCH_PAIR(kernel, which, grid, block, stream, ...)                                   \
    do {                                                                                            \
        if (which)                                                                                  \
            PLH_LAUNCH_LAST(kernel<true>, grid, block, 0, stream, __VA_ARGS__);                     \
        else                                                                                        \
            PLH_LAUNCH_LAST(kernel<false>, grid, block, 0, stream, __VA_ARGS__);                    \
    } while (0)

// k_nearest_fast, k_bilinear_fast: PL_HIP_BILIN_ITERS cells per lane (0 = the generic kernel, for
// either) of a clamped sampler of `type` on a packed 16-bit source, nothing in front of it; 0: not such a pass
static int pass_fast_cells(const plh_pass *pass, int type)
{
    const int iters_env = plh_switch(PLH_SW_BILIN_ITERS);
    if (!iters_env || pass->s.type != type ||
        pass->s.address_mode != PLH_ADDRESS_CLAMP || pass->num_pre_ops || pass->transpose ||
        (pass->s.src.fmt != PLH_FMT_RGBA16 && pass->s.src.fmt != PLH_FMT_RGBA16F))
        return 0;
    return iters_env == 2 || iters_env == 4 ? iters_env : 1;
}

static bool nearest_fast_applies(plh_pass *pass)
{
    if (!pass_fast_cells(pass, PLH_SAMPLE_NEAREST))
        return false;
    plh_match_fast_epilogue(pass, true);
    return pass->epi.enabled;
}

static int launch_nearest_fast(hipStream_t stream, const plh_pass *pass)
{
    const int cells_w = (pass->width + pass->cell_padx + 1) / 2;
    const dim3 grid((cells_w + BF_BW - 1) / BF_BW, (pass->height + BF_BH * NF_ROWS - 1) / (BF_BH * NF_ROWS));
    PASS_LAUNCH_PAIR(k_nearest_fast, pass->s.src.fmt == PLH_FMT_RGBA16F, grid, dim3(BF_BW, BF_BH), stream, *pass);
    return plh_launch_status();
}

static bool bilinear_fast_applies(plh_pass *pass)
{
    if (!pass_fast_cells(pass, PLH_SAMPLE_BILINEAR))
        return false;
    plh_match_fast_epilogue(pass, true);
    return pass->epi.enabled;
}

// k_bilinear_fast's instance for the source's texels, the cells per lane and the alpha override
template <bool F16SRC>
static plh_pass_launch_fn *bilinear_fast_cells_instance(const plh_pass *pass)
{
#define BF(IT) return pass->epi.has_alpha ? plh_launch_last_lds<k_bilinear_fast<F16SRC, IT, true>> \
                                          : plh_launch_last_lds<k_bilinear_fast<F16SRC, IT, false>>
    switch (pass_fast_cells(pass, PLH_SAMPLE_BILINEAR)) {
    case 4:  BF(4);
    case 2:  BF(2);
    default: BF(1);
    }
#undef BF
}

static plh_pass_launch_fn *bilinear_fast_instance(const plh_pass *pass)
{
    return pass->s.src.fmt == PLH_FMT_RGBA16F ? bilinear_fast_cells_instance<true>(pass)
                                              : bilinear_fast_cells_instance<false>(pass);
}

static int launch_bilinear_fast(hipStream_t stream, const plh_pass *pass)
{
    const int cells_w = (pass->width + pass->cell_padx + 1) / 2;
    const int cells_h = (pass->height + pass->cell_pady + 1) / 2;
    const int bh = BF_BH * pass_fast_cells(pass, PLH_SAMPLE_BILINEAR);
    const dim3 grid((cells_w + BF_BW - 1) / BF_BW, (cells_h + bh - 1) / bh);
    return bilinear_fast_instance(pass)(grid, dim3(BF_BW, BF_BH), 0, stream, *pass);
}

// grid of the kernels that give a lane two horizontally adjacent pixels of a 1:1 pass, in
// workgroups of PASS_BW x PASS_BH lanes (k_pass_merge, k_pass_mix, k_pass_features)
static dim3 pass_pair_grid(const plh_pass *pass)
{
    return dim3(((pass->width + 1) / 2 + PASS_BW - 1) / PASS_BW, (pass->height + PASS_BH - 1) / PASS_BH);
}

static int launch_pass_merge(hipStream_t stream, const plh_pass *pass)
{
    plh_merge m;
    pass_merge_plan(pass, &m);
    PASS_LAUNCH_PAIR(k_pass_merge, pass->dst.fmt == PLH_FMT_RGBA16F, pass_pair_grid(pass), dim3(PASS_BW, PASS_BH),
                     stream, *pass, m);
    return plh_launch_status();
}

static int launch_pass_mix(hipStream_t stream, const plh_pass *pass)
{
    plh_mixplan m;
    pass_mix_plan(pass, &m);
    PASS_LAUNCH_PAIR(k_pass_mix, pass->dst.fmt == PLH_FMT_RGBA16F, pass_pair_grid(pass), dim3(PASS_BW, PASS_BH),
                     stream, *pass, m);
    return plh_launch_status();
}

static bool pass_features_applies(plh_pass *pass) { return pass_native_shape(pass, true); }

static int launch_pass_features(hipStream_t stream, const plh_pass *pass)
{
    PASS_LAUNCH_PAIR(k_pass_features, pass->s.src.fmt == PLH_FMT_RGBA16F, pass_pair_grid(pass), dim3(PASS_BW, PASS_BH),
                     stream, *pass);
    return plh_launch_status();
}

// k_pass_chain: k_pass_native's shape with an op list that is a map chain -- into rgba16 every chain,
// into the rgba16hf intermediate the ones without contrast recovery
static bool pass_chain_applies(plh_pass *pass)
{
    if (!pass_native_shape(pass))
        return false;
    plh_match_map_chain(pass, true, true, true);
    plh_map_chain &c = pass->chain;
    if (!c.enabled || (pass->dst.fmt != PLH_FMT_RGBA16 && c.contrast_recovery))
        return false;
    if (pass->dst.fmt == PLH_FMT_RGBA16) {
        // the tone curve's table in LDS where it fits
        c.tone_lds = 0;
        if (c.tone >= 0 && pass->ops[c.tone].i0 >= 2 && pass->ops[c.tone].ptr) {
            const int n = (int) pass->ops[c.tone].f[8] + 1;
            if (n >= 2 && n <= PQSEG_TONE_MAX)
                c.tone_lds = n;
        }
    }
    return true;
}

static int launch_pass_chain(hipStream_t stream, const plh_pass *pass)
{
    const dim3 block(PASS_BW, PASS_BH);
    const bool f16 = pass->s.src.fmt == PLH_FMT_RGBA16F;
    if (pass->dst.fmt == PLH_FMT_RGBA16F) {
        // (two pixels per lane: into the f16 intermediate the chain is short -- decode, linearize,
        // [sigmoidize] -- and the pass moves 16 bytes per pixel: 16-byte loads and stores. 4K:
        // 40.8 -> 35.5 us, 1080p unchanged, profiles/r05_33)
        const int cells_w = (pass->width + 1) / 2;
        const dim3 grid((cells_w + PASS_BW - 1) / PASS_BW, (pass->height + PASS_BH - 1) / PASS_BH);
        if (f16) PLH_LAUNCH_LAST((k_pass_chain<true, 2, false, true>), grid, block, 0, stream, *pass);
        else     PLH_LAUNCH_LAST((k_pass_chain<false, 2, false, true>), grid, block, 0, stream, *pass);
        return plh_launch_status();
    }
    // (The PQ pair as piecewise cubics in LDS, pqseg.hiph, was tried here as k_pass_chain_seg and
    // dropped: 14 % fewer vector instructions and the same time -- 94.5 us against 93.5 with the
    // tables staged per 64 x 4 pixels, 100 / 102 with two / eight rows per workgroup, whose
    // gathers then wait for the previous row's store, 119 with two pixels per lane
    // (profiles/r06_16_seg_ab.txt, r06_17_seg_ab.txt). At eight waves per SIMD this pass is
    // bound by the latency chain load -> tone gather -> gamut gathers -> store, not by
    // instruction issue; k_polar_mx at four waves per SIMD is, and gains 14 %.)
    const int cells_w = (pass->width + CHAIN_NP - 1) / CHAIN_NP;
    const dim3 grid((cells_w + PASS_BW - 1) / PASS_BW, (pass->height + PASS_BH - 1) / PASS_BH);
    const size_t shmem = (size_t) pass->chain.tone_lds * 4;
    if (pass->chain.contrast_recovery) {
        if (f16) PLH_LAUNCH_LAST((k_pass_chain<true, CHAIN_NP, true>), grid, block, shmem, stream, *pass);
        else     PLH_LAUNCH_LAST((k_pass_chain<false, CHAIN_NP, true>), grid, block, shmem, stream, *pass);
    } else {
        if (f16) PLH_LAUNCH_LAST((k_pass_chain<true, CHAIN_NP, false>), grid, block, shmem, stream, *pass);
        else     PLH_LAUNCH_LAST((k_pass_chain<false, CHAIN_NP, false>), grid, block, shmem, stream, *pass);
    }
    return plh_launch_status();
}

// k_pass_native: the same shape, any op list, interpreted
static bool pass_native_applies(plh_pass *pass) { return pass_native_shape(pass); }

static int launch_pass_native(hipStream_t stream, const plh_pass *pass)
{
    const dim3 block(PASS_BW, PASS_BH);
    const int cells_w = (pass->width + 1) / 2, bh = PASS_BH * PASS_ITERS;
    const dim3 grid((cells_w + PASS_BW - 1) / PASS_BW, (pass->height + bh - 1) / bh);
    const bool fs = pass->s.src.fmt == PLH_FMT_RGBA16F, fd = pass->dst.fmt == PLH_FMT_RGBA16F;
#define NATIVE(LITE) do { \
        if (fs && fd)   PLH_LAUNCH_LAST((k_pass_native<LITE, true, true>), grid, block, 0, stream, *pass); \
        else if (fs)    PLH_LAUNCH_LAST((k_pass_native<LITE, true, false>), grid, block, 0, stream, *pass); \
        else if (fd)    PLH_LAUNCH_LAST((k_pass_native<LITE, false, true>), grid, block, 0, stream, *pass); \
        else            PLH_LAUNCH_LAST((k_pass_native<LITE, false, false>), grid, block, 0, stream, *pass); \
    } while (0)
    if (plh_ops_lite(pass, 0, pass->num_ops))
        NATIVE(true);
    else
        NATIVE(false);
#undef NATIVE
    return plh_launch_status();
}

// k_pass_generic: every pass that has come this far
static int launch_pass_generic(hipStream_t stream, const plh_pass *pass)
{
    return plh_launch_generic(stream, pass, pass_has_tricubic(pass), false);
}
#undef PASS_LAUNCH_PAIR

extern "C" int plh_launch_pass(plh_stream stream_, const struct plh_pass *pass)
{
    hipStream_t stream = (hipStream_t) stream_;
    if (pass->width <= 0 || pass->height <= 0)
        return 0;

    if (plh_switch(PLH_SW_PASS_TRACE)) {
        fprintf(stderr, "[plh] pass %dx%d sampler=%d src.fmt=%d dst.fmt=%d transpose=%d pre=%d ops:",
                pass->width, pass->height, pass->s.type, pass->s.src.fmt, pass->dst.fmt,
                pass->transpose, pass->num_pre_ops);
        for (int i = 0; i < pass->num_ops; i++)
            fprintf(stderr, " %d", pass->ops[i].kind);
        fprintf(stderr, "\n");
    }

    const bool measuring = plh_pass_has_op(pass, PLH_OP_PEAK_DETECT);
    const bool mixing = plh_pass_has_op(pass, PLH_OP_MIX_ADD);

    // lut3d_tricubic lives in one variant of the generic kernel: such a colour map must be its
    // own pass (the renderer arranges that; a hand-built shader samples from an FBO first)
    const bool cubic = pass_has_tricubic(pass);
    if (cubic && (!pass_simple_sampler(pass) || measuring || mixing))
        return -1004;

    // Dolby Vision ops exist in one variant of the generic kernel only: such a pass (the
    // renderer's decoding pass of a Dolby Vision frame) goes straight there, past every
    // specialised kernel, and is refused behind a sampler that has its own kernel
    // (the corner-rounding op lives in the same variant and takes the same way: no specialised
    // kernel carries it, so none may be handed a pass with it -- it would be dropped)
    // The colour map's diagnostics (show_clipping, visualize_lut) take the same way, to a
    // sibling of that variant with the clip flags' register (k_pass_viz.hip), which also has the
    // tricubic lookup: the plot goes through the pixel's own LUT.
    bool dovi = false, viz = false;
    for (int i = 0; i < pass->num_ops; i++) {
        dovi |= plh_op_generic_only(pass->ops[i].kind);
        viz |= plh_op_is_viz(pass->ops[i].kind);
    }
    if (dovi) {
        if (measuring || (viz && mixing))
            return -1004;
        if (pass->s.type >= PLH_SAMPLE_POLAR && pass->s.type != PLH_SAMPLE_DISTORT)
            return -1004;
        if (viz)
            return pass->num_pre_ops ? -1004 : plh_launch_generic_viz(stream, pass, cubic);
        return plh_launch_generic(stream, pass, cubic, true);
    }

    switch (pass->s.type) {
    case PLH_SAMPLE_POLAR:
        return plh_launch_polar(stream, pass);
    case PLH_SAMPLE_ORTHO:
        return plh_launch_ortho(stream, pass);
    case PLH_SAMPLE_DEBAND:
        return plh_launch_deband(stream, pass);
    case PLH_SAMPLE_DEINTERLACE:
        // (its kernel carries the plain interpreter: a measurement, a frame mix or the tricubic
        // LUT behind it need the deinterlaced plane as a texture first, as the renderer arranges)
        return measuring || mixing || cubic ? -1004 : plh_launch_deinterlace(stream_, pass);
    default:
        break;
    }

    // a peak-detection stage needs the 16x16 tiling + LDS state of k_peak.hip
    if (measuring)
        return plh_launch_peak(stream, pass);

    // The kernels for every other pass, in the order they are tried
    static const plh_candidate candidates[] = {
        { "k_nearest_fast",  nearest_fast_applies,  launch_nearest_fast },   // nearest / bilinear fetch + the fused epilogue
        { "k_bilinear_fast", bilinear_fast_applies, launch_bilinear_fast },
        { "k_pass_merge",    pass_merge_applies,    launch_pass_merge },     // texel for texel: a planar frame assembled
        { "k_pass_mix",      pass_mix_applies,      launch_pass_mix },       // ... cached frames blended
        { "k_pass_features", pass_features_applies, launch_pass_features },  // ... the feature plane
        { "k_pass_chain",    pass_chain_applies,    launch_pass_chain },     // ... a map chain as straight-line code
        { "k_pass_native",   pass_native_applies,   launch_pass_native },    // ... any op list, interpreted
        { "k_pass_generic",  plh_applies_always,    launch_pass_generic },   // every pass
    };
    return plh_launch_first(candidates, stream, pass);
}

// Test hook (tests/test_chain_match.py, CPU): plh_match_map_chain on an op list described by its
// kinds and one flag word per op -- TONE_MAP: 1 = contrast recovery; GAMUT_LUT: 1 = tricubic;
// PLANE_MAP: 1 = not an identity mapping; DITHER: 1 = not the plain LUT path; SCALE: 1 = not uniform.
extern "C" __attribute__((visibility("default")))
int plh_test_match_chain(const int *kinds, const int *flags, int n, int num_pre, int dst_fmt, int transpose,
                         int allow_cr, int allow_plane_map, int allow_f16_dst, int *out)
{
    static plh_pass pass;   // (2.5 KB)
    pass = plh_pass{};
    if (n > PLH_MAX_OPS)
        return -1;
    pass.num_ops = n;
    pass.num_pre_ops = num_pre;
    pass.dst.fmt = dst_fmt;
    pass.transpose = transpose;
    for (int i = 0; i < n; i++) {
        plh_op &op = pass.ops[i];
        op.kind = kinds[i];
        switch (kinds[i]) {
        case PLH_OP_TONE_MAP:   op.i2 = flags[i] ? 0x100010 : 0; break;
        case PLH_OP_GAMUT_LUT:  op.f[3] = flags[i] ? 1.0f : 0.0f; break;
        case PLH_OP_PLANE_MAP:  op.i2 = !flags[i]; op.i1 = 3; op.f[3] = 1.0f; break;
        case PLH_OP_DITHER:     op.i0 = 64; op.i1 = flags[i] ? 1 : 0; op.f[0] = 1023.0f; op.f[1] = 1.0f;
                                op.f[3] = 10.0f; op.f[8] = 1.0f / 1023.0f; break;
        case PLH_OP_SCALE:      op.f[0] = op.f[1] = op.f[2] = 0.5f; op.f[3] = flags[i] ? 0.25f : 0.5f; break;
        default: break;
        }
    }
    plh_match_map_chain(&pass, allow_cr != 0, allow_plane_map != 0, allow_f16_dst != 0);
    const plh_map_chain &c = pass.chain;
    const int v[15] = { c.enabled, c.lin, c.in, c.tone, c.gamut, c.out, c.delin, c.contrast_recovery, c.unsig, c.sig,
                        c.pmap, c.tail, pass.epi.enabled, pass.epi.has_dither, pass.epi.has_scale };
    for (int i = 0; i < 15; i++)
        out[i] = v[i];
    return c.enabled;
}

// Test hook (tests/test_chain_match.py, CPU): pass_mix_applies on a texel-for-texel NEAREST pass
// whose op list is given by its kinds (DITHER / SCALE as the plain fused epilogue).
// out = { frames, delin, epi.enabled, lin[0..3], fetch[0..3] }
extern "C" __attribute__((visibility("default")))
int plh_test_match_mix(const int *kinds, int n, int dst_fmt, int sampler, int *out)
{
    static plh_pass pass;
    pass = plh_pass{};
    if (n > PLH_MAX_OPS)
        return -1;
    pass.num_ops = n;
    pass.width = pass.s.src.w = pass.dst.w = 64;
    pass.height = pass.s.src.h = pass.dst.h = 48;
    pass.s.pos[1][0] = pass.s.pos[3][0] = pass.s.pos[2][1] = pass.s.pos[3][1] = 1.0f;
    pass.s.type = sampler;
    pass.s.address_mode = PLH_ADDRESS_CLAMP;
    pass.s.src.fmt = PLH_FMT_RGBA16F;
    pass.dir_x = pass.dir_y = 1;
    pass.dst.fmt = dst_fmt;
    for (int i = 0; i < n; i++) {
        plh_op &op = pass.ops[i];
        op.kind = kinds[i];
        if (kinds[i] == PLH_OP_DITHER) {
            op.i0 = 64; op.f[0] = 1023.0f; op.f[1] = 1.0f; op.f[3] = 10.0f; op.f[8] = 1.0f / 1023.0f;
        } else if (kinds[i] == PLH_OP_SCALE) {
            op.f[0] = op.f[1] = op.f[2] = op.f[3] = 0.5f;
        }
    }
    plh_mixplan m;
    pass_mix_plan(&pass, &m);
    const bool ok = pass_mix_applies(&pass);
    out[0] = ok ? m.n : 0;
    out[1] = m.delin;
    out[2] = pass.epi.enabled;
    for (int f = 0; f < 4; f++) {
        out[3 + f] = f < m.n ? m.lin[f] : -1;
        out[7 + f] = f < m.n ? m.fetch[f] : -1;
    }
    return ok;
}
