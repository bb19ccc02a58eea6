/*
 * libplacebo-hip — polar on the matrix pipe: the host-built blob that k_polar_mx, k_polar_mxp,
 * k_polar_mxr and k_polar_mxd read (device side: k_polar_mx.hiph, struct plh_polar_mx).
 *
 * Pure arithmetic on host arrays -- no pl_gpu, no pl_buf: polar_tables.c hands in what the device
 * evaluated for the pass (struct mx_input) and uploads what comes back (struct mx_tables). The blob
 * holds the filter weights as f16 hi + lo halves in MFMA fragment order, their first-order
 * derivatives in the phase, and the per-column / per-row phase deviations:
 *   [nfrag][64 lanes][8] f16 | dfx[W padded to PLH_MX_PAD] | dfy[H padded] | (kind 1: 512 B sink)
 * Each geometry below keeps its axis recogniser and its (phase, tap) -> (fragment, lane, element)
 * map; every other step exists once. tests/test_polar_mx_tables.py pins the bytes.
 */
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "polar_priv.h"

// IEEE binary32 -> binary16, round to nearest even (subnormals and overflow included)
static uint16_t f32_to_f16(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u)
        return sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u);
    if (x >= 0x477ff000u)   // rounds to >= 65520: infinity
        return sign | 0x7c00u;
    if (x < 0x38800000u) {  // below the smallest normal half: a multiple of 2^-24
        const float scaled = fabsf(f) * 16777216.0f;       // exact
        return sign | (uint16_t) lrintf(scaled);            // (round-half-even rounding mode)
    }
    const uint32_t mant = x & 0x007fffffu, exp = (x >> 23) - 112;
    uint32_t h = (exp << 10) | (mant >> 13);
    const uint32_t rest = mant & 0x1fffu;
    if (rest > 0x1000u || (rest == 0x1000u && (h & 1)))
        h++;                // (a carry into the exponent is the correct result)
    return sign | (uint16_t) h;
}

static float f16_to_f32(uint16_t h)
{
    const int exp = (h >> 10) & 0x1f, mant = h & 0x3ff;
    float v;
    if (exp == 0)
        v = ldexpf((float) mant, -24);
    else if (exp == 31)
        v = mant ? NAN : INFINITY;
    else
        v = ldexpf((float) (mant | 0x400), exp - 25);
    return (h & 0x8000) ? -v : v;
}

/* ---- the steps every geometry shares ------------------------------------------------------- */

// what all three kinds ask of the pass (each adds its own shared-memory need, the upscales a bound)
static bool pass_fits(const struct polar_pass *p)
{
    return !p->tile_fp32 && p->address_mode == PLH_ADDRESS_CLAMP && !p->transpose && p->src_w >= 2 &&
           !(p->antiring > 0);
}

// tap (x, y) -> index in the list, for x, y in [-o, n - 1 - o]
struct tap_grid {
    int n, o;
    int at[PLH_MXD_TAPS][PLH_MXD_TAPS];     // [y + o][x + o], -1: no such tap
};

static inline int tap_x(const struct polar_weights *w, int t)
{
    return (int8_t) (w->taps[t] & 0xff);
}

static inline int tap_y(const struct polar_weights *w, int t)
{
    return (int8_t) ((w->taps[t] >> 8) & 0xff);
}

// false if a tap lies outside the grid
static bool tap_grid_fill(struct tap_grid *g, const struct polar_weights *w, int n, int o)
{
    g->n = n;
    g->o = o;
    for (int y = 0; y < n; y++) {
        for (int x = 0; x < n; x++)
            g->at[y][x] = -1;
    }
    for (int t = 0; t < w->ntaps; t++) {
        const int x = tap_x(w, t) + o, y = tap_y(w, t) + o;
        if (x < 0 || x >= n || y < 0 || y >= n)
            return false;
        g->at[y][x] = t;
    }
    return true;
}

// the tap one position further along axis a (0: x, 1: y), -1 if the list has none there
static int tap_next(const struct tap_grid *g, const struct polar_weights *w, int t, int a)
{
    const int x = tap_x(w, t) + g->o + !a, y = tap_y(w, t) + g->o + a;
    return x < g->n && y < g->n ? g->at[y][x] : -1;
}

// normalised weight (w * scale / wsum) of tap t for the class pair (kx, ky)
static inline double wn(const struct mx_input *in, int kx, int ky, int t)
{
    const float *w = in->w.wall + ((size_t) ky * in->x.ncls + kx) * (in->w.ntaps + 1);
    return (double) w[t] * (double) w[in->w.ntaps];
}

// d w' / d fcoord along axis a (0: x, 1: y) at the class pair at[] = (kx, ky), for every tap: the
// slope of a least-squares line through the normalised weights of the classes within 0.01 of
// at[a] (the classes of that phase -- the weights the per-pixel kernels actually use for them),
// the other axis' class held fixed. A class above `wrap` counts for the texel one higher, as
// fcoord - 1 with its weights one tap position further along the axis (k_polar_mxr's phase at
// fcoord = 0); fcoord < 1, so wrap = 1 means none. The sums run over the classes, then the taps,
// in double: their order is part of the blob's bytes.
static void fit_slopes(const struct mx_input *in, const struct tap_grid *g, int a, const int at[2],
                       float wrap, double *s)
{
    const struct polar_axis *ax = a ? &in->y : &in->x;
    const int ntaps = in->w.ntaps;
    double den = 0.0;
    memset(s, 0, ntaps * sizeof(double));
    for (int c = 0; c < ax->ncls; c++) {
        const bool wrapped = ax->cls[c] > wrap;
        const double d = (double) ax->cls[c] - (wrapped ? 1.0 : 0.0) - (double) ax->cls[at[a]];
        if (fabs(d) > 0.01)
            continue;   // another phase
        den += d * d;
        const int kx = a ? at[0] : c, ky = a ? c : at[1];
        for (int t = 0; t < ntaps; t++) {
            const int ts = wrapped ? tap_next(g, &in->w, t, a) : t;
            s[t] += d * ((ts >= 0 ? wn(in, kx, ky, ts) : 0.0) - wn(in, at[0], at[1], t));
        }
    }
    for (int t = 0; t < ntaps; t++)
        s[t] = den > 0.0 ? s[t] / den : 0.0;
}

// Blob of nfrag fragments for a target of in->x.len x in->y.len outputs, zeroed; t->mx gets the
// offsets of dfx / dfy (and of the sink, where the kind has one; bfrag is offset 0)
static bool tables_alloc(struct mx_tables *t, const struct mx_input *in, int nfrag, bool sink)
{
    const size_t nfx = ((size_t) in->x.len + PLH_MX_PAD - 1) / PLH_MX_PAD * PLH_MX_PAD;
    const size_t nfy = ((size_t) in->y.len + PLH_MX_PAD - 1) / PLH_MX_PAD * PLH_MX_PAD;
    const size_t o_dfx = (size_t) nfrag * 64 * 8 * sizeof(uint16_t), o_dfy = o_dfx + nfx * 4;
    const size_t o_sink = o_dfy + nfy * 4;      // (512 bytes nobody reads: plh_polar_mx.sink)
    t->size = o_sink + (sink ? 512 : 0);
    t->blob = calloc(1, t->size);
    t->mx.dfx = (const float *) o_dfx;
    t->mx.dfy = (const float *) o_dfy;
    t->mx.sink = sink ? (void *) o_sink : NULL;
    return t->blob;
}

// a weight and its slopes in fcoord_x / fcoord_y
struct weight {
    double v, vx, vy;
};

// `w` into fragments f .. f + 3 at lane l, element e: kind 0 / 1 the hi / lo f16 halves of the
// weight, kind 2 / 3 its slopes times 2^-PLH_MX_DSHIFT
static void frag_put(struct mx_tables *t, size_t f, int l, int e, struct weight w)
{
    uint16_t *frag = (uint16_t *) t->blob;
    const double dscale = ldexp(1.0, -PLH_MX_DSHIFT);
    const uint16_t hi = f32_to_f16((float) w.v);
    const uint16_t lo = f32_to_f16((float) (w.v - (double) f16_to_f32(hi)));
    t->worst = PL_MAX(t->worst, fabs(w.v - (double) f16_to_f32(hi) - (double) f16_to_f32(lo)));
    frag[((f + 0) * 64 + l) * 8 + e] = hi;
    frag[((f + 1) * 64 + l) * 8 + e] = lo;
    frag[((f + 2) * 64 + l) * 8 + e] = f32_to_f16((float) (w.vx * dscale));
    frag[((f + 3) * 64 + l) * 8 + e] = f32_to_f16((float) (w.vy * dscale));
}

// the phase output i is expanded about: at[(i + shift) % period]
struct phase_ref {
    int period, shift;
    float at[PLH_MXR_MAX_RATIO];
};

// dfx (a = 0) / dfy (a = 1): how far every output's own phase fc[i] lies from the one it is
// expanded about, times 2^PLH_MX_DSHIFT
static void dev_table(struct mx_tables *t, int a, const float *fc, int len, const struct phase_ref *p)
{
    float *df = (float *) (t->blob + (size_t) (a ? t->mx.dfy : t->mx.dfx));
    const float up = ldexpf(1.0f, PLH_MX_DSHIFT);
    for (int i = 0; i < len; i++) {
        const float d = fc[i] - p->at[(i + p->shift) % p->period];
        t->dev = fmaxf(t->dev, fabsf(d));
        df[i] = d * up;
    }
}

/* ---- the exact 2x upscale (k_polar_mx, k_polar_mxp) ---------------------------------------- */

// The geometry k_polar_mx covers: an axis whose outputs alternate between two phases and step
// one source texel per two outputs (an exact 2x upscale, any sub-texel offset). Returns the
// class of each parity and c1 = base(1) - base(0); false if the axis does not have that shape.
static bool mx_axis(const struct polar_axis *ax, int canon[2], int *c1)
{
    const float *fc = ax->fc;
    const int32_t *base = ax->base;
    if (ax->len < 2)
        return false;
    *c1 = base[1] - base[0];
    if (*c1 != 0 && *c1 != 1)
        return false;
    for (int q = 0; q < 2; q++) {
        canon[q] = ax->ids[q];
        // (a phase next to 0 or 1 could flip its base texel with the rounding of one pixel)
        if (fc[q] < 0.02f || fc[q] > 0.98f)
            return false;
    }
    for (int i = 0; i < ax->len; i++) {
        const int q = i & 1;
        if (base[i] != base[0] + (i >> 1) + (q ? *c1 : 0))
            return false;
        // the phase of a column differs from its parity's by the fp32 rounding of the attribute
        // interpolation, which grows with the coordinate: a few ulps of the source position
        if (fabsf(fc[i] - fc[q]) > 1e-5f + 1.5f * FLT_EPSILON * (float) ax->len)
            return false;
    }
    return true;
}

// B fragments (plh_device.h): frag f = 4 * (py * npairs + j) + kind, lane l, element e hold
//   T(py, wy)[k][n] with n = l & 15, k = 8 * ((l >> 4) & 1) + e, wy = first[py] + 2 j + (l >> 5),
//   = w'(phase py, phase n & 1, tap (k - dbx[n] - 3, wy - 3)), kinds as in frag_put.
// first[py] = the first tap row of row phase py that carries a weight for either column phase;
// npairs = 3 when both row phases have at most six such rows (every centred 2x upscale with a
// radius <= 3.25: rows -3 and 4 of the reference's 8 x 8 tap square lie 3.25 / 3.75 texels from
// the sample), else 4.
static enum mx_refusal polar_mx_build(const struct mx_input *in, struct mx_tables *t)
{
    // LDS of the widest variant (RGBA tile, 4 wave-tile columns: 36 KiB of B fragments + 4 planes
    // of 41 rows x 96 B; the RGB tile of 8 columns needs 55.5 KiB) against the limit the backend
    // was created with (pl_hip_params.max_shmem_size)
    if (in->p.max_shmem_size < 64 * 1024)
        return MX_SHMEM;
    if (in->p.bound > 4 || !pass_fits(&in->p))
        return MX_PASS;
    int cx[2], cy[2], c1x, c1y;
    if (!mx_axis(&in->x, cx, &c1x) || !mx_axis(&in->y, cy, &c1y))
        return MX_GEOMETRY;
    const int ntaps = in->w.ntaps;
    struct tap_grid g;
    enum mx_refusal res = MX_REFUSED;
    // slopes at the class pair (cx[px], cy[py]): [axis][(py * 2 + px) * ntaps + t]
    double *slope[2] = { calloc((size_t) 4 * PL_MAX(ntaps, 1), sizeof(double)),
                         calloc((size_t) 4 * PL_MAX(ntaps, 1), sizeof(double)) };
    if (!tap_grid_fill(&g, &in->w, 8, 3) || !slope[0] || !slope[1] ||
        !tables_alloc(t, in, PLH_MX_NFRAG, true))
        goto done;
    for (int p = 0; p < 4; p++) {
        const int at[2] = { cx[p & 1], cy[p >> 1] };
        fit_slopes(in, &g, 0, at, 1.0f, slope[0] + (size_t) p * ntaps);
        fit_slopes(in, &g, 1, at, 1.0f, slope[1] + (size_t) p * ntaps);
    }

    // live tap rows of each row phase: a row counts when any column phase has a weight, a slope
    // included (the slopes are fitted through neighbouring classes, whose tap sets are the same:
    // mx_axis holds every class of a parity within 1e-5 of it)
    int first[2], npairs = 3;
    for (int py = 0; py < 2; py++) {
        int lo = 8, hi = -1;
        for (int wy = 0; wy < 8; wy++) {
            bool live = false;
            for (int wx = 0; wx < 8 && !live; wx++) {
                const int tap = g.at[wy][wx];
                if (tap < 0)
                    continue;
                for (int px = 0; px < 2 && !live; px++) {
                    live = wn(in, cx[px], cy[py], tap) != 0.0 ||
                           slope[0][(size_t) (py * 2 + px) * ntaps + tap] != 0.0 ||
                           slope[1][(size_t) (py * 2 + px) * ntaps + tap] != 0.0;
                }
            }
            if (live) {
                lo = PL_MIN(lo, wy);
                hi = wy;
            }
        }
        if (hi < lo)
            lo = hi = 3;
        first[py] = lo;
        if (hi - lo + 1 > 6)
            npairs = 4;
    }
    for (int py = 0; py < 2; py++)
        first[py] = PL_MIN(first[py], 8 - 2 * npairs);  // (the pairs stay inside the 8 tap rows)

    for (int py = 0; py < 2; py++) {
        for (int j = 0; j < npairs; j++) {
            for (int l = 0; l < 64; l++) {
                const int n = l & 15, px = n & 1;
                const int dbx = (n >> 1) + (px ? c1x : 0);
                const int wy = first[py] + 2 * j + (l >> 5);
                for (int e = 0; e < 8; e++) {
                    const int k = 8 * ((l >> 4) & 1) + e, wx = k - dbx;
                    struct weight w = {0};
                    if (wx >= 0 && wx < 8 && wy >= 0 && wy < 8 && g.at[wy][wx] >= 0) {
                        const int tap = g.at[wy][wx];
                        w.v = wn(in, cx[px], cy[py], tap);
                        w.vx = slope[0][(size_t) (py * 2 + px) * ntaps + tap];
                        w.vy = slope[1][(size_t) (py * 2 + px) * ntaps + tap];
                    }
                    frag_put(t, 4 * (size_t) (py * npairs + j), l, e, w);
                }
            }
        }
    }
    // how far a pixel's own phase lies from the one its parity is expanded about
    dev_table(t, 0, in->x.fc, in->x.len, &(struct phase_ref) { 2, 0, { in->x.fc[0], in->x.fc[1] } });
    dev_table(t, 1, in->y.fc, in->y.len, &(struct phase_ref) { 2, 0, { in->y.fc[0], in->y.fc[1] } });
    t->mx.enabled = 1;
    t->mx.org_x = in->x.base[0] - 3;
    t->mx.org_y = in->y.base[0] - 3;
    t->mx.npairs = npairs;
    // tile row of tap row first[py] for the output row pair 0: rows 2 m + py sample from base
    // rowbase[0] + m + (py ? c1y : 0)
    t->mx.row_first[0] = first[0];
    t->mx.row_first[1] = first[1] + c1y;
    res = MX_BUILT;
done:
    free(slope[0]);
    free(slope[1]);
    return res;
}

/* ---- the exact upscales by 3, 4 and 3 : 2 (k_polar_mxr) ------------------------------------ */

// fcoords above this belong to the phase at fcoord = 0 of the next texel
#define MXR_WRAP 0.98f

// what mxr_axis finds on an axis (canon: [len], the caller's)
struct mxr_found {
    int shift, origin, off[PLH_MXR_MAX_RATIO], rep[PLH_MXR_MAX_RATIO];
    float *canon;
};

// The geometry k_polar_mxr covers: an axis of an exact upscale by R : G (R outputs per G source
// texels; G = 1: the integer ratios). Output i belongs to base index (i + shift) / R and phase
// (i + shift) % R; the base texel of an output is origin + G * index + off[phase] with the same small
// offset for every output of a phase (G = 1: none); the phase of an output is its phase class' up
// to the fp32 rounding of the attribute interpolation. A phase at fcoord = 0 (odd integer ratios
// have one) is where that rounding decides between (base b, fcoord +eps) and (base b - 1, fcoord
// 1 - eps): the same sample position -- the tap that enters at one end and the one that leaves at
// the other lie beyond the filter's radius -- so such an output is taken as (b, fcoord - 1), a small
// negative deviation from the phase (`canon`: the outputs' canonical fcoord, which the caller turns
// into the deviations). Returns the shift, the origin, the offsets and a representative, unwrapped
// output of every phase.
static bool mxr_axis(const float *fc, const int32_t *base, int len, const int ratio[2],
                     struct mxr_found *m)
{
    const int R = ratio[0], G = ratio[1];
    if (len < 3 * R)
        return false;
    for (int i = 0; i < len; i++)
        m->canon[i] = fc[i] > MXR_WRAP ? fc[i] - 1.0f : fc[i];
#define CANON_BASE(i) (base[i] + (fc[i] > MXR_WRAP ? 1 : 0))
    // the shift: the one under which the offsets are consistent and smallest
    int best = -1, best_max = 0, best_org = 0;
    for (int sh = 0; sh < R; sh++) {
        int org = INT_MAX;
        for (int i = 0; i < 2 * R; i++)
            org = PL_MIN(org, CANON_BASE(i) - G * ((i + sh) / R));
        int o[PLH_MXR_MAX_RATIO], omax = 0;
        bool ok = true;
        for (int q = 0; q < R; q++)
            o[q] = -1;
        for (int i = 0; i < len && ok; i++) {
            const int q = (i + sh) % R;
            const int d = CANON_BASE(i) - G * ((i + sh) / R) - org;
            if (o[q] < 0)
                o[q] = d;
            ok = d == o[q] && d >= 0 && d <= (G == 1 ? 0 : 2);
            omax = PL_MAX(omax, d);
        }
        if (ok && (best < 0 || omax < best_max)) {
            best = sh;
            best_max = omax;
            best_org = org;
        }
    }
    if (best < 0)
        return false;
    m->shift = best;
    m->origin = best_org;
    for (int q = 0; q < R; q++)
        m->rep[q] = m->off[q] = -1;
    for (int i = 0; i < len; i++) {
        const int q = (i + best) % R;
        if (m->off[q] < 0)
            m->off[q] = CANON_BASE(i) - G * ((i + best) / R) - best_org;
        if (m->rep[q] < 0 && !(fc[i] > MXR_WRAP))
            m->rep[q] = i;
    }
#undef CANON_BASE
    for (int q = 0; q < R; q++) {
        if (m->rep[q] < 0 || m->off[q] < 0)
            return false;
    }
    for (int i = 0; i < len; i++) {
        const int q = (i + best) % R;
        if (fabsf(m->canon[i] - fc[m->rep[q]]) > 1e-5f + 1.5f * FLT_EPSILON * (float) len)
            return false;
    }
    return true;
}

// Test hook (tests/test_mxr_axis.py, CPU): mxr_axis on an axis described by its per-output base
// texels and fcoords. out = { shift, origin, off[0..3], rep[0..3] }; canon: len floats.
PL_API int plh_test_mxr_axis(const float *fc, const int32_t *base, int len, int R, int G,
                             int *out, float *canon);
int plh_test_mxr_axis(const float *fc, const int32_t *base, int len, int R, int G, int *out, float *canon)
{
    struct mxr_found m = { .canon = canon };
    if (R < 2 || R > PLH_MXR_MAX_RATIO || !mxr_axis(fc, base, len, (const int[2]) { R, G }, &m))
        return 0;
    out[0] = m.shift;
    out[1] = m.origin;
    for (int q = 0; q < PLH_MXR_MAX_RATIO; q++) {
        out[2 + q] = q < R ? m.off[q] : -1;
        out[2 + PLH_MXR_MAX_RATIO + q] = q < R ? m.rep[q] : -1;
    }
    return 1;
}

// B fragments of k_polar_mxr (plh_device.h): frag f = 32 py + 4 * (NH * j + h) + kind, lane l,
// element e hold T(py, j, h)[k][n], n = l & 15 the output column within half h of the wave's 8 / G
// bases -- base bi = 4 h + n / R, phase px = n % R, n < 4 R -- and K index (row 2 j + (l >> 5) of the
// base's footprint rows, column k = 8 * ((l >> 4) & 1) + e of the wave's 16-column window):
//   = w'(py, px, tap (k - G bi - offx[px] - 3, 2 j + (l >> 5) - offy[py] - 3)), kinds as in
// frag_put. NH halves and NJ row pairs: 2 and 4 for the integer ratios, 1 and 5 for 3 : 2.
// The classes a slope is fitted through: those within 0.01 of the phase -- and, for the phase at
// fcoord = 0 of an odd ratio, the WRAPPED ones on the other side of it (fcoord 1 - eps on the
// base one texel lower = -eps on this base: their weight for footprint position (x, y) is their
// own weight one position further along the axis). Without them that phase may have a single
// class, fcoord = 0 exactly, no slope, and its wrapped outputs -- up to 1e-4 away -- no
// first-order term (4 codes on white noise at 720p -> 4K).
static enum mx_refusal polar_mxr_build(const struct mx_input *in, struct mx_tables *t)
{
    if (in->p.max_shmem_size < 64 * 1024 || in->p.bound > 4 || !pass_fits(&in->p))
        return MX_REFUSED;
    const int W = in->x.len, H = in->y.len, ntaps = in->w.ntaps;
    enum mx_refusal res = MX_REFUSED;
    struct mxr_found fx = {0}, fy = {0};
    struct tap_grid g;
    double *slx = NULL, *sly = NULL;
    fx.canon = malloc(((size_t) W + H) * sizeof(float));
    if (!fx.canon)
        goto done;
    fy.canon = fx.canon + W;
    static const int ratios[][2] = { {3, 1}, {4, 1}, {3, 2} };
    int R = 0, G = 0;
    for (int r = 0; r < 3 && !R; r++) {
        if (mxr_axis(in->x.fc, in->x.base, W, ratios[r], &fx) &&
            mxr_axis(in->y.fc, in->y.base, H, ratios[r], &fy)) {
            R = ratios[r][0];
            G = ratios[r][1];
        }
    }
    if (!R) {
        res = MX_GEOMETRY;
        goto done;
    }
    const int NJ = G == 1 ? 4 : 5, NH = G == 1 ? 2 : 1;
    int cx[PLH_MXR_MAX_RATIO], cy[PLH_MXR_MAX_RATIO];
    struct phase_ref refx = { R, fx.shift }, refy = { R, fy.shift };
    for (int q = 0; q < R; q++) {
        cx[q] = in->x.ids[fx.rep[q]];
        cy[q] = in->y.ids[fy.rep[q]];
        refx.at[q] = in->x.fc[fx.rep[q]];
        refy.at[q] = in->y.fc[fy.rep[q]];
    }
    // d w' / d fcoord at every phase pair: [(py * R + px) * nt + t]
    const size_t nt = (size_t) PL_MAX(ntaps, 1);
    slx = calloc((size_t) R * R * nt, sizeof(double));
    sly = calloc((size_t) R * R * nt, sizeof(double));
    if (ntaps > 64 || !tap_grid_fill(&g, &in->w, 8, 3) || !slx || !sly ||
        !tables_alloc(t, in, R * PLH_MXR_FRAGS_PER_PHASE, false))
        goto done;
    for (int py = 0; py < R; py++) {
        for (int px = 0; px < R; px++) {
            const int at[2] = { cx[px], cy[py] };
            fit_slopes(in, &g, 0, at, MXR_WRAP, slx + (size_t) (py * R + px) * nt);
            fit_slopes(in, &g, 1, at, MXR_WRAP, sly + (size_t) (py * R + px) * nt);
        }
    }
    for (int py = 0; py < R; py++) {
        for (int j = 0; j < NJ; j++) {
            for (int h = 0; h < NH; h++) {
                const size_t f = (size_t) py * PLH_MXR_FRAGS_PER_PHASE + 4 * (size_t) (NH * j + h);
                for (int l = 0; l < 64; l++) {
                    const int n = l & 15, px = n % R, bi = 4 * h + n / R;
                    const int wy = 2 * j + (l >> 5) - fy.off[py];
                    for (int e = 0; e < 8; e++) {
                        const int k = 8 * ((l >> 4) & 1) + e, wx = k - G * bi - fx.off[px];
                        struct weight w = {0};
                        if (n < 4 * R && wx >= 0 && wx < 8 && wy >= 0 && wy < 8 && g.at[wy][wx] >= 0) {
                            const int tap = g.at[wy][wx];
                            w.v = wn(in, cx[px], cy[py], tap);
                            w.vx = slx[(size_t) (py * R + px) * nt + tap];
                            w.vy = sly[(size_t) (py * R + px) * nt + tap];
                        }
                        frag_put(t, f, l, e, w);
                    }
                }
            }
        }
    }
    dev_table(t, 0, fx.canon, W, &refx);
    dev_table(t, 1, fy.canon, H, &refy);
    t->mx.enabled = 3;
    t->mx.ratio = R;
    t->mx.group = G;
    t->mx.sx = fx.shift;
    t->mx.sy = fy.shift;
    t->mx.org_x = fx.origin - 3;    // (origin: the texel of base index 0, offset 0)
    t->mx.org_y = fy.origin - 3;
    res = MX_BUILT;
done:
    free(slx);
    free(sly);
    free(fx.canon);
    return res;
}

/* ---- the 2 : 1 downscale (k_polar_mxd) ----------------------------------------------------- */

// every output i has its base texel at base[0] + 2 i and a phase within 4e-3 of 1/2
static bool mxd_axis(const struct polar_axis *ax)
{
    if (ax->len < 2)
        return false;
    for (int i = 0; i < ax->len; i++) {
        if (ax->base[i] != ax->base[0] + 2 * i)
            return false;
        // (first-order expansion about 1/2: its neglected term is (d / a texel)^2 of a weight)
        if (fabsf(ax->fc[i] - 0.5f) > 4e-3f)
            return false;
    }
    return true;
}

// the class at exactly 1/2, or -1
static int half_class(const struct polar_axis *ax)
{
    int c0 = -1;
    for (int c = 0; c < ax->ncls; c++)
        c0 = ax->cls[c] == 0.5f ? c : c0;
    return c0;
}

// B fragments of k_polar_mxd (plh_device.h): frag f = 4 * (2 j + kb) + kind, lane l, element e hold
//   T_j[i], i = 32 kb + k - 2 n, n = l & 15, k = 8 * (l >> 4) + e  (0 outside the 14 taps),
// T_j[i] = the normalised weight w' of tap (i - 6, j - 6) at fcoord (1/2, 1/2) and its slopes over
// the phase classes that occur (all of them lie next to 1/2), kinds as in frag_put. Rows j and
// 13 - j are averaged (they agree to rounding: the distance of a tap to the sample point is the same).
static enum mx_refusal polar_mxd_build(const struct mx_input *in, struct mx_tables *t)
{
    enum { NT = PLH_MXD_TAPS };
    if (!pass_fits(&in->p))
        return MX_REFUSED;
    // (56 KiB of B fragments + a 140 x 76 tile of three f16 planes: one workgroup per CU)
    if (in->p.max_shmem_size < 124 * 1024)
        return MX_SHMEM;
    if (!mxd_axis(&in->x) || !mxd_axis(&in->y))
        return MX_REFUSED;
    // the class pair at exactly (1/2, 1/2): the expansion point
    const int at[2] = { half_class(&in->x), half_class(&in->y) };
    if (at[0] < 0 || at[1] < 0)
        return MX_NO_HALF;
    const int ntaps = in->w.ntaps;
    struct tap_grid g;
    enum mx_refusal res = MX_REFUSED;
    double *sx = calloc(PL_MAX(ntaps, 1), sizeof(double)), *sy = calloc(PL_MAX(ntaps, 1), sizeof(double));
    if (!tap_grid_fill(&g, &in->w, NT, 6) || !sx || !sy || !tables_alloc(t, in, PLH_MXD_NFRAG, false))
        goto done;
    fit_slopes(in, &g, 0, at, 1.0f, sx);
    fit_slopes(in, &g, 1, at, 1.0f, sy);

    // the first source row (and, mirrored, the last) that carries a weight at all: at fcoord = 1/2
    // rows -6 and 7 of the reference's 14 x 14 tap square lie 6.5 texels from the sample, beyond
    // twice any radius <= 3.25 (ewa_lanczos: 6.4766) -- the kernel starts its contraction there
    int first_row = NT / 2 - 1;
    for (int j = 0; j < NT / 2; j++) {
        for (int kb = 0; kb < 2; kb++) {
            for (int l = 0; l < 64; l++) {
                const int n = l & 15;
                for (int e = 0; e < 8; e++) {
                    const int i = 32 * kb + 8 * (l >> 4) + e - 2 * n;
                    struct weight w = {0};
                    if (i >= 0 && i < NT) {
                        const int ta = g.at[j][i], tb = g.at[NT - 1 - j][i];
                        if ((ta < 0) != (tb < 0))
                            goto done;      // (a tap list that is not symmetric: not this filter)
                        if (ta >= 0) {
                            const double wa = wn(in, at[0], at[1], ta), wb = wn(in, at[0], at[1], tb);
                            t->asym = PL_MAX(t->asym, fabs(wa - wb));
                            w.v = 0.5 * (wa + wb);
                            w.vx = 0.5 * (sx[ta] + sx[tb]);
                            w.vy = 0.5 * (sy[ta] - sy[tb]);
                        }
                    }
                    if (w.v != 0.0 || w.vx != 0.0 || w.vy != 0.0)
                        first_row = PL_MIN(first_row, j);
                    frag_put(t, 4 * (size_t) (2 * j + kb), l, e, w);
                }
            }
        }
    }
    if (t->asym > 1e-7) {
        res = MX_ASYM;
        goto done;
    }
    dev_table(t, 0, in->x.fc, in->x.len, &(struct phase_ref) { 1, 0, { 0.5f } });
    dev_table(t, 1, in->y.fc, in->y.len, &(struct phase_ref) { 1, 0, { 0.5f } });
    t->mx.enabled = 2;
    t->mx.org_x = in->x.base[0] - 6;
    t->mx.org_y = in->y.base[0] - 6;
    t->mx.row_first[0] = first_row;
    res = MX_BUILT;
done:
    free(sx);
    free(sy);
    return res;
}

/* ---- all three ----------------------------------------------------------------------------- */

int plh_polar_mx_tables(const struct mx_input *in, struct mx_tables *t)
{
    static enum mx_refusal (*const build[MX_KINDS])(const struct mx_input *, struct mx_tables *) = {
        polar_mx_build, polar_mxr_build, polar_mxd_build,
    };
    enum mx_refusal why[MX_KINDS] = { MX_REFUSED, MX_REFUSED, MX_REFUSED };
    for (int k = 0; k < MX_KINDS; k++) {
        *t = (struct mx_tables) {0};
        why[k] = build[k](in, t);
        if (why[k] == MX_BUILT)
            break;
        // (a kind that gives up half-way leaves nothing behind but the figures of its refusal)
        free(t->blob);
        t->blob = NULL;
        t->mx = (struct plh_polar_mx) {0};
    }
    memcpy(t->why, why, sizeof(why));
    return t->mx.enabled;
}

// Test hook (tests/test_polar_mx_tables.py, CPU): the tables of one captured geometry. Classifies
// both axes itself and returns -1 where that disagrees with the captured classes; else the kind
// (0: every kind refused) with scalars = { ratio, group, sx, sy, org_x, org_y, npairs, row_first[0],
// row_first[1] }, layout = { dfx, dfy, sink (0: none), blob size }, figures = { dev, worst, asym }
// (what the log line of the kind prints) and the blob (-2: over `cap`).
struct plh_test_mx_case {
    int32_t w, h, ncx, ncy, ntaps;
    int32_t bound, tile_fp32, address_mode, transpose, src_w;
    float antiring;
    uint64_t max_shmem_size;
    const float *colfc, *rowfc;
    const int32_t *colbase, *rowbase;
    const float *clsx, *clsy;
    const uint16_t *idx, *idy;
    const uint32_t *taps;
    const float *wall;
};

static bool same_classes(const float *fc, int len, const float *cls, const uint16_t *ids, int ncls)
{
    float *c = malloc((ncls + 1) * sizeof(float));
    uint16_t *id = malloc(len * sizeof(uint16_t));
    const bool same = c && id && plh_classify_axis(fc, len, c, id, ncls + 1) == ncls &&
                      !memcmp(c, cls, ncls * sizeof(float)) && !memcmp(id, ids, len * sizeof(uint16_t));
    free(c);
    free(id);
    return same;
}

PL_API int plh_test_polar_mx_tables(const struct plh_test_mx_case *c, int32_t *scalars,
                                    uint64_t *layout, double *figures, uint8_t *blob, size_t cap);
int plh_test_polar_mx_tables(const struct plh_test_mx_case *c, int32_t *scalars, uint64_t *layout,
                             double *figures, uint8_t *blob, size_t cap)
{
    if (!same_classes(c->colfc, c->w, c->clsx, c->idx, c->ncx) ||
        !same_classes(c->rowfc, c->h, c->clsy, c->idy, c->ncy))
        return -1;
    const struct mx_input in = {
        .x = { c->w, c->colfc, c->colbase, c->idx, c->ncx, c->clsx },
        .y = { c->h, c->rowfc, c->rowbase, c->idy, c->ncy, c->clsy },
        .w = { c->ntaps, c->taps, c->wall },
        .p = { c->bound, c->tile_fp32, c->address_mode, c->transpose, c->src_w, c->antiring,
               c->max_shmem_size },
    };
    struct mx_tables t;
    int kind = plh_polar_mx_tables(&in, &t);
    const struct plh_polar_mx *m = &t.mx;
    const int32_t s[9] = { m->ratio, m->group, m->sx, m->sy, m->org_x, m->org_y, m->npairs,
                           m->row_first[0], m->row_first[1] };
    memcpy(scalars, s, sizeof(s));
    layout[0] = (uintptr_t) m->dfx;
    layout[1] = (uintptr_t) m->dfy;
    layout[2] = (uintptr_t) m->sink;
    layout[3] = kind ? t.size : 0;
    figures[0] = t.dev;
    figures[1] = t.worst;
    figures[2] = t.asym;
    if (kind && t.size > cap)
        kind = -2;
    else if (kind)
        memcpy(blob, t.blob, t.size);
    free(t.blob);
    return kind;
}
