/*
 * libplacebo-hip — tables of the polar (EWA) kernels that are built once per geometry, at launch
 * time, and everything about them that needs the device: the phase classes of k_polar_pp (device
 * side: k_polar.hip, struct plh_polar_pp) and the upload of the matrix-pipe blob that
 * polar_mx_tables.c computes from them.
 */
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "polar_priv.h"


static int cmp_u32(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *) a, y = *(const uint32_t *) b;
    return x < y ? -1 : x > y;
}

int plh_classify_axis(const float *fc, int n, float *cls, uint16_t *ids, int max_cls)
{
    uint32_t *tmp = malloc(n * sizeof(uint32_t));
    if (!tmp)
        return -1;
    memcpy(tmp, fc, n * sizeof(uint32_t));
    qsort(tmp, n, sizeof(uint32_t), cmp_u32);
    int nc = 0;
    for (int i = 0; i < n; i++) {
        if (i && tmp[i] == tmp[i - 1])
            continue;
        if (nc == max_cls) {
            free(tmp);
            return -1;
        }
        memcpy(&cls[nc++], &tmp[i], 4);
    }
    free(tmp);
    for (int i = 0; i < n; i++) {
        uint32_t key;
        memcpy(&key, &fc[i], 4);
        int lo = 0, hi = nc - 1;
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            uint32_t v;
            memcpy(&v, &cls[mid], 4);
            if (v < key)
                lo = mid + 1;
            else
                hi = mid;
        }
        ids[i] = lo;
    }
    return nc;
}

// Can `n` consecutive outputs [n*c - pad, n*c - pad + n) always share a base texel?
static bool cells_share_base(const int32_t *base, int len, int n, int pad)
{
    for (int c0 = -pad; c0 < len; c0 += n) {
        int b = 0;
        bool have = false;
        for (int i = 0; i < n; i++) {
            const int x = c0 + i;
            if (x < 0 || x >= len)
                continue;
            if (have && base[x] != b)
                return false;
            b = base[x];
            have = true;
        }
    }
    return true;
}

struct axis_tiles {
    int ntiles;
    uint8_t *loc;       // [len]
    uint16_t *list;     // [ntiles][PLH_PP_LMAX]
    uint8_t *cnt;       // [ntiles]
    int32_t *org;       // [ntiles]
    int extent;         // LDS tile extent needed along this axis (texels)
    int max_cnt;
};

// Split an axis of `len` outputs into tiles of `tile_cells` cells of `n` outputs
static bool build_axis_tiles(struct axis_tiles *t, const uint16_t *ids, const int32_t *base,
                             int len, int n, int pad, int tile_cells, int bound)
{
    const int cells = (len + pad + n - 1) / n;
    t->ntiles = (cells + tile_cells - 1) / tile_cells;
    t->loc = calloc(len, 1);
    t->list = calloc((size_t) t->ntiles * PLH_PP_LMAX, sizeof(uint16_t));
    t->cnt = calloc(t->ntiles, 1);
    t->org = calloc(t->ntiles, sizeof(int32_t));
    t->extent = 0;
    t->max_cnt = 0;
    if (!t->loc || !t->list || !t->cnt || !t->org)
        return false;
    for (int ti = 0; ti < t->ntiles; ti++) {
        const int x0 = PL_MAX(ti * tile_cells * n - pad, 0);
        const int x1 = PL_MIN((ti + 1) * tile_cells * n - pad, len);
        uint16_t *list = t->list + (size_t) ti * PLH_PP_LMAX;
        int cnt = 0, bmin = INT32_MAX, bmax = INT32_MIN;
        for (int x = x0; x < x1; x++) {
            int l = 0;
            while (l < cnt && list[l] != ids[x])
                l++;
            if (l == cnt) {
                if (cnt == PLH_PP_LMAX)
                    return false;
                list[cnt++] = ids[x];
            }
            t->loc[x] = l;
            bmin = PL_MIN(bmin, base[x]);
            bmax = PL_MAX(bmax, base[x]);
        }
        if (x1 <= x0) {
            bmin = bmax = 0;
            cnt = 1;
        }
        t->cnt[ti] = cnt;
        t->max_cnt = PL_MAX(t->max_cnt, cnt);
        // taps span [base - (bound-1), base + bound]; one texel of slack per side for the
        // rare pixel whose own base is off by one (per-pixel path inside k_polar_pp)
        t->org[ti] = bmin - (bound - 1) - 1;
        t->extent = PL_MAX(t->extent, bmax - bmin + 2 * bound + 2);
    }
    return true;
}

static void free_axis_tiles(struct axis_tiles *t)
{
    free(t->loc);
    free(t->list);
    free(t->cnt);
    free(t->org);
    memset(t, 0, sizeof(*t));
}

static inline size_t align16(size_t x)
{
    return (x + 15) & ~(size_t) 15;
}

int plh_launch_polar_classify(plh_stream stream, const struct plh_pass *pass, void *out);
int plh_launch_polar_weights(plh_stream stream, const struct plh_pass *pass, const float *clsx,
                             int ncx, const float *clsy, int ncy, float *weights);


// The matrix-pipe tables of the geometry (polar_mx_tables.c), where one of the kinds has its shape:
// the blob goes to the device, its offsets become pointers. obj->mx_host.enabled = 0 otherwise.
static void mx_upload(pl_gpu gpu, pl_log log, struct polar_tables *obj, const struct mx_input *in)
{
    struct mx_tables t;
    obj->mx_host = (struct plh_polar_mx) {0};
    const int kind = plh_polar_mx_tables(in, &t);
    const struct polar_pass *p = &in->p;
    // (what every kind that was tried, in that order, has to say for itself)
    if (t.why[0] == MX_SHMEM) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe polar: needs 64 KiB of shared memory, the limit is %zu",
               p->max_shmem_size);
    } else if (t.why[0] == MX_PASS) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe polar: not this pass (bound %d, fp32 tile %d, address "
               "mode %d, transpose %d, antiring %g)", p->bound, p->tile_fp32, p->address_mode,
               p->transpose, p->antiring);
    } else if (t.why[0] == MX_GEOMETRY) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe polar: not an exact 2x geometry");
    }
    if (t.why[1] == MX_GEOMETRY)
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe polar: not an exact 3x / 4x / 3 : 2 geometry either");
    if (t.why[2] == MX_SHMEM) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe downscale: needs 124 KiB of shared memory, the limit is %zu",
               p->max_shmem_size);
    } else if (t.why[2] == MX_NO_HALF) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe downscale: no output at phase 1/2 exactly");
    } else if (t.why[2] == MX_ASYM) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe downscale: weights not symmetric about the sample "
               "point (%.2e)", t.asym);
    }
    if (!kind)
        return;

    pl_buf_destroy(gpu, &obj->mx_blob);
    obj->mx_blob = pl_buf_create(gpu, pl_buf_params(.size = t.size, .storable = true,
                                                    .initial_data = t.blob));
    free(t.blob);
    if (!obj->mx_blob)
        return;
    const char *base = pl_hip_buf_ptr(obj->mx_blob);
    obj->mx_host = t.mx;
    obj->mx_host.bfrag = base;
    obj->mx_host.dfx = (const float *) (base + (size_t) t.mx.dfx);
    obj->mx_host.dfy = (const float *) (base + (size_t) t.mx.dfy);
    obj->mx_host.sink = t.mx.sink ? (void *) (base + (size_t) t.mx.sink) : NULL;
    obj->mx_announced = false;
    const struct plh_polar_mx *m = &t.mx;
    if (kind == 1) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe tables for the polar pass: 2 x 2 phases (fcoord %.6f %.6f / %.6f %.6f, "
               "per-pixel phases within %.2e: first-order terms), %d row pairs per phase from tile rows %d / %d, "
               "weight split error <= %.2e", in->x.fc[0], in->x.fc[1], in->y.fc[0], in->y.fc[1], t.dev,
               m->npairs, m->row_first[0], m->row_first[1], t.worst);
    } else if (kind == 3) {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe tables for the polar pass: %d x %d phases (%d : %d upscale, shifts %d / %d, "
               "per-pixel phases within %.2e: first-order terms), weight split error <= %.2e",
               m->ratio, m->ratio, m->ratio, m->group, m->sx, m->sy, t.dev, t.worst);
    } else {
        pl_msg(log, PL_LOG_DEBUG, "matrix-pipe tables for the polar pass: 2 : 1 downscale, one phase (1/2, 1/2), "
               "per-pixel phases within %.2e: first-order terms; row symmetry %.1e, weight split error <= %.2e",
               t.dev, t.asym, t.worst);
    }
}

static bool polar_pp_build(pl_gpu gpu, pl_log log, struct polar_tables *obj,
                           const struct plh_pass *pass)
{
    const struct plh_sampler_args *s = &pass->s;
    const int W = pass->width, H = pass->height, ntaps = s->num_taps;
    const plh_stream stream = plh_gpu_stream(gpu);
    bool ok = false;
    pl_buf tmp = NULL, wbuf = NULL;
    float *host = NULL, *clsx = NULL, *clsy = NULL, *wall = NULL;
    uint16_t *idx = NULL, *idy = NULL;
    uint8_t *blob = NULL;
    struct axis_tiles tx = {0}, ty = {0};
    enum { MAX_CLS = 96 };

    // ---- 1. fcoord / base of every column and row, evaluated by the device ------------------
    const size_t cls_bytes = (size_t) 2 * (W + H) * 4;
    tmp = pl_buf_create(gpu, pl_buf_params(.size = cls_bytes, .storable = true,
                                           .host_readable = true));
    host = malloc(cls_bytes);
    clsx = malloc(MAX_CLS * sizeof(float));
    clsy = malloc(MAX_CLS * sizeof(float));
    idx = malloc(W * sizeof(uint16_t));
    idy = malloc(H * sizeof(uint16_t));
    if (!tmp || !host || !clsx || !clsy || !idx || !idy)
        goto done;
    if (plh_launch_polar_classify(stream, pass, pl_hip_buf_ptr(tmp)) ||
        !plh_buf_read(gpu, tmp, 0, host, cls_bytes))
        goto done;
    const float *colfc = host, *rowfc = host + 2 * W;
    const int32_t *colbase = (const int32_t *) (host + W);
    const int32_t *rowbase = (const int32_t *) (host + 2 * W + H);

    // ---- 2. classes ---------------------------------------------------------------------------
    const int ncx = plh_classify_axis(colfc, W, clsx, idx, MAX_CLS);
    const int ncy = plh_classify_axis(rowfc, H, clsy, idy, MAX_CLS);
    if (ncx < 0 || ncy < 0) {
        // arbitrary (non-rational) ratio: every column has its own phase
        pl_msg(log, PL_LOG_DEBUG, "polar phase classes: more than %d distinct phases per axis "
               "(%dx%d outputs)", MAX_CLS, W, H);
        goto done;
    }

    // ---- 3. outputs per lane: 2x2 when pairs of outputs share their base texel --------------
    int n = 1, padx = 0, pady = 0;
    for (int px = 0; px < 2 && n == 1; px++) {
        if (!cells_share_base(colbase, W, 2, px))
            continue;
        for (int py = 0; py < 2; py++) {
            if (cells_share_base(rowbase, H, 2, py)) {
                n = 2; padx = px; pady = py;
                break;
            }
        }
    }

    // ---- 4. tiles: 32 x 8*rows cells, LDS = lut + weights + source tile ----------------------
    const size_t texel = s->tile_fp32 ? 16 : 8;
    const size_t max_lds = 64 * 1024;   // >= 2 workgroups per CU
    int rows = n == 2 ? 3 : 4, tp = 0, ntc = 0;    // (measured: 3 beats 4 by ~2 % for 2x2 cells)
    const int rows_forced = plh_switch(PLH_SW_PP_ROWS);     // profiling aid
    if (rows_forced > 0)
        rows = PL_MIN(rows_forced, 8);
    rows = PL_MIN(rows, 64 / (POLAR_BH * n));   // the kernel stages <= 64 output rows of info
    // a small output (the chroma planes of 1080p video: 1920 x 1080 = 690 workgroups at 3 rows) does
    // not fill 256 CUs twice with such tiles, and the kernel lives on latency hiding: fewer rows
    // per workgroup until there are two rounds of them (NV12 1080p -> 4K, the chroma pass:
    // 37.5 -> 26.2 us, profiles/r04_49_pp_rows_small.txt)
    if (rows_forced <= 0) {
        while (rows > 1 && (size_t) ((W + POLAR_BW * n - 1) / (POLAR_BW * n)) *
                           (size_t) ((H + POLAR_BH * rows * n - 1) / (POLAR_BH * rows * n)) < 1024)
            rows--;
    }
    size_t lds_w = 0;
    for (;; rows >>= 1) {
        free_axis_tiles(&tx);
        free_axis_tiles(&ty);
        if (!build_axis_tiles(&tx, idx, colbase, W, n, padx, POLAR_BW, s->bound) ||
            !build_axis_tiles(&ty, idy, rowbase, H, n, pady, POLAR_BH * rows, s->bound))
            goto done;
        // worst-case weights slice; the compacted tap count is only known later
        lds_w = align16((size_t) tx.max_cnt * ty.max_cnt * (ntaps + 4) * 4) + align16(ntaps * 4);
        if (2048 + 1024 + 64 + lds_w + (size_t) tx.extent * ty.extent * texel <= max_lds)
            break;
        if (rows == 1)
            goto done;
    }

    // ---- 5. weights of every class pair, by the device; compaction of dead taps -------------
    const size_t wall_bytes = (size_t) ncx * ncy * (ntaps + 1) * 4;
    wbuf = pl_buf_create(gpu, pl_buf_params(.size = wall_bytes + (ncx + ncy) * 4, .storable = true,
                                            .host_readable = true, .host_writable = true));
    wall = malloc(wall_bytes);
    if (!wbuf || !wall)
        goto done;
    plh_buf_write(gpu, wbuf, wall_bytes, clsx, ncx * 4);
    plh_buf_write(gpu, wbuf, wall_bytes + ncx * 4, clsy, ncy * 4);
    const float *dcls = (const float *) ((const char *) pl_hip_buf_ptr(wbuf) + wall_bytes);
    if (plh_launch_polar_weights(stream, pass, dcls, ncx, dcls + ncx, ncy, pl_hip_buf_ptr(wbuf)) ||
        !plh_buf_read(gpu, wbuf, 0, wall, wall_bytes))
        goto done;

    uint32_t *taps_all = malloc(PL_MAX(ntaps, 1) * sizeof(uint32_t));
    int *keep = malloc(PL_MAX(ntaps, 1) * sizeof(int));
    if (!taps_all || !keep || !plh_buf_read(gpu, obj->taps, 0, taps_all, ntaps * sizeof(uint32_t))) {
        free(taps_all);
        free(keep);
        goto done;
    }
    for (int t = 0; t < ntaps; t++) {
        bool used = false;
        for (int pr = 0; pr < ncx * ncy && !used; pr++)
            used = wall[(size_t) pr * (ntaps + 1) + t] != 0.0f;
        if (used)
            keep[ntc++] = t;
    }
    tp = (ntc + 1 + 3) & ~3;    // weights + norm, padded to 16 bytes
    // + the compacted tap offsets, staged at the tail of this area (k_polar_pp)
    lds_w = align16((size_t) tx.max_cnt * ty.max_cnt * tp * 4) + align16(ntc * 4);

    // ---- 6. one device blob: struct + tables ---------------------------------------------------
    size_t off = align16(sizeof(struct plh_polar_pp));
#define PLACE(name, bytes) const size_t o_##name = off; off = align16(off + (bytes))
    PLACE(colfc, (size_t) W * 4);   PLACE(rowfc, (size_t) H * 4);
    PLACE(colbase, (size_t) W * 4); PLACE(rowbase, (size_t) H * 4);
    PLACE(colloc, W);               PLACE(rowloc, H);
    PLACE(collist, (size_t) tx.ntiles * PLH_PP_LMAX * 2);
    PLACE(rowlist, (size_t) ty.ntiles * PLH_PP_LMAX * 2);
    PLACE(coln, (size_t) tx.ntiles * 4); PLACE(rown, (size_t) ty.ntiles * 4);
    PLACE(colorg, (size_t) tx.ntiles * 4); PLACE(roworg, (size_t) ty.ntiles * 4);
    PLACE(weights, (size_t) ncx * ncy * tp * 4);
    PLACE(tapoff, (size_t) PL_MAX(ntc, 1) * 4);
    PLACE(tilemap, (size_t) tx.ntiles * ty.ntiles * 4);
#undef PLACE
    blob = calloc(1, off);
    if (!blob) {
        free(taps_all);
        free(keep);
        goto done;
    }
    memcpy(blob + o_colfc, colfc, (size_t) W * 4);
    memcpy(blob + o_rowfc, rowfc, (size_t) H * 4);
    memcpy(blob + o_colbase, colbase, (size_t) W * 4);
    memcpy(blob + o_rowbase, rowbase, (size_t) H * 4);
    memcpy(blob + o_colloc, tx.loc, W);
    memcpy(blob + o_rowloc, ty.loc, H);
    memcpy(blob + o_collist, tx.list, (size_t) tx.ntiles * PLH_PP_LMAX * 2);
    memcpy(blob + o_rowlist, ty.list, (size_t) ty.ntiles * PLH_PP_LMAX * 2);
    for (int i = 0; i < tx.ntiles; i++)
        ((int32_t *) (blob + o_coln))[i] = tx.cnt[i];
    for (int i = 0; i < ty.ntiles; i++)
        ((int32_t *) (blob + o_rown))[i] = ty.cnt[i];
    memcpy(blob + o_colorg, tx.org, (size_t) tx.ntiles * 4);
    memcpy(blob + o_roworg, ty.org, (size_t) ty.ntiles * 4);
    float *wc = (float *) (blob + o_weights);
    for (int pr = 0; pr < ncx * ncy; pr++) {
        const float *src = wall + (size_t) pr * (ntaps + 1);
        float *dst = wc + (size_t) pr * tp;
        for (int k = 0; k < ntc; k++)
            dst[k] = src[keep[k]];
        dst[ntc] = src[ntaps];      // scale / wsum
    }
    int32_t *tapoff = (int32_t *) (blob + o_tapoff);
    for (int k = 0; k < ntc; k++) {
        const uint32_t tap = taps_all[keep[k]];
        const int x = (int8_t) (tap & 0xff), y = (int8_t) ((tap >> 8) & 0xff);
        tapoff[k] = (y * tx.extent + x) * (int) texel;
    }
    // the same geometry on the matrix pipe, where it has the shape for it
    mx_upload(gpu, log, obj, &(struct mx_input) {
        .x = { W, colfc, colbase, idx, ncx, clsx },
        .y = { H, rowfc, rowbase, idy, ncy, clsy },
        .w = { ntaps, taps_all, wall },
        .p = { s->bound, s->tile_fp32, s->address_mode, pass->transpose, s->src.w, s->antiring,
               gpu->glsl.max_shmem_size },
    });
    free(taps_all);
    free(keep);

    // XCD-aware launch order: workgroups go to the 8 XCDs round-robin, each XCD has its own L2;
    // XCD x gets the x-th contiguous eighth of the tiles so that neighbours share halo texels
    const uint32_t gx = tx.ntiles, total = (uint32_t) tx.ntiles * ty.ntiles;
    const bool remap = n == 2 && tx.ntiles <= 0xffff && ty.ntiles <= 0xffff;
    if (remap) {
        uint32_t *tm = (uint32_t *) (blob + o_tilemap);
        const uint32_t q = total / 8, r = total % 8;
        for (uint32_t lin = 0; lin < total; lin++) {
            const uint32_t xcd = lin % 8, k = lin / 8;
            const uint32_t tile = xcd * q + PL_MIN(xcd, r) + k;
            tm[lin] = (tile % gx) | ((tile / gx) << 16);
        }
    }

    pl_buf_destroy(gpu, &obj->pp_blob);
    obj->pp_blob = pl_buf_create(gpu, pl_buf_params(.size = off, .storable = true,
                                                    .host_writable = true));
    if (!obj->pp_blob)
        goto done;
    const char *d = pl_hip_buf_ptr(obj->pp_blob);
    struct plh_polar_pp *pp = &obj->pp_host;
    *pp = (struct plh_polar_pp) {
        .n = n, .padx = padx, .pady = pady,
        .cells_w = (W + padx + n - 1) / n, .cells_h = (H + pady + n - 1) / n,
        .ncx = ncx, .ncy = ncy, .ntaps = ntc, .tp = tp,
        .colfc = (const float *) (d + o_colfc), .rowfc = (const float *) (d + o_rowfc),
        .colbase = (const int32_t *) (d + o_colbase), .rowbase = (const int32_t *) (d + o_rowbase),
        .colloc = (const uint8_t *) (d + o_colloc), .rowloc = (const uint8_t *) (d + o_rowloc),
        .collist = (const uint16_t *) (d + o_collist), .rowlist = (const uint16_t *) (d + o_rowlist),
        .coln = (const int32_t *) (d + o_coln), .rown = (const int32_t *) (d + o_rown),
        .colorg = (const int32_t *) (d + o_colorg), .roworg = (const int32_t *) (d + o_roworg),
        .weights = (const float *) (d + o_weights), .tapoff = (const int32_t *) (d + o_tapoff),
        .tilemap = remap ? (const uint32_t *) (d + o_tilemap) : NULL,
    };
    memcpy(blob, pp, sizeof(*pp));
    plh_buf_write(gpu, obj->pp_blob, 0, blob, off);

    obj->pp_tile_w = tx.extent;
    obj->pp_tile_h = ty.extent;
    obj->pp_rows = rows;
    obj->pp_lds_weights = lds_w;
    pl_msg(log, PL_LOG_DEBUG, "polar phase classes: %dx%d classes, %d/%d live taps, %dx%d px per "
           "lane, tile %dx%d, %d rows, %zu B of weights in LDS", ncx, ncy, ntc, ntaps, n, n,
           tx.extent, ty.extent, rows, lds_w);
    ok = true;

done:
    pl_buf_destroy(gpu, &tmp);
    pl_buf_destroy(gpu, &wbuf);
    free_axis_tiles(&tx);
    free_axis_tiles(&ty);
    free(host); free(clsx); free(clsy); free(idx); free(idy); free(wall); free(blob);
    return ok;
}

void plh_polar_pp_setup(pl_gpu gpu, pl_log log, void *polar_obj, struct plh_pass *pass)
{
    struct polar_tables *obj = polar_obj;
    struct plh_sampler_args *s = &pass->s;
    s->pp = NULL;
    memset(&s->mx, 0, sizeof(s->mx));
    if (plh_switch(PLH_SW_POLAR_PER_PIXEL))
        return;
    const uint32_t cm = s->comp_mask & 0xf;
    if (cm != 0x7 && cm != 0xf && cm != 0x1 && cm != 0x3)
        return; // k_polar_pp is instantiated for RGB / RGBA and for 1- / 2-component planes

    struct polar_pp_key key = {
        .src_w = s->src.w, .src_h = s->src.h, .width = pass->width, .height = pass->height,
        .bound = s->bound, .num_taps = s->num_taps, .fp32_tile = s->tile_fp32,
        .scale = s->scale, .radius = s->radius, .filter_gen = obj->filter_gen,
    };
    memcpy(key.pos, s->pos, sizeof(key.pos));
    if (!obj->pp_state || memcmp(&key, &obj->pp_key, sizeof(key))) {
        obj->pp_key = key;
        obj->pp_state = polar_pp_build(gpu, log, obj, pass) ? 1 : -1;
        if (obj->pp_state < 0)
            pl_msg(log, PL_LOG_DEBUG, "polar phase classes not applicable to this geometry; "
                   "using per-pixel weights");
    }
    if (obj->pp_state != 1)
        return;

    s->pp = pl_hip_buf_ptr(obj->pp_blob);
    s->ppv = obj->pp_host;
    s->pp_n = obj->pp_host.n;
    s->pp_cells_w = obj->pp_host.cells_w;
    s->pp_cells_h = obj->pp_host.cells_h;
    s->pp_lds_weights = obj->pp_lds_weights;
    s->pp_debug = plh_switch(PLH_SW_PP_DEBUG);
    s->tile_w = obj->pp_tile_w;
    s->tile_h = obj->pp_tile_h;
    s->tile_rows = obj->pp_rows;

    // k_polar_mx: the contraction on the f16 matrix pipe, within +-1 code of 16 bits of the
    // sequential-fma kernels. PL_HIP_POLAR_MFMA=0 keeps the bit-exact reference variant.
    // That bound holds behind EVERY epilogue, the ones that amplify near black included -- a pass
    // that scales in linear / sigmoidized light continues with UNSIGMOIDIZE (slope up to 17 at
    // the dark end) and DELINEARIZE ((1 / 2.4) x^-0.58) -- because the contraction's error scales
    // with the taps' products, which are small where the output is dark: measured <= 1 code at
    // 1080p -> 4K on white noise and on a dark field with isolated full-scale texels
    // (tests/test_gpu_default_kernels.py::test_matrix_pipe_behind_sigmoid_measured).
    memset(&s->mx, 0, sizeof(s->mx));
    if (obj->mx_host.enabled && plh_switch(PLH_SW_POLAR_MFMA) && (cm == 0x7 || cm == 0xf) &&
        !pass->transpose && s->address_mode == PLH_ADDRESS_CLAMP) {
        s->mx = obj->mx_host;
        if (!obj->mx_announced)
            pl_msg(log, PL_LOG_DEBUG, "polar on the matrix pipe (%s)",
                   s->mx.enabled == 2 ? "k_polar_mxd, where the pass has its shape" :
                   s->mx.enabled == 3 ? "k_polar_mxr, where the pass has its shape" : "k_polar_mx");
        obj->mx_announced = true;
    }
}
