/*
 * libplacebo-hip — host tables of the polar (EWA) kernels: what shader_sampling.c (the sampler
 * object), polar_tables.c (phase classes of k_polar_pp, and everything that needs the device) and
 * polar_mx_tables.c (the matrix-pipe blob of k_polar_mx / mxp / mxr / mxd, pure host arithmetic)
 * share.
 */
#ifndef PLH_POLAR_PRIV_H_
#define PLH_POLAR_PRIV_H_

#include "shaders_priv.h"

// Output tile of the polar kernel (csrc/hip/k_polar.hip): 32 columns, 8 lanes
// rows x `rows` rows per lane
#define POLAR_BW 32
#define POLAR_BH 8

// Geometry a set of polar phase-class tables was built for (plh_polar_pp_setup)
struct polar_pp_key {
    float pos[4][2];
    int src_w, src_h, width, height;
    int bound, num_taps, fp32_tile;
    float scale, radius;
    uint64_t filter_gen;
};

// The polar half of a sampler object (struct sh_sampler_obj, shader_sampling.c): what
// pl_shader.polar_obj points at
struct polar_tables {
    pl_buf taps;                    // packed tap list
    uint64_t filter_gen;            // bumped whenever lut/taps are regenerated

    // polar phase classes (k_polar_pp): one device blob holding struct plh_polar_pp
    // and every table it points to
    struct polar_pp_key pp_key;
    int pp_state;                   // 0 = not built, 1 = usable, -1 = not applicable
    pl_buf pp_blob;
    struct plh_polar_pp pp_host;    // host copy (device pointers)
    int pp_tile_w, pp_tile_h, pp_rows, pp_lds_weights;

    // matrix-pipe variant of the same geometry (k_polar_mx): B fragments + tile origin
    pl_buf mx_blob;
    struct plh_polar_mx mx_host;    // .enabled = 0: geometry not eligible
    bool mx_announced;
};

// distinct bit patterns of fc[0..n) -> sorted class values; ids[i] = class of element i
int plh_classify_axis(const float *fc, int n, float *cls, uint16_t *ids, int max_cls);

/* ---- inputs of the matrix-pipe tables (polar_mx_tables.c) -------------------------------- */

// one axis of the pass as the device evaluated it: fcoord and base texel of every output, and
// the phase classes of the fcoords (plh_classify_axis)
struct polar_axis {
    int len;
    const float *fc;
    const int32_t *base;
    const uint16_t *ids;    // [len] class of every output
    int ncls;
    const float *cls;       // [ncls] class values
};

// tap list and wall[ncy][ncx][ntaps + 1]: the weights of every class pair, then scale / wsum
struct polar_weights {
    int ntaps;
    const uint32_t *taps;
    const float *wall;
};

// what eligibility reads of the pass and the device
struct polar_pass {
    int bound, tile_fp32, address_mode, transpose, src_w;
    float antiring;
    size_t max_shmem_size;
};

struct mx_input {
    struct polar_axis x, y;
    struct polar_weights w;
    struct polar_pass p;
};

// why a kind was not built; the caller words it (polar_tables.c: mx_upload)
enum mx_refusal {
    MX_BUILT = 0,
    MX_REFUSED,     // nothing to say: another pass, a tap outside the footprint, no memory
    MX_SHMEM,       // the device's shared memory limit is too small
    MX_PASS,        // kind 1: not this pass
    MX_GEOMETRY,    // no axis of this kind
    MX_NO_HALF,     // kind 2: no output at phase 1/2 exactly
    MX_ASYM,        // kind 2: weights not symmetric about the sample point (`asym`)
};

enum { MX_KINDS = 3 };  // in the order they are tried: 2x, R : G, 2 : 1

struct mx_tables {
    struct plh_polar_mx mx;     // pointer members: byte offsets into `blob` (sink: 0 = none)
    uint8_t *blob;              // malloc'd, NULL unless a kind was built
    size_t size;
    // figures for the log
    float dev;                  // largest per-pixel phase deviation
    double worst, asym;         // weight split error; row asymmetry (kind 2)
    enum mx_refusal why[MX_KINDS];
};

// Tries the three kinds in order. Returns plh_polar_mx.enabled of the one that was built (the
// caller frees t->blob), or 0.
int plh_polar_mx_tables(const struct mx_input *in, struct mx_tables *t);

#endif // PLH_POLAR_PRIV_H_
