// pq_eotf_pos<true> (libplacebo_amd/csrc/hip/pqseg.hiph: the tier decided on v, ONE product with the
// selected scale) against the formulation it replaces (v * 128, the test on that, `* 64` behind it)
// over ALL 2^32 bit patterns of v: the negative numbers, both zeros, the denormals, +-inf and every NaN
// included. Stand-alone: its own main, no library, no Python.
//   make -f tests/c/eotf_pos_exhaustive.mk && tests/c/build/eotf_pos_exhaustive
// Per pattern three things are compared: the tier, the piece index (the conversion of the position
// that pq_eotf_seg1 makes) and the bits of u (its fract). The old formulation is kept HERE, as the
// reference, written out as it stood; pq_eotf_pos<false>, which the generic chains still compile, is
// held to it as well.
// Prints the mismatch counts on one line and exits 0 only if all are 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pqseg.hiph"

#define CHECK(e)                                                                              \
    do {                                                                                      \
        hipError_t err_ = (e);                                                                \
        if (err_ != hipSuccess) {                                                             \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));                         \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

// the formulation before the change. (noinline: the compiler must not merge the two evaluations)
__device__ __noinline__ float eotf_pos_reference(float v, bool &fine)
{
    const float p = v * 128.0f;
    fine = p < (float) PQSEG_E_SPLIT;
    return fmaxf(fine ? p * (float) (PQSEG_E_LO_N / PQSEG_E_SPLIT) : p, 0.0f);
}

__device__ bool differs(float pos, bool fine, float want, bool want_fine)
{
    // what pq_eotf_seg1 takes from the position: the piece and the local coordinate
    const uint32_t i = (uint32_t) pos, wi = (uint32_t) want;
    const uint32_t u = __builtin_bit_cast(uint32_t, __builtin_amdgcn_fractf(pos));
    const uint32_t wu = __builtin_bit_cast(uint32_t, __builtin_amdgcn_fractf(want));
    return fine != want_fine || i != wi || u != wu;
}

__global__ void __launch_bounds__(256) k_check(unsigned long long *bad)
{
    // 2^20 patterns per block, consecutive patterns in consecutive lanes
    const pq_seg seg = pq_seg_view(nullptr, 0, threadIdx.x & 63u, true);
    unsigned long long b1 = 0, b0 = 0;
    const uint32_t base = blockIdx.x * (1u << 20);
    for (uint32_t i = threadIdx.x; i < (1u << 20); i += 256) {
        const float v = __builtin_bit_cast(float, base + i);
        bool wf, f1, f0;
        const float want = eotf_pos_reference(v, wf);
        const float p1 = pq_eotf_pos<true>(v, seg, f1);
        const float p0 = pq_eotf_pos<false>(v, seg, f0);
        b1 += differs(p1, f1, want, wf);
        b0 += differs(p0, f0, want, wf);
    }
    if (b1) atomicAdd(&bad[0], b1);
    if (b0) atomicAdd(&bad[1], b0);
}

int main()
{
    unsigned long long *d_bad, bad[2];
    CHECK(hipMalloc(&d_bad, sizeof(bad)));
    CHECK(hipMemset(d_bad, 0, sizeof(bad)));
    // 4096 blocks x 2^20 patterns = 2^32: bit patterns 0x00000000 .. 0xffffffff
    hipLaunchKernelGGL(k_check, dim3(4096), dim3(256), 0, 0, d_bad);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_bad));
    printf("EOTF position over 4294967296 bit patterns, mismatches (tier, piece or bits of u) against the "
           "two-product form: pq_eotf_pos<true> %llu, pq_eotf_pos<false> %llu\n", bad[0], bad[1]);
    return bad[0] || bad[1] ? 1 : 0;
}
