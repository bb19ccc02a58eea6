// plh_sqrt_n / plh_sqrt_core (libplacebo_amd/csrc/hip/devmath.hiph) against __builtin_sqrtf over ALL
// 2^31 non-negative bit patterns (zero, the denormals, every normal number, +inf, the positive NaNs),
// bit for bit. Stand-alone: its own main, no library, no Python.
//   make -f tests/c/sqrt_exhaustive.mk && tests/c/build/sqrt_exhaustive
// Three results per pattern are compared with the compiler's own expansion:
//   n1    plh_sqrt_n<1>: the wave takes the short form or the expansion, as the colour map does
//   n2    plh_sqrt_n<2> with the pattern beside 1.0f (a second value that never asks for the expansion)
//   core  plh_sqrt_core alone, counted only where plh_sqrt_n may use it (x >= 2^-96, +inf included)
// Prints the three mismatch counts and exits 0 only if all are 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "devmath.hiph"

#define CHECK(e)                                                                              \
    do {                                                                                      \
        hipError_t err_ = (e);                                                                \
        if (err_ != hipSuccess) {                                                             \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));                         \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

// the compiler must not see through to a constant or merge the two evaluations
__device__ __noinline__ float sqrt_builtin(float x) { return __builtin_sqrtf(x); }

__global__ void __launch_bounds__(256) k_check(uint32_t first, unsigned long long *bad)
{
    // 2^20 patterns per block: consecutive patterns in consecutive lanes, so that waves near 2^-96
    // hold arguments of both kinds (the uniform branch of plh_sqrt_n goes both ways)
    unsigned long long b1 = 0, b2 = 0, bc = 0;
    const uint32_t base = first + blockIdx.x * (1u << 20);
    for (uint32_t i = threadIdx.x; i < (1u << 20); i += 256) {
        const uint32_t bits = base + i;
        const float x = __builtin_bit_cast(float, bits);
        const uint32_t want = __builtin_bit_cast(uint32_t, sqrt_builtin(x));
        float a[1] = { x };
        plh_sqrt_n(a);
        b1 += __builtin_bit_cast(uint32_t, a[0]) != want;
        float b[2] = { x, 1.0f };
        plh_sqrt_n(b);
        b2 += __builtin_bit_cast(uint32_t, b[0]) != want || b[1] != 1.0f;
        if (x >= 0x1p-96f)
            bc += __builtin_bit_cast(uint32_t, plh_sqrt_core(x)) != want;
    }
    if (b1) atomicAdd(&bad[0], b1);
    if (b2) atomicAdd(&bad[1], b2);
    if (bc) atomicAdd(&bad[2], bc);
}

int main()
{
    unsigned long long *d_bad, bad[3];
    CHECK(hipMalloc(&d_bad, sizeof(bad)));
    CHECK(hipMemset(d_bad, 0, sizeof(bad)));
    // 2048 blocks x 2^20 patterns = 2^31: bit patterns 0x00000000 .. 0x7fffffff
    hipLaunchKernelGGL(k_check, dim3(2048), dim3(256), 0, 0, 0u, d_bad);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_bad));
    printf("sqrt over 2147483648 non-negative bit patterns, mismatches against __builtin_sqrtf: "
           "plh_sqrt_n<1> %llu, plh_sqrt_n<2> %llu, plh_sqrt_core (x >= 2^-96) %llu\n",
           bad[0], bad[1], bad[2]);
    return bad[0] || bad[1] || bad[2] ? 1 : 0;
}
