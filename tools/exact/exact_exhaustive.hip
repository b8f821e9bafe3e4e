// Exhaustive checks on the GPU of rt_exact.hpp's device forms (v_rcp_f32 / v_sqrt_f32 seeds), the product header itself:
//   root        rtx::sqrt_exact over all 2^32 bit patterns, against __builtin_sqrtf;
//   quotient    rtx::div3 for EVERY denominator mantissa: with the denominator's exponent 0, 4,098 numerators each
//               (structured mantissas -- all-zeros, all-ones and their neighbours, the middle -- and hashed ones,
//               exponents -1 .. 1, both signs, zeros of both signs), then 42 exponent pairs at and beyond both ends
//               of the guard (and at the ends of the exponent range) with 24 numerators each: 4.3 x 10^10 quotients,
//               against `/`;
//   normalize   rtx::normalize_mag over 2^30 hashed vectors across its guard's ends, against sqrtf and `/`;
//   reciprocal  rtx::rcp_small over every float of magnitude <= 2 (zeros, denormals included), against rtd::rcp_ieee.
// Prints one line per check; exit 0 iff none has a mismatch. Built by the Makefile (tools/exact/exact_exhaustive), run
// by tests/test_gpu_exact_forms.py. Test infrastructure only.
#include <cstdint>
#include <cstdio>

#include "hip/rt_device.hpp"  // rt_exact.hpp (rtx::), rtd::rcp_ieee

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// out[0] mismatches, out[1] checked, out[2] first mismatching operand (bits)
__device__ __forceinline__ void tally(unsigned long long* out, unsigned long long bad, unsigned long long n, uint32_t w) {
    // one atomic per wave for the count
    for (int o = 32; o; o >>= 1) {
        n += __shfl_down(n, o);
        bad += __shfl_down(bad, o);
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(out + 1, n);
        if (bad) atomicAdd(out, bad);
    }
    if (w) atomicCAS(out + 2, 0ull, (unsigned long long)w);
}

__global__ void k_root(uint32_t base, unsigned long long* out) {
    const uint32_t bits = base + blockIdx.x * 256u + threadIdx.x;
    const float x = __uint_as_float(bits);
    const bool bad = !same(rtx::sqrt_exact(x), __builtin_sqrtf(x));
    tally(out, bad, 1, bad ? bits : 0u);
}

__global__ void k_rcp(uint32_t base, unsigned long long* out) {
    const uint32_t i = base + blockIdx.x * 256u + threadIdx.x;  // magnitude bits 0 .. 0x40000000, then the sign
    const uint32_t mag = i & 0x7FFFFFFFu;
    const bool in = mag <= 0x40000000u;
    const float x = __uint_as_float(i);
    const bool bad = in && !same(rtx::rcp_small(x), rtd::rcp_ieee(x));
    tally(out, bad, in ? 1 : 0, bad ? (i | 1u) : 0u);
}

__device__ __forceinline__ unsigned check3(rtx::f3 a, float b) {
    const rtx::f3 q = rtx::div3(a, b);
    return (same(q.x, a.x / b) ? 0u : 1u) + (same(q.y, a.y / b) ? 0u : 1u) + (same(q.z, a.z / b) ? 0u : 1u);
}
// numerator i of denominator mantissa m: structured mantissas first, then hashed; the sign and a zero from the hash
__device__ __forceinline__ float numerator(uint32_t m, uint32_t i, int e) {
    const uint32_t h = hash32(m * 4099u + i);
    uint32_t mn;
    if (i < 16u) mn = i & 7u ? (i < 8u ? i : 0x7FFFFFu - (i & 7u)) : (i ? 0x7FFFFFu : 0u);
    else if (i < 24u) mn = 0x400000u + i - 20u;
    else if (i < 32u) mn = m + i - 28u;  // the denominator's own mantissa and its neighbours
    else mn = h >> 9;
    const uint32_t sg = (h & 1u) << 31;
    if ((h & 0x1Eu) == 0u && i >= 32u) return __uint_as_float(sg);  // +-0, one in 16
    return __uint_as_float(sg | (uint32_t)(e + 127) << 23 | (mn & 0x7FFFFFu));
}
__global__ void k_div(unsigned long long* out) {
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;  // every denominator mantissa (grid = 2^23 / 256 blocks)
    unsigned long long bad = 0, n = 0;
    const float b0 = __uint_as_float(127u << 23 | m);
    for (uint32_t i = 0; i < 4098u; i += 3u) {
        const int e = (int)(i % 9u) / 3 - 1;
        bad += check3(rtx::f3{numerator(m, i, e), numerator(m, i + 1u, e), numerator(m, i + 2u, e)}, b0);
        n += 3;
    }
    // at and beyond the guard's ends: the denominator's and the numerators' exponents
    const int de[7] = {-126, -41, -40, 0, 39, 40, 127}, ne[6] = {-126, -51, -50, 49, 50, 127};
    for (int j = 0; j < 7; j++)
        for (int k = 0; k < 6; k++) {
            // (2^40 and 2^50 themselves are the guards' upper ends: mantissa 0 is inside, every other outside)
            const float b = __uint_as_float((uint32_t)(de[j] + 127) << 23 | m);
            for (uint32_t i = 0; i < 24u; i += 3u) {
                const uint32_t s = 5000u + 24u * (uint32_t)(j * 6 + k) + i;
                bad += check3(rtx::f3{numerator(m, i, ne[k]), numerator(m, s + 1u, ne[k]), numerator(m, s + 2u, ne[k])}, b);
                n += 3;
            }
        }
    // a negative denominator, a zero one
    bad += check3(rtx::f3{numerator(m, 40u, 0), numerator(m, 41u, 1), -0.0f}, -b0);
    bad += check3(rtx::f3{numerator(m, 42u, 0), 0.0f, -0.0f}, 0.0f);
    n += 6;
    tally(out, bad, n, bad ? (m | 0x80000000u) : 0u);
}

__global__ void k_norm(unsigned long long* out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // 2^22 threads x 256 vectors
    unsigned long long bad = 0;
    for (uint32_t i = 0; i < 256u; i++) {
        const uint32_t h = hash32(t * 256u + i);
        // the components' common scale across both ends of [2^-32, 2^32]; one in 8 vectors has mixed scales or a zero
        const int e0 = -36 + (int)(h % 73u);
        float c[3];
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t g = hash32(h + 0x9E3779B9u * (k + 1u));
            int e = e0 - (int)(g >> 30);
            if ((h >> 8 & 7u) == 0u) e = -40 + (int)(g >> 24) % 81;
            c[k] = __uint_as_float((g & 1u) << 31 | (uint32_t)(e + 127) << 23 | (g >> 1 & 0x7FFFFFu));
            if ((h >> 11 & 63u) == k) c[k] = 0.0f;
        }
        float mg;
        const rtx::f3 a{c[0], c[1], c[2]}, q = rtx::normalize_mag(a, mg);
        const float s = __builtin_sqrtf(a.x * a.x + a.y * a.y + a.z * a.z);
        bad += !(same(mg, s) && same(q.x, a.x / s) && same(q.y, a.y / s) && same(q.z, a.z / s));
    }
    tally(out, bad, 256, bad ? (t | 1u) : 0u);
}

int main() {
    unsigned long long* out;  // [check][mismatches, checked, first]
    if (hipMalloc(&out, 4 * 3 * 8) != hipSuccess || hipMemset(out, 0, 4 * 3 * 8) != hipSuccess) { printf("hip error\n"); return 2; }
    const uint32_t chunk = 1u << 28;
    for (uint64_t b = 0; b < (1ull << 32); b += chunk) {
        k_root<<<chunk / 256, 256>>>((uint32_t)b, out);
        k_rcp<<<chunk / 256, 256>>>((uint32_t)b, out + 9);
    }
    k_div<<<(1u << 23) / 256, 256>>>(out + 3);
    k_norm<<<(1u << 22) / 256, 256>>>(out + 6);
    if (hipDeviceSynchronize() != hipSuccess) { printf("hip error\n"); return 2; }
    unsigned long long h[12];
    if (hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { printf("hip error\n"); return 2; }
    const char* name[4] = {"root", "quotient", "normalize", "rcp_small"};
    int rc = 0;
    for (int i = 0; i < 4; i++) {
        printf("%s mismatches %llu of %llu", name[i], h[3 * i], h[3 * i + 1]);
        if (h[3 * i]) printf(" (first at 0x%08llx)", h[3 * i + 2]);
        printf("\n");
        if (h[3 * i] || !h[3 * i + 1]) rc = 1;
    }
    return rc;
}
