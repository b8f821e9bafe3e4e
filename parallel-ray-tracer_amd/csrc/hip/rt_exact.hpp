// rt_exact.hpp — short forms of the correctly rounded fp32 division and square root for the code around the walks
// (ray formation, shading, level setup), kept free of HIP so that tests/c/exact_forms_test.cpp can check the host
// forms with g++ alone; the kernels call the same functions (tools/exact/exact_exhaustive.hip checks the device forms).
//
// The build keeps IEEE `/` and sqrtf (-fhip-fp32-correctly-rounded-divide-sqrt). The compiler's division is
// v_div_scale x2, v_rcp, five FMAs, v_div_fmas, v_div_fixup (about 12 instructions per quotient); its root is about 25.
// Most divisions of the shading code come three to a denominator (a vec_t divided by a length), with operands far from
// the ends of the exponent range, where the scaling and the fix-up do nothing. Every function here returns the bits
// of the `/` or sqrtf it replaces FOR EVERY INPUT: inside a guard range the short form, outside it the operation itself.
//
//   reciprocal  y = RN(1 / b): v_rcp_f32 (1 ulp) and one FMA correction, rtd::rcp_ieee's three instructions, checked
//               for every normal float below 2^126 (tools/rcp/rcp_exhaustive). Host: 1.0f / b.
//   quotient    q0 = RN(a y); r = a - b q0 (one FMA, exact); q = RN(q0 + r y): Markstein's correction of a quotient by a
//               correctly rounded reciprocal. Three numerators share y.
//               The residual is formed as -fma(b, q0, -a): the same value for a != 0, and for a = +-0 and b > 0 it is
//               -0, so that q = fma(-0, y, +-0) keeps the numerator's sign (fma(-b, q0, a) gives +0 and turns -0 / b
//               into +0). This is why the guard wants b > 0; every denominator of the shading code is a length or a
//               squared length.
//   root        s = v_sqrt_f32(x) (1 ulp), then the choice among s - 1 ulp, s, s + 1 ulp by the signs of two FMA
//               residuals x - (s - 1 ulp) s and x - (s + 1 ulp) s: the compiler's own sequence without its scaling and
//               class handling. Any seed within 1 ulp of the correctly rounded root gives the correctly rounded root.
//
// Guard ranges (v_div_scale_f32 scales when the denominator or the quotient nears the denormals or the exponents differ
// by 96 or more; inside the ranges below none of that happens and no intermediate under- or overflows):
//   denominator b in [2^-40, 2^40] (positive; a NaN fails the comparison), so y = RN(1 / b) is in [2^-40, 2^40];
//   numerator   a = +-0, or |a| in [2^-50, 2^50]: q0 and q lie in [2^-91, 2^91], normal; r = a - b q0 is a multiple of
//               ulp(b) ulp(q0) >= 2^-46 |a| / 4 >= 2^-98, far above the smallest denormal 2^-149, and |r| <= ulp(q0) b,
//               so the FMA forms it exactly whenever q0 is within an ulp of the quotient (no mismatch in 4 x 10^10
//               device and 6 x 10^9 host quotients);
//   root        x in [2^-64, 2^66]: the compiler's sequence scales only below 2^-96 (where the residuals' low bits
//               ulp(s)^2 would leave the denormals); s (s + 1 ulp) stays far below overflow.
//   normalize   every |a_i| in [2^-32, 2^32] and the root at most 2^33: then x = a.a is in [2^-64, 3 2^64], inside the
//               root's range, and the three quotients' operands are inside theirs. One comparison of min |a_i| and one of
//               the root's seed (a NaN component makes the seed NaN and fails it). A zero component takes the fallback.
// Zeros pass the quotient's guard (a light in shadow multiplies its contribution by 0: the common case of the `/ mg`
// triples); denormals, infinities and NaNs fail it and take `/`.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_HD __host__ __device__ __forceinline__
#else
#define RTX_HD inline
#endif

namespace rtx {

struct f3 {
    float x, y, z;
};

constexpr float DEN_LO = 0x1p-40f, DEN_HI = 0x1p40f;  // quotient: the denominator's range
constexpr float NUM_LO = 0x1p-50f, NUM_HI = 0x1p50f;  // quotient: a nonzero numerator's range
constexpr float ROOT_LO = 0x1p-64f, ROOT_HI = 0x1p66f;
constexpr float NRM_LO = 0x1p-32f, NRM_HI = 0x1p33f;  // normalize: the components' lower end, the root's upper end

RTX_HD std::uint32_t bits_of(float x) {
    std::uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
RTX_HD float float_of(std::uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// RN(1 / b) for a normal |b| < 2^126 without a branch (device: 3 instructions; rtd::rcp_ieee without its division above
// 2^125). For operands known to be small: a component of a unit-length direction (<= 2 with any rounding), a length
// inside the quotient's guard.
RTX_HD float rcp_small(float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_rcpf(b);
    return __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
#else
    return 1.0f / b;
#endif
}
// the root's seed: within 1 ulp of the correctly rounded root
RTX_HD float sqrt_seed(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return __builtin_sqrtf(x);
#endif
}

// a / b given y = RN(1 / b), for a and b inside the guard (b > 0)
RTX_HD float div_core(float a, float b, float y) {
    const float q0 = a * y;
    const float r = -__builtin_fmaf(b, q0, -a);
    return __builtin_fmaf(r, y, q0);
}
// sqrtf(x) given a seed within 1 ulp of it, for x inside the guard
RTX_HD float sqrt_core(float x, float seed) {
    const float sd = float_of(bits_of(seed) - 1u), su = float_of(bits_of(seed) + 1u);
    const float rd = __builtin_fmaf(-sd, seed, x), ru = __builtin_fmaf(-su, seed, x);
    float s = rd <= 0.0f ? sd : seed;
    s = ru > 0.0f ? su : s;
    return s;
}

RTX_HD float absf(float x) { return __builtin_fabsf(x); }
RTX_HD bool num_ok(float a) { return a == 0.0f || (absf(a) >= NUM_LO && absf(a) <= NUM_HI); }
RTX_HD bool div3_ok(f3 a, float b) { return b >= DEN_LO && b <= DEN_HI && num_ok(a.x) && num_ok(a.y) && num_ok(a.z); }

// The operations themselves. Inlined at every site: as functions of their own (noinline) they gave the frame kernels
// a stack (16 B of scratch, 1-3 scratch instructions) where they have none, so each site carries its fallback in a
// cold block instead (bench instantiation: 6,368 -> 6,593 static instructions).
RTX_HD f3 div3_ieee(f3 a, float b) { return f3{a.x / b, a.y / b, a.z / b}; }
RTX_HD f3 normalize_ieee(f3 a, float x, float& mg) {
    const float s = __builtin_sqrtf(x);
    mg = s;
    return f3{a.x / s, a.y / s, a.z / s};
}

// (a.x / b, a.y / b, a.z / b)
RTX_HD f3 div3(f3 a, float b) {
    if (div3_ok(a, b)) {
        const float y = rcp_small(b);
        return f3{div_core(a.x, b, y), div_core(a.y, b, y), div_core(a.z, b, y)};
    }
    return div3_ieee(a, b);
}

// sqrtf(x); the seed is a parameter so that a test can hand in the root moved by an ulp either way
RTX_HD float sqrt_exact(float x, float seed) {
    if (x >= ROOT_LO && x <= ROOT_HI) return sqrt_core(x, seed);
    return __builtin_sqrtf(x);
}
RTX_HD float sqrt_exact(float x) { return sqrt_exact(x, sqrt_seed(x)); }

// vec.c's normalize: mg = sqrtf(a.x a.x + a.y a.y + a.z a.z) (the squares added in that order), a / mg
RTX_HD f3 normalize_mag(f3 a, float& mg) {
    const float x = a.x * a.x + a.y * a.y + a.z * a.z;
    const float seed = sqrt_seed(x);
    const float lo = __builtin_fminf(__builtin_fminf(absf(a.x), absf(a.y)), absf(a.z));
    if (lo >= NRM_LO && seed <= NRM_HI) {
        const float s = sqrt_core(x, seed);
        const float y = rcp_small(s);
        mg = s;
        return f3{div_core(a.x, s, y), div_core(a.y, s, y), div_core(a.z, s, y)};
    }
    return normalize_ieee(a, x, mg);
}
RTX_HD f3 normalize3(f3 a) {
    float mg;
    return normalize_mag(a, mg);
}

}  // namespace rtx
