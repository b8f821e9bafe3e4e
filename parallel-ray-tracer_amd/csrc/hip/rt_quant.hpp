// rt_quant.hpp — the wide BVH's per-axis outward quantisation and a wide node's re-quantisation, shared by the host
// refit (rt_wide.cpp rth_wbvh_refit) and the device refit (rt_refit.hpp): plain C++17 under g++, __host__ __device__
// under hipcc, and the same bits from both.
//
// The rule is the collapse's (rt_wide.cpp quantise_axis): the grid's origin lies QBIAS steps below the lowest plane,
// every plane is checked with the walks' own decode fmaf(2^e, QBIAS + q, p) and moved outward until the decoded box
// contains the grown box; the exponent rises until all planes fit 8 bits. Only the starting exponent is formed
// differently: the collapse takes ceil(log2(extent / 255)) from libm, here it is the same number from the extent's
// exponent and mantissa bits (no libm call whose rounding host and device could disagree on). Nothing else here calls
// libm either: powers of two and the next float below are made from bits, floor / ceil / fma are exact operations.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RTQ_HD __host__ __device__ inline
#else
#define RTQ_HD inline
#endif

namespace rtq {

constexpr int QBIAS = 1024;  // rt_wide.cpp QBIAS
constexpr int WIDTH = 8;
constexpr int E_MAX = 117;   // the largest grid exponent: QBIAS * 2^E_MAX = 2^127 is still a float
constexpr int E_NONE = 127;  // quantise_axis: no grid holds the boxes

RTQ_HD float u2f(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
RTQ_HD uint32_t f2u(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
// 2^e, e in -126 .. 127
RTQ_HD float pow2(int e) { return u2f((uint32_t)(e + 127) << 23); }
RTQ_HD float decode(float scale, int q, float p) { return __builtin_fmaf(scale, (float)(QBIAS + q), p); }
// the next float below a finite f
RTQ_HD float next_below(float f) {
    const uint32_t u = f2u(f);
    return f > 0.0f ? u2f(u - 1) : (f == 0.0f ? u2f(0x80000001u) : u2f(u + 1));
}
// the largest float <= x
RTQ_HD float round_down(double x) {
    const float f = (float)x;
    return (double)f > x ? next_below(f) : f;
}
// the smallest e with 255 * 2^e >= ext, for a positive finite normal double ext
RTQ_HD int start_exponent(double ext) {
    uint64_t b;
    __builtin_memcpy(&b, &ext, 8);
    const int x = (int)((b >> 52) & 0x7FF) - 1023;  // ext = 1.f * 2^x
    const uint64_t frac = b & ((1ull << 52) - 1);
    return frac <= (127ull << 45) ? x - 7 : x - 6;  // 1.f <= 255 / 128
}

// a plane's step count as an int; a quotient far outside the 8 bits (an exponent still too small for the extent) is
// pinned instead of overflowing the conversion -- such an exponent is rejected either way
RTQ_HD int steps(double q) { return (int)(q < -1e9 ? -1e9 : (q > 1e9 ? 1e9 : q)); }

// Quantise one axis of k <= 8 child boxes (already grown) on the grid pb + 2^e * (QBIAS + q), q in 0..255. Returns the
// grid's exponent e (-126 .. E_MAX); pb receives the grid's origin, qlo / qhi the planes. E_NONE: no exponent up to
// E_MAX gives a grid with a finite origin whose decoded planes contain the boxes; pb and the planes are then not
// valid. With max|coordinate| <= RT_COORD_MAX = 2^123 (include/rt_hip.h) that cannot happen: the grown boxes span at
// most 2^124 (1 + 2^-16), about half of the 255 * 2^117 that E_MAX spans, and the origin lies within 2^123 + 2^127 of 0.
RTQ_HD int quantise_axis(const float* lo, const float* hi, int k, float& pb, int* qlo, int* qhi) {
    float p = lo[0], top = hi[0];
    for (int c = 1; c < k; c++) {
        p = lo[c] < p ? lo[c] : p;
        top = hi[c] > top ? hi[c] : top;
    }
    const double ext = (double)top - (double)p;
    int e = ext > 0 ? start_exponent(ext) : -126;
    e = e < -126 ? -126 : (e > 100 ? 100 : e);
    for (; e <= E_MAX; e++) {  // (QBIAS * 2^e stays finite)
        const float scale = pow2(e);
        pb = round_down((double)p - (double)QBIAS * scale);  // q = 0 decodes to the lowest plane or below it
        // (a lowest plane more than 2^52 times smaller than QBIAS * 2^e vanishes from that double difference: step down
        // until q = 0 decodes below it -- never taken while the difference is exact, i.e. on any sane box)
        for (int i = 0; i < 4 && decode(scale, 0, pb) > p; i++) pb = next_below(pb);
        bool ok = true;
        for (int c = 0; c < k && ok; c++) {
            int a = steps(__builtin_floor(((double)lo[c] - (double)pb) / scale)) - QBIAS;
            a = a < 0 ? 0 : (a > 255 ? 255 : a);
            while (a > 0 && decode(scale, a, pb) > lo[c]) a--;
            int b = steps(__builtin_ceil(((double)hi[c] - (double)pb) / scale)) - QBIAS;
            b = b < 0 ? 0 : b;
            while (b <= 255 && decode(scale, b, pb) < hi[c]) b++;
            if (b > 255 || decode(scale, a, pb) > lo[c]) ok = false;
            qlo[c] = a;
            qhi[c] = b;
        }
        if (ok) return e;
    }
    return E_NONE;
}

// ---- a wide node's 20 words (rt_device.hpp DWide), topology fields
RTQ_HD uint32_t imask_of(const uint32_t* W) { return W[3] >> 24; }
RTQ_HD uint32_t meta_of(const uint32_t* W, int s) { return (W[6 + (s >> 2)] >> (8 * (s & 3))) & 0xFFu; }
RTQ_HD bool occupied(const uint32_t* W, int s) { return ((imask_of(W) >> s) & 1u) || meta_of(W, s) != 0; }
// slot s's interior child: child_base + the interior slots below s
RTQ_HD uint32_t child_of(const uint32_t* W, int s) {
    return W[4] + (uint32_t)__builtin_popcount(imask_of(W) & ((1u << s) - 1u));
}

// A box as six floats: lo.xyz, hi.xyz. Folds start from the empty box.
struct Box {
    float lo[3], hi[3];
};
RTQ_HD Box empty_box() {
    const float inf = u2f(0x7F800000u);
    return Box{{inf, inf, inf}, {-inf, -inf, -inf}};
}
RTQ_HD void grow(Box& b, const float* v) {  // one vertex
    for (int a = 0; a < 3; a++) {
        b.lo[a] = v[a] < b.lo[a] ? v[a] : b.lo[a];
        b.hi[a] = v[a] > b.hi[a] ? v[a] : b.hi[a];
    }
}
RTQ_HD void grow(Box& b, const Box& o) {
    for (int a = 0; a < 3; a++) {
        b.lo[a] = o.lo[a] < b.lo[a] ? o.lo[a] : b.lo[a];
        b.hi[a] = o.hi[a] > b.hi[a] ? o.hi[a] : b.hi[a];
    }
}

// the summed surface area of a node's decoded child boxes (rt_update_info.area_ratio)
RTQ_HD double decoded_area(const uint32_t* W) {
    double sum = 0.0;
    float p[3], sc[3];
    for (int a = 0; a < 3; a++) {
        p[a] = u2f(W[a]);
        sc[a] = pow2((int)(int8_t)(uint8_t)(W[3] >> (8 * a)));
    }
    for (int s = 0; s < WIDTH; s++) {
        if (!occupied(W, s)) continue;
        double d[3];
        for (int a = 0; a < 3; a++) {
            const uint32_t w = W[8 + 4 * a + (s >> 1)] >> (16 * (s & 1));
            d[a] = (double)decode(sc[a], (int)((w >> 8) & 0xFFu), p[a]) - (double)decode(sc[a], (int)(w & 0xFFu), p[a]);
        }
        sum += 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    }
    return sum;
}

// Re-quantise a node in place from its occupied slots' exact child boxes (box[s], read for occupied slots only), each
// grown by `inflate`: rewrites the origin p, the three exponents and the plane words; imask, child_base, tri_base, meta
// and the slot assignment stay. The collapse's own arithmetic (rt_wide.cpp form): slots in rising order, lo - inflate
// and hi + inflate in float, empty slots an inverted box (255, 0). false: an axis has no grid (quantise_axis' E_NONE);
// the node is left as it was.
RTQ_HD bool requantise(uint32_t* W, const Box* box, float inflate) {
    float lo[3][WIDTH], hi[3][WIDTH];
    int qlo[3][WIDTH], qhi[3][WIDTH];
    int slot_list[WIDTH];
    int ks = 0;
    for (int s = 0; s < WIDTH; s++)
        if (occupied(W, s)) {
            for (int a = 0; a < 3; a++) {
                lo[a][ks] = box[s].lo[a] - inflate;
                hi[a][ks] = box[s].hi[a] + inflate;
            }
            slot_list[ks++] = s;
        }
    if (ks == 0) return true;
    float p[3];
    int eb[3];
    for (int a = 0; a < 3; a++) eb[a] = quantise_axis(lo[a], hi[a], ks, p[a], qlo[a], qhi[a]);
    if (eb[0] == E_NONE || eb[1] == E_NONE || eb[2] == E_NONE) return false;
    W[0] = f2u(p[0]);
    W[1] = f2u(p[1]);
    W[2] = f2u(p[2]);
    W[3] = (uint32_t)(uint8_t)(int8_t)eb[0] | ((uint32_t)(uint8_t)(int8_t)eb[1] << 8) |
           ((uint32_t)(uint8_t)(int8_t)eb[2] << 16) | (imask_of(W) << 24);
    uint32_t planes[3][WIDTH / 2];
    for (int a = 0; a < 3; a++)
        for (int j = 0; j < WIDTH / 2; j++) planes[a][j] = 0x00FF00FFu;  // qlo 255, qhi 0 in both halves
    for (int j = 0; j < ks; j++) {
        const int s = slot_list[j];
        for (int a = 0; a < 3; a++) {
            const uint32_t pair = (uint32_t)qlo[a][j] | ((uint32_t)qhi[a][j] << 8);
            uint32_t& w = planes[a][s >> 1];
            w = (s & 1) ? ((w & 0x0000FFFFu) | (pair << 16)) : ((w & 0xFFFF0000u) | pair);
        }
    }
    for (int a = 0; a < 3; a++)
        for (int j = 0; j < WIDTH / 2; j++) W[8 + 4 * a + j] = planes[a][j];
    return true;
}

}  // namespace rtq
