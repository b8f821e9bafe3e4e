// The host forms of rt_exact.hpp against `/` and sqrtf, bit for bit (g++ -ffp-contract=off; tests/test_exact_forms.py).
// On the host the reciprocal is 1.0f / b and the root's seed is handed in, so what is checked here is the algebra of
// the short forms and the guards: the quotient's one correction, the root's choice among three neighbours, zeros' signs,
// and that everything outside the ranges takes the operation itself. The device forms (v_rcp_f32, v_sqrt_f32) are
// checked on the GPU by tools/exact/exact_exhaustive.
//   exact_forms_test [millions of random operands per operation, default 100]
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "rt_exact.hpp"

using rtx::bits_of;
using rtx::f3;
using rtx::float_of;

static std::atomic<unsigned long long> bad_div{0}, bad_root{0}, bad_norm{0}, bad_rcp{0}, n_short{0}, n_fall{0};
static std::atomic<int> printed{0};
static thread_local unsigned long long tl_short = 0, tl_fall = 0;  // (flushed per thread: no contended counter per check)
static void flush() {
    n_short += tl_short, n_fall += tl_fall;
    tl_short = tl_fall = 0;
}

struct Rng {
    uint64_t s;
    uint64_t next() {  // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};
// a mantissa biased towards all-zeros and all-ones: a quarter each within a few low bits of either, half uniform
static uint32_t mant(Rng& g) {
    const uint64_t r = g.next();
    const uint32_t m = (uint32_t)(r >> 20) & 0x7FFFFFu, low = (uint32_t)(r >> 44) & ((1u << ((r >> 50) % 12)) - 1u);
    switch (r & 3u) {
        case 0: return low;
        case 1: return 0x7FFFFFu - low;
        default: return m;
    }
}
// a float with an unbiased exponent uniform in [elo, ehi] (clamped to the normal range), either sign when `sign`
static float rnd(Rng& g, int elo, int ehi, bool sign) {
    const uint64_t r = g.next();
    int e = elo + (int)(r % (uint64_t)(ehi - elo + 1)) + 127;
    if (e < 1) e = 1;
    if (e > 254) e = 254;
    return float_of(((sign && (r >> 40 & 1)) ? 0x80000000u : 0u) | ((uint32_t)e << 23) | mant(g));
}

static void report(const char* what, float a, float b, float got, float want) {
    if (printed.fetch_add(1) < 20)
        std::printf("MISMATCH %s a=%a (0x%08x) b=%a (0x%08x) got 0x%08x want 0x%08x\n", what, (double)a, bits_of(a), (double)b,
                    bits_of(b), bits_of(got), bits_of(want));
}
static void check_div3(f3 a, float b) {
    const f3 q = rtx::div3(a, b);
    const float wx = a.x / b, wy = a.y / b, wz = a.z / b;
    if (bits_of(q.x) != bits_of(wx)) bad_div++, report("div3.x", a.x, b, q.x, wx);
    if (bits_of(q.y) != bits_of(wy)) bad_div++, report("div3.y", a.y, b, q.y, wy);
    if (bits_of(q.z) != bits_of(wz)) bad_div++, report("div3.z", a.z, b, q.z, wz);
    (rtx::div3_ok(a, b) ? tl_short : tl_fall)++;
}
// the three seeds: the correctly rounded root moved by -1, 0, +1 ulp
static void check_root(float x) {
    const float want = std::sqrt(x);
    for (int d = -1; d <= 1; d++) {
        const float seed = float_of(bits_of(want) + (uint32_t)d);
        const float got = rtx::sqrt_exact(x, seed);
        if (bits_of(got) != bits_of(want)) bad_root++, report(d < 0 ? "root-1" : d ? "root+1" : "root", x, seed, got, want);
    }
    const float got = rtx::sqrt_exact(x);
    if (bits_of(got) != bits_of(want)) bad_root++, report("root(x)", x, 0.0f, got, want);
}
static void check_norm(f3 a) {
    float mg;
    const f3 q = rtx::normalize_mag(a, mg);
    const float s = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    const float wx = a.x / s, wy = a.y / s, wz = a.z / s;
    if (bits_of(mg) != bits_of(s)) bad_norm++, report("norm.mg", a.x, a.y, mg, s);
    if (bits_of(q.x) != bits_of(wx)) bad_norm++, report("norm.x", a.x, s, q.x, wx);
    if (bits_of(q.y) != bits_of(wy)) bad_norm++, report("norm.y", a.y, s, q.y, wy);
    if (bits_of(q.z) != bits_of(wz)) bad_norm++, report("norm.z", a.z, s, q.z, wz);
    const f3 p = rtx::normalize3(a);
    if (bits_of(p.x) != bits_of(wx) || bits_of(p.y) != bits_of(wy) || bits_of(p.z) != bits_of(wz)) bad_norm++;
}
static void check_rcp(float b) {
    const float got = rtx::rcp_small(b), want = 1.0f / b;
    if (bits_of(got) != bits_of(want)) bad_rcp++, report("rcp_small", 1.0f, b, got, want);
}

static void random_part(uint64_t seed, uint64_t n) {
    Rng g{seed};
    for (uint64_t i = 0; i < n; i++) {
        // the quotient: denominators across both edges of [2^-40, 2^40] (a few negative), numerators across both edges of
        // [2^-50, 2^50], one in 16 a zero of either sign; every third triple shares the narrow range the issue's check used
        const bool narrow = i % 3 == 0;
        float b = narrow ? rnd(g, -31, 33, false) : rnd(g, -44, 44, false);
        if ((g.next() & 63u) == 0) b = -b;
        f3 a;
        float* c[3] = {&a.x, &a.y, &a.z};
        for (float* p : c) {
            *p = narrow ? rnd(g, -31, 33, true) : rnd(g, -54, 54, true);
            if ((g.next() & 15u) == 0) *p = float_of(bits_of(*p) & 0x80000000u);
        }
        check_div3(a, b);
        // the root across both edges of [2^-64, 2^66]
        check_root(rnd(g, -68, 70, false));
        // normalize: components of one scale (across both edges of [2^-32, 2^32]) or of mixed scales
        const int e0 = -36 + (int)(g.next() % 73);
        const bool mixed = (g.next() & 3u) == 0;
        f3 v;
        float* d[3] = {&v.x, &v.y, &v.z};
        for (float* p : d) *p = mixed ? rnd(g, -40, 40, true) : rnd(g, e0 - 3, e0, true);
        check_norm(v);
        check_rcp(rnd(g, -70, 1, true));
    }
    flush();
}

static void structured_part() {
    const uint32_t mants[] = {0u, 1u, 2u, 0x7FFFFFu, 0x7FFFFEu, 0x7FFFFDu, 0x400000u, 0x3FFFFFu, 0x400001u, 0x2AAAABu, 0x555555u};
    std::vector<float> nums, dens, roots;
    const int ne[] = {-52, -51, -50, -49, -1, 0, 1, 23, 49, 50, 51, -126, 127, -100, 100};
    const int de[] = {-42, -41, -40, -39, -1, 0, 1, 12, 39, 40, 41, -126, 127, -125, 125};
    const int re[] = {-66, -65, -64, -63, -1, 0, 1, 2, 65, 66, 67, -126, 127, -97, -96, -95};
    for (uint32_t m : mants) {
        for (int e : ne)
            for (uint32_t sg : {0u, 0x80000000u}) nums.push_back(float_of(sg | (uint32_t)(e + 127) << 23 | m));
        for (int e : de)
            for (uint32_t sg : {0u, 0x80000000u}) dens.push_back(float_of(sg | (uint32_t)(e + 127) << 23 | m));
        for (int e : re) roots.push_back(float_of((uint32_t)(e + 127) << 23 | m));
    }
    // zeros, denormals, infinities, NaNs
    const uint32_t special[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu, 0x00400000u, 0x7F800000u,
                                0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0x7FFFFFFFu, 0x7F7FFFFFu, 0xFF7FFFFFu};
    for (uint32_t u : special) {
        nums.push_back(float_of(u));
        dens.push_back(float_of(u));
        roots.push_back(float_of(u));
    }
    // the guards' ends themselves and their neighbours
    for (float e : {rtx::DEN_LO, rtx::DEN_HI, rtx::NUM_LO, rtx::NUM_HI, rtx::ROOT_LO, rtx::ROOT_HI, rtx::NRM_LO, rtx::NRM_HI})
        for (int d = -1; d <= 1; d++) {
            const float v = float_of(bits_of(e) + (uint32_t)d);
            nums.push_back(v), nums.push_back(-v), dens.push_back(v), dens.push_back(-v), roots.push_back(v);
        }
    for (float b : dens)
        for (size_t i = 0; i < nums.size(); i++)
            check_div3(f3{nums[i], nums[(i * 7 + 3) % nums.size()], nums[(i * 13 + 5) % nums.size()]}, b);
    for (float x : roots) check_root(x), check_root(-x);
    for (float x : nums) {
        check_rcp(x);
        for (size_t i = 0; i < nums.size(); i += 5) {
            check_norm(f3{x, nums[i], nums[(i * 11 + 1) % nums.size()]});
            check_norm(f3{nums[i], x, x});
            check_norm(f3{nums[i], nums[i], x});
        }
    }
    // -0 / b stays -0 inside the guard
    const f3 z = rtx::div3(f3{-0.0f, 0.0f, -0.0f}, 3.0f);
    if (!rtx::div3_ok(f3{-0.0f, 0.0f, -0.0f}, 3.0f) || bits_of(z.x) != 0x80000000u || bits_of(z.y) != 0u ||
        bits_of(z.z) != 0x80000000u)
        bad_div++, std::printf("MISMATCH signed zeros\n");
}

int main(int argc, char** argv) {
    const uint64_t millions = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100;
    structured_part();
    flush();
    const unsigned nt = 8;
    std::vector<std::thread> th;
    const uint64_t per = (millions * 1000000ull + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(random_part, 0x1234ull + 977ull * t, per);
    for (auto& t : th) t.join();
    std::printf("random operands per operation: %llu; quotient triples short %llu, fallback %llu\n",
                (unsigned long long)(per * nt), (unsigned long long)n_short.load(), (unsigned long long)n_fall.load());
    std::printf("mismatches: div3 %llu root %llu normalize %llu rcp_small %llu\n", (unsigned long long)bad_div.load(),
                (unsigned long long)bad_root.load(), (unsigned long long)bad_norm.load(), (unsigned long long)bad_rcp.load());
    const bool ok = !bad_div && !bad_root && !bad_norm && !bad_rcp && n_short.load() > per && n_fall.load() > per / 4;
    if (ok) std::printf("all checks passed\n");
    return ok ? 0 : 1;
}
