// The shared quantiser (rt_quant.hpp) on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_refit_host.py builds and runs this): random and adversarial sets of up to 8 child boxes per axis --
// equal planes, extents of exactly 255 * 2^k, denormal extents, magnitudes near 1e10 -- must come back with planes in
// 0..255 whose fmaf decode contains every box, and a re-quantised node must keep its topology words.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "rt_quant.hpp"

namespace {

int failures = 0;
long long cases = 0;

void check_axis(const float* lo, const float* hi, int k, const char* what) {
    float pb = 0.0f;
    int qlo[8], qhi[8];
    for (int c = 0; c < 8; c++) qlo[c] = qhi[c] = -1;
    const int e = rtq::quantise_axis(lo, hi, k, pb, qlo, qhi);
    cases++;
    bool ok = e >= -126 && e <= 110 && std::isfinite(pb);
    const float scale = std::ldexp(1.0f, e);
    ok = ok && scale == rtq::pow2(e);
    for (int c = 0; c < k && ok; c++) {
        ok = qlo[c] >= 0 && qlo[c] <= 255 && qhi[c] >= 0 && qhi[c] <= 255;
        // the walks' decode: one fma, fmaf(2^e, 1024 + q, p)
        ok = ok && std::fmaf(scale, (float)(1024 + qlo[c]), pb) <= lo[c];
        ok = ok && std::fmaf(scale, (float)(1024 + qhi[c]), pb) >= hi[c];
    }
    if (!ok) {
        if (failures++ < 10) {
            std::printf("FAIL %s: k=%d e=%d pb=%a\n", what, k, e, pb);
            for (int c = 0; c < k; c++) std::printf("   lo=%a hi=%a qlo=%d qhi=%d\n", lo[c], hi[c], qlo[c], qhi[c]);
        }
    }
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    float lo[8], hi[8];
    // random sets over many magnitudes and extents
    for (int it = 0; it < 200000; it++) {
        const int k = 1 + (int)(rng() % 8);
        const double centre = (U(rng) - 0.5) * std::ldexp(1.0, (int)(rng() % 40) - 6);
        const double ext = std::ldexp(U(rng) + 1e-3, (int)(rng() % 50) - 30);
        for (int c = 0; c < k; c++) {
            const double a = centre + (U(rng) - 0.5) * ext, b = centre + (U(rng) - 0.5) * ext;
            lo[c] = (float)std::fmin(a, b);
            hi[c] = (float)std::fmax(a, b);
        }
        check_axis(lo, hi, k, "random");
    }
    // equal planes: zero-extent axes, alone and beside others, at several magnitudes and both signs of zero
    for (float v : {0.0f, -0.0f, 1.0f, -1.0f, 3.14159f, 1e-30f, -1e-38f, 1e10f, -1e10f, 16.000002f, 1.17549435e-38f}) {
        for (int k = 1; k <= 8; k++) {
            for (int c = 0; c < k; c++) lo[c] = hi[c] = v;
            check_axis(lo, hi, k, "equal planes");
            lo[0] = std::nextafter(v, -INFINITY);
            check_axis(lo, hi, k, "equal planes, one a float below");
            hi[k - 1] = std::nextafter(v, INFINITY);
            check_axis(lo, hi, k, "equal planes, one a float above");
        }
    }
    // extents of exactly 255 * 2^k (the starting exponent's boundary), one float less and one more, at several origins
    for (int k2 = -140; k2 <= 90; k2++)
        for (double origin : {0.0, 1.0, -1.0, 1024.0, -0.333, 1e10, -1e10, 7e-39}) {
            const double ext = 255.0 * std::ldexp(1.0, k2);
            const float p = (float)origin;
            const float tops[3] = {(float)((double)p + ext), std::nextafter((float)((double)p + ext), -INFINITY),
                                   std::nextafter((float)((double)p + ext), INFINITY)};
            for (float top : tops) {
                if (!(top >= p) || !std::isfinite(top)) continue;
                lo[0] = p;
                hi[0] = top;
                check_axis(lo, hi, 1, "255 * 2^k");
                lo[1] = hi[1] = (float)((double)p + 0.5 * ext);  // an inner plane pair
                lo[2] = p;
                hi[2] = (float)((double)p + ext / 255.0);
                check_axis(lo, hi, 3, "255 * 2^k with inner planes");
            }
        }
    // denormal extents and denormal planes
    for (int it = 0; it < 20000; it++) {
        const int k = 1 + (int)(rng() % 8);
        const float base = (rng() & 1) ? 0.0f : std::ldexp(1.0f, -(int)(rng() % 30) - 100);
        for (int c = 0; c < k; c++) {
            const float a = base + std::ldexp((float)(rng() % 4096), -149), b = base + std::ldexp((float)(rng() % 4096), -149);
            lo[c] = std::fmin(a, b) * ((it & 1) ? 1.0f : -1.0f);
            hi[c] = std::fmax(a, b) * ((it & 1) ? 1.0f : -1.0f);
            if (lo[c] > hi[c]) std::swap(lo[c], hi[c]);
        }
        check_axis(lo, hi, k, "denormal");
    }
    // magnitudes near 1e10 (the reference's empty-box seeds), tiny and huge extents beside them
    for (int it = 0; it < 20000; it++) {
        const int k = 1 + (int)(rng() % 8);
        for (int c = 0; c < k; c++) {
            const int kind = (int)(rng() % 4);
            double a, b;
            if (kind == 0) a = b = 1e10;
            else if (kind == 1) a = -1e10, b = 1e10;
            else if (kind == 2) a = 1e10 - U(rng) * 5000.0, b = a + U(rng) * 3000.0;
            else a = -1e10 * U(rng), b = a + U(rng);
            lo[c] = (float)std::fmin(a, b);
            hi[c] = (float)std::fmax(a, b);
        }
        check_axis(lo, hi, k, "near 1e10");
    }
    // a node: random occupancy, re-quantised in place; topology words stay, decoded slots contain their grown boxes
    for (int it = 0; it < 50000; it++) {
        uint32_t W[20], W0[20];
        for (uint32_t& w : W) w = (uint32_t)rng();
        const uint32_t imask = (uint32_t)(rng() & 0xFF);
        uint8_t meta[8];
        rtq::Box box[8];
        for (int s = 0; s < 8; s++) {
            const bool leaf = !((imask >> s) & 1u) && (rng() & 1);
            meta[s] = leaf ? (uint8_t)(((1 + rng() % 4) << 5) | (rng() % 28)) : 0;
            for (int a = 0; a < 3; a++) {
                const double c = (U(rng) - 0.5) * 40.0, e = (rng() % 5 == 0) ? 0.0 : U(rng) * std::ldexp(1.0, (int)(rng() % 12) - 8);
                box[s].lo[a] = (float)c;
                box[s].hi[a] = (float)(c + e) < box[s].lo[a] ? box[s].lo[a] : (float)(c + e);
            }
        }
        W[3] = (W[3] & 0x00FFFFFFu) | (imask << 24);
        std::memcpy(&W[6], meta, 8);
        std::memcpy(W0, W, sizeof W);
        const float inflate = (it & 1) ? 0.0f : std::ldexp(16.0f, -16);
        rtq::requantise(W, box, inflate);
        cases++;
        bool ok = (W[3] >> 24) == imask && W[4] == W0[4] && W[5] == W0[5] && W[6] == W0[6] && W[7] == W0[7];
        bool any = false;
        for (int s = 0; s < 8 && ok; s++) {
            const bool occ = rtq::occupied(W0, s);
            any = any || occ;
            for (int a = 0; a < 3 && ok; a++) {
                const uint32_t w = W[8 + 4 * a + (s >> 1)] >> (16 * (s & 1));
                const int ql = (int)(w & 0xFF), qh = (int)((w >> 8) & 0xFF);
                if (!occ) continue;  // (an empty slot's planes are checked below)
                const float scale = std::ldexp(1.0f, (int)(int8_t)(uint8_t)(W[3] >> (8 * a)));
                const float p = rtq::u2f(W[a]);
                ok = std::fmaf(scale, (float)(1024 + ql), p) <= box[s].lo[a] - inflate &&
                     std::fmaf(scale, (float)(1024 + qh), p) >= box[s].hi[a] + inflate;
            }
        }
        if (ok && any)  // empty slots: the inverted box (255, 0)
            for (int s = 0; s < 8 && ok; s++)
                if (!rtq::occupied(W0, s))
                    for (int a = 0; a < 3; a++) {
                        const uint32_t w = W[8 + 4 * a + (s >> 1)] >> (16 * (s & 1));
                        ok = ok && (w & 0xFFFF) == 0x00FFu;
                    }
        if (!any) ok = ok && std::memcmp(W, W0, sizeof W) == 0;  // nothing occupied: the node is left alone
        if (!ok && failures++ < 10) std::printf("FAIL node %d\n", it);
    }
    if (failures) {
        std::printf("refit_quant: %d failures in %lld cases\n", failures, cases);
        return 1;
    }
    std::printf("refit_quant: ok (%lld cases)\n", cases);
    return 0;
}
