// pool_handout_test.cpp — the shadow pool's job-list indexing (rt_pool_list.hpp, the code the kernel runs) against a
// direct transcription of the cursor hand-out it replaces (rt_shpool.hpp shadow_pool<.., LIST = false>): the same
// (lane -> job) map round by round, every job handed out exactly once. g++ only, no GPU.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "rt_pool_list.hpp"

namespace {

using u64 = unsigned long long;
int fails = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (fails++ < 20) {                \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);      \
                std::printf("\n");             \
            }                                  \
        }                                      \
    } while (0)

// ---- the cursor hand-out, as the kernel has it (kth_bit, drop_low, advance, the while (req && cm) loop)
int kth_bit(u64 m, unsigned k) {
    int pos = 0;
    unsigned c = (unsigned)__builtin_popcount((unsigned)m);
    if (k >= c) {
        k -= c;
        m >>= 32;
        pos = 32;
    }
    unsigned w = (unsigned)m;
    for (int b = 16; b >= 2; b >>= 1) {
        c = (unsigned)__builtin_popcount(w & ((1u << b) - 1u));
        if (k >= c) {
            k -= c;
            w >>= b;
            pos += b;
        }
    }
    return pos + (k >= (w & 1u) ? 1 : 0);
}
u64 drop_low(u64 m, unsigned n) {
    if (n == 0) return m;
    const int p = kth_bit(m, n - 1u);
    return p >= 63 ? 0ull : m & ~((2ull << p) - 1ull);
}

struct Cursor {
    const std::vector<u64>& grp;  // [level][light] owner masks
    int LV, nl;
    int cl = 0, cj = -1;
    u64 cm = 0;
    unsigned shad = 0;
    Cursor(const std::vector<u64>& g, int lv, int n) : grp(g), LV(lv), nl(n) {}
    void advance() {
        while (cm == 0 && (cl + 1 < LV || cj + 1 < nl)) {
            if (cj + 1 < nl) {
                cj = cj + 1;
            } else {
                cj = 0;
                cl = cl + 1;
            }
            cm = grp[(size_t)cl * nl + cj];
            shad += (unsigned)__builtin_popcountll(cm);
        }
    }
    bool more() const { return cm != 0 || cj + 1 < nl || cl + 1 < LV; }
    // one refill: job[lane] = the job the idle lane takes, -1: none. Returns false when the pool is done (all idle,
    // nothing left)
    bool refill(u64 idle, u64 all, int* job) {
        for (int i = 0; i < 64; i++) job[i] = -1;
        advance();
        if (idle == all && cm == 0) return false;
        if (cm != 0) {
            u64 req = idle;
            while (req != 0ull && cm != 0ull) {
                const unsigned nreq = (unsigned)__builtin_popcountll(req), nav = (unsigned)__builtin_popcountll(cm);
                for (unsigned lane = 0; lane < 64; lane++) {
                    const unsigned k = rtp::rank_below(req, lane);
                    if (((req >> lane) & 1ull) && k < nav) job[lane] = kth_bit(cm, k) | (cl << 6) | (cj << 9);
                }
                if (nreq >= nav) {
                    req = drop_low(req, nav);
                    cm = 0ull;
                    advance();
                } else {
                    cm = drop_low(cm, nreq);
                    req = 0ull;
                }
            }
        }
        return true;
    }
};

// ---- the list hand-out, through rt_pool_list.hpp as the kernel calls it
struct List {
    std::vector<rtp::job_t> jl;
    unsigned head = 0, total = 0;
    List(const std::vector<u64>& grp, int LV, int nl) : jl((size_t)64 * LV * nl, 0xFFFFu) {
        for (int l = 0; l < LV; l++)
            for (int j = 0; j < nl; j++) {
                const u64 M = grp[(size_t)l * nl + j];
                for (unsigned lane = 0; lane < 64; lane++)
                    if ((M >> lane) & 1ull) {
                        const unsigned slot = rtp::owner_slot(total, rtp::rank_below(M, lane));
                        CHECK(slot < jl.size(), "slot %u past the list (%zu)", slot, jl.size());
                        CHECK(jl[slot] == 0xFFFFu, "slot %u written twice", slot);
                        jl[slot] = rtp::job_of(lane, (unsigned)l, (unsigned)j);
                    }
                total = rtp::next_base(total, M);
            }
    }
    bool more() const { return head < total; }
    bool refill(u64 idle, u64 all, int* job) {
        for (int i = 0; i < 64; i++) job[i] = -1;
        if (idle == all && head == total) return false;
        if (head < total) {
            for (unsigned lane = 0; lane < 64; lane++) {
                unsigned slot;
                if (((idle >> lane) & 1ull) && rtp::take(head, total, rtp::rank_below(idle, lane), slot))
                    job[lane] = (int)jl[slot];
            }
            head = rtp::head_after(head, total, (unsigned)__builtin_popcountll(idle));
        }
        return true;
    }
};

// One pool run: the two hand-outs side by side. After each refill a pseudo-random subset of the busy lanes ends its
// walk (`finish` of 256: the chance per lane and step), until `regroup` lanes are idle or all are -- the kernel's walk
// loop as far as the hand-out sees it. n_active: lanes of the wave (lanes past it never exist: a partial wave).
void run_case(const char* what, const std::vector<u64>& grp, int LV, int nl, int regroup, unsigned finish,
              std::mt19937& rng, int n_active = 64) {
    const u64 all = n_active == 64 ? ~0ull : ((1ull << n_active) - 1ull);
    Cursor cur(grp, LV, nl);
    List lst(grp, LV, nl);
    std::vector<int> given((size_t)64 * LV * nl, 0);
    unsigned want_total = 0;
    for (u64 m : grp) want_total += (unsigned)__builtin_popcountll(m);
    CHECK(lst.total == want_total, "%s: list total %u, masks hold %u", what, lst.total, want_total);
    u64 busy = 0;
    int rounds = 0;
    for (;; rounds++) {
        CHECK(rounds < 100000, "%s: no end", what);
        if (rounds >= 100000) return;
        const u64 idle = all & ~busy;
        int ja[64], jb[64];
        const bool ga = cur.refill(idle, all, ja), gb = lst.refill(idle, all, jb);
        CHECK(ga == gb, "%s: round %d: cursor %s, list %s", what, rounds, ga ? "goes on" : "ends", gb ? "goes on" : "ends");
        if (!ga || !gb) break;
        for (int lane = 0; lane < 64; lane++) {
            CHECK(ja[lane] == jb[lane], "%s: round %d lane %d: cursor job %d, list job %d", what, rounds, lane, ja[lane],
                  jb[lane]);
            if (jb[lane] < 0) continue;
            CHECK((idle >> lane) & 1ull, "%s: round %d: busy lane %d given a job", what, rounds, lane);
            const unsigned j = (unsigned)jb[lane];
            const unsigned ow = rtp::job_lane(j), l = rtp::job_level(j), li = rtp::job_light(j);
            CHECK((int)l < LV && (int)li < nl && ((grp[(size_t)l * nl + li] >> ow) & 1ull), "%s: job %u is no owner", what, j);
            CHECK(rtp::job_slot_of_owner(j) == 64 * l + ow, "%s: job %u slot", what, j);
            if ((int)l < LV && (int)li < nl) given[((size_t)l * nl + li) * 64 + ow]++;
            busy |= 1ull << lane;
        }
        CHECK(cur.more() || !lst.more(), "%s: round %d: the list has work the cursor has not", what, rounds);
        // (the cursor's `more` may still be true over trailing empty groups: it then breaks the walk loop early once,
        // finds nothing, and walks on -- no step more or less)
        for (;;) {  // the walk loop
            for (int lane = 0; lane < 64; lane++)
                if (((busy >> lane) & 1ull) && (rng() & 255u) < finish) busy &= ~(1ull << lane);
            const u64 id2 = all & ~busy;
            if (id2 == all || (lst.more() && __builtin_popcountll(id2) >= regroup)) break;
        }
    }
    CHECK(cur.shad == want_total, "%s: cursor counted %u rays of %u", what, cur.shad, want_total);
    CHECK(lst.head == lst.total, "%s: list ends at %u of %u", what, lst.head, lst.total);
    for (int l = 0; l < LV; l++)
        for (int j = 0; j < nl; j++)
            for (int ow = 0; ow < 64; ow++) {
                const int want = (int)((grp[(size_t)l * nl + j] >> ow) & 1ull);
                CHECK(given[((size_t)l * nl + j) * 64 + ow] == want, "%s: job (%d, %d, %d) handed out %d times, want %d",
                      what, ow, l, j, given[((size_t)l * nl + j) * 64 + ow], want);
            }
}

}  // namespace

int main() {
    std::mt19937 rng(20240607u);
    const int regroups[] = {1, 16, 63, 64};
    auto every = [&](const char* what, const std::vector<u64>& grp, int LV, int nl, int n_active = 64) {
        for (int rg : regroups)
            for (unsigned fin : {32u, 128u, 256u}) run_case(what, grp, LV, nl, rg, fin, rng, n_active);
    };
    // all group masks empty
    every("empty", std::vector<u64>(8, 0ull), 4, 2);
    every("empty 1x1", std::vector<u64>(1, 0ull), 1, 1);
    {  // one job: in the first group, in the last group, lane 0, lane 63
        for (int g : {0, 7})
            for (int lane : {0, 17, 63}) {
                std::vector<u64> grp(8, 0ull);
                grp[g] = 1ull << lane;
                every("one job", grp, 4, 2);
            }
    }
    {  // a group of 64 followed by empty groups and a group of 1
        std::vector<u64> grp(8, 0ull);
        grp[0] = ~0ull;
        grp[6] = 1ull << 40;
        every("64 then 1", grp, 4, 2);
        grp[7] = 0ull;
        every("64 then 1, trailing empty", grp, 4, 2);
    }
    {  // more requesters than jobs left: 3 jobs in two groups for 64 idle lanes; then 64 + 5
        std::vector<u64> grp(2, 0ull);
        grp[0] = (1ull << 3) | (1ull << 62);
        grp[1] = 1ull << 0;
        every("3 jobs", grp, 1, 2);
        grp[0] = ~0ull;
        grp[1] = 0x1Full << 20;
        every("69 jobs", grp, 1, 2);
    }
    {  // exactly as many requesters as jobs: 64 jobs over four groups for 64 idle lanes; 64 in one
        std::vector<u64> grp(4, 0ull);
        grp[0] = 0x00000000FFFF0000ull;
        grp[1] = 0xFFFF000000000000ull;
        grp[2] = 0x000000000000FFFFull;
        grp[3] = 0x0000FFFF00000000ull;
        every("64 = 64", grp, 2, 2);
        every("64 = 64 one group", std::vector<u64>(1, ~0ull), 1, 1);
        // a partial wave: 20 lanes, 20 jobs
        every("20 = 20", std::vector<u64>(1, (1ull << 20) - 1ull), 1, 1, 20);
    }
    // 1, 2 and 8 lights x 1, 4 and 8 levels, full and sparse; a few thousand seeded random mask sets
    int sets = 0;
    for (int nl : {1, 2, 8})
        for (int LV : {1, 4, 8}) {
            every("full", std::vector<u64>((size_t)LV * nl, ~0ull), LV, nl);
            for (int rep = 0; rep < 400; rep++, sets++) {
                std::vector<u64> grp((size_t)LV * nl);
                const unsigned dens = rng() % 5u;  // dense .. very sparse, empty groups included
                for (u64& m : grp) {
                    m = ((u64)rng() << 32) | rng();
                    for (unsigned i = 0; i < dens; i++) m &= ((u64)rng() << 32) | rng();
                    if (rng() % 4u == 0u) m = 0ull;
                }
                const int n_active = rep % 7 == 0 ? 1 + (int)(rng() % 64u) : 64;
                if (n_active < 64)
                    for (u64& m : grp) m &= (1ull << n_active) - 1ull;
                run_case("random", grp, LV, nl, regroups[rng() % 4u], 16u + rng() % 240u, rng, n_active);
            }
        }
    // the job encoding and the list's size
    CHECK(rtp::job_of(63, 7, 31) == (63u | (7u << 6) | (31u << 9)), "job_of");
    CHECK(rtp::list_words(4, 2) * 4 == 64 * 4 * 2 * 2, "list_words(4, 2) = %d words", rtp::list_words(4, 2));
    CHECK(rtp::head_after(5, 9, 64) == 9 && rtp::head_after(5, 9, 3) == 8 && rtp::head_after(9, 9, 64) == 9, "head_after");
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("all checks passed (%d random mask sets)\n", sets);
    return 0;
}
