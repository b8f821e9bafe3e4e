// The greedy collapse (csrc/hip/rt_collapse.hpp through rth_wbvh_build_greedy) and the wide-tree validator
// (rth_wbvh_check) as a plain program, so that it can run under the host sanitizers: random scenes through both
// binary builders, comb and balanced hand-made trees of 1, 2, 8, 9 and 33 triangles, the validator on every result,
// a refit of the result with unmoved triangles, and the validator's answer to corrupted words.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_host.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

// greedy collapse of (bvh, idx) over T: valid, refit-stable; returns the node count
static int run(const rt_bvh_node* bvh, int nn, const int* idx, const rt_triangle* T, int n) {
    uint32_t* words = nullptr;
    int* order = nullptr;
    rth_wbvh_info wi{}, ci{};
    const float inflate = 16.0f / 65536.0f;
    CHECK(rth_wbvh_build_greedy(bvh, nn, idx, T, n, inflate, &words, &order, &wi) == RT_OK);
    if (!words) return 0;
    CHECK(rth_wbvh_check(words, wi.n_nodes, order, n, 64, &ci) == RT_OK);
    CHECK(ci.depth == wi.depth && ci.max_children == wi.max_children && wi.n_tris == n);
    std::vector<uint32_t> again(words, words + 20 * (size_t)wi.n_nodes);
    CHECK(rth_wbvh_refit(again.data(), wi.n_nodes, order, T, n, inflate) == RT_OK);
    CHECK(std::memcmp(again.data(), words, sizeof(uint32_t) * again.size()) == 0);
    if (n > 8) {  // corrupted words: the validator's codes
        std::vector<uint32_t> w(words, words + 20 * (size_t)wi.n_nodes);
        w[4] = (uint32_t)wi.n_nodes;  // the root's child base
        CHECK(rth_wbvh_check(w.data(), wi.n_nodes, order, n, 64, nullptr) == ((words[3] >> 24) ? RTH_WCHK_RANGE : RT_OK));
        std::vector<int> o(order, order + n);
        o[0] = o[1];
        CHECK(rth_wbvh_check(words, wi.n_nodes, o.data(), n, 64, nullptr) == RTH_WCHK_ORDER);
        CHECK(rth_wbvh_check(words, wi.n_nodes, order, n, wi.depth - 1, nullptr) == (wi.depth > 1 ? RTH_WCHK_DEPTH : RT_OK));
    }
    const int nodes = wi.n_nodes;
    rth_free(words);
    rth_free(order);
    return nodes;
}

// a comb (balanced = false) or a balanced tree over leaves first .. first + cnt - 1 in the reference layout
static void make(std::vector<rt_bvh_node>& out, int at, int first, int cnt, bool balanced) {
    if (cnt == 1) {
        out[at].tr_len = 1;
        out[at].child = first;
        return;
    }
    const int c = (int)out.size(), l = balanced ? cnt / 2 : cnt - 1;
    out[at].tr_len = 0;
    out[at].child = c;
    out.push_back(rt_bvh_node{});
    out.push_back(rt_bvh_node{});
    make(out, c, first, l, balanced);
    make(out, c + 1, first + l, cnt - l, balanced);
}

int main() {
    rth_rng g;
    for (int n : {1, 2, 3, 8, 9, 33, 500, 3000}) {
        rth_srand(&g, 7u + (unsigned)n);
        rt_triangle* T = nullptr;
        CHECK(rth_triangles_random((size_t)n, &g, &T) == RT_OK);
        for (int heur : {3, (int)RTH_BVH_BINNED_SAH}) {
            rt_bvh_node* bvh = nullptr;
            int nn = 0;
            int* idx = nullptr;
            CHECK(rth_bvh_build(T, (size_t)n, heur, &g, &bvh, &nn, &idx, nullptr) == RT_OK);
            run(bvh, nn, idx, T, n);
            rth_free(bvh);
            rth_free(idx);
        }
        if (n <= 33)
            for (bool balanced : {false, true}) {
                std::vector<rt_bvh_node> bvh(1);
                bvh.reserve(2 * (size_t)n);
                make(bvh, 0, 0, n, balanced);
                std::vector<int> idx(n);
                for (int i = 0; i < n; i++) idx[i] = n - 1 - i;
                const int nodes = run(bvh.data(), (int)bvh.size(), idx.data(), T, n);
                if (!balanced && n == 33) CHECK(nodes == 5);
                if (n <= 4) CHECK(nodes == 1);
            }
        rth_free(T);
    }
    if (fails) return 1;
    std::printf("collapse: ok\n");
    return 0;
}
