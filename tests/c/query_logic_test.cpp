// Host-only checks of what the query entry points decide alike (parallel-ray-tracer_amd/csrc/hip/rt_query_logic.hpp),
// compiled with plain g++ by tests/test_query_logic.py: no GPU, no HIP.
//   * every shared message of every family, verbatim: the header composes them from a family's words, and the strings
//     below are the ones the entry points carried one by one before they shared the header;
//   * each check next to its accepted neighbour, in the order the entry points made them;
//   * the list capacity rule and the grid rule at their edges.
#include <climits>
#include <cstdio>
#include <string>

#include "rt_query_logic.hpp"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                                   \
        }                                                                 \
    } while (0)

// ---------------------------------------------------------------- messages
struct Expect {
    rtq::Fam f;
    const char* no_scene;
    const char* null_args;
    const char* bad_kernel;
    const char* negative;
    // the list families' (null: the family has no lists)
    const char* cap_range;
    const char* count_all;
    const char* needs_count_all;
    const char* count_out;
};
static const Expect EXPECT[rtq::NFAM] = {
    {rtq::RAYS, "rt_trace_rays: no scene uploaded", "rt_trace_rays: null rays / results", "rt_trace_rays: bad kernel",
     "rt_trace_rays: negative ray count", nullptr, nullptr, nullptr, nullptr},
    {rtq::SHADE, "rt_shade_rays: no scene uploaded", "rt_shade_rays: null rays / results", "rt_shade_rays: bad kernel",
     "rt_shade_rays: negative ray count", nullptr, nullptr, nullptr, nullptr},
    {rtq::HITS, "rt_trace_hits: no scene uploaded", "rt_trace_hits: null rays / results", "rt_trace_hits: bad kernel",
     "rt_trace_hits: negative ray count", "rt_trace_hits: max_hits must be 0..16",
     "rt_trace_hits: count_all must be 0 or 1", "rt_trace_hits: max_hits = 0 needs count_all",
     "rt_trace_hits: a counting query needs a count output"},
    {rtq::NEAREST, "rt_nearest_points: no scene uploaded", "rt_nearest_points: null points / results",
     "rt_nearest_points: bad kernel", "rt_nearest_points: negative point count", nullptr, nullptr, nullptr, nullptr},
    {rtq::NEIGHBOURS, "rt_nearest_tris: no scene uploaded", "rt_nearest_tris: null points / results",
     "rt_nearest_tris: bad kernel", "rt_nearest_tris: negative point count", "rt_nearest_tris: max_tris must be 0..16",
     "rt_nearest_tris: count_all must be 0 or 1", "rt_nearest_tris: max_tris = 0 needs count_all",
     "rt_nearest_tris: a counting query needs a count output"},
    {rtq::OVERLAPS, "rt_overlap_boxes: no scene uploaded", "rt_overlap_boxes: null boxes / results",
     "rt_overlap_boxes: bad kernel", "rt_overlap_boxes: negative box count", "rt_overlap_boxes: max_tris must be 0..16",
     "rt_overlap_boxes: count_all must be 0 or 1", "rt_overlap_boxes: max_tris = 0 needs count_all",
     "rt_overlap_boxes: a counting query needs a count output"},
    {rtq::SWEEP, "rt_sweep_spheres: no scene uploaded", "rt_sweep_spheres: null spheres / results",
     "rt_sweep_spheres: bad kernel", "rt_sweep_spheres: negative sphere count", nullptr, nullptr, nullptr, nullptr},
    {rtq::CONTACTS, "rt_sweep_contacts: no scene uploaded", "rt_sweep_contacts: null spheres / results",
     "rt_sweep_contacts: bad kernel", "rt_sweep_contacts: negative sphere count",
     "rt_sweep_contacts: max_tris must be 0..16", "rt_sweep_contacts: count_all must be 0 or 1",
     "rt_sweep_contacts: max_tris = 0 needs count_all", "rt_sweep_contacts: a counting query needs a count output"},
    {rtq::CUTS, "rt_cut_triangles: no scene uploaded", "rt_cut_triangles: null tris / results",
     "rt_cut_triangles: bad kernel", "rt_cut_triangles: negative triangle count",
     "rt_cut_triangles: max_tris must be 0..16", "rt_cut_triangles: count_all must be 0 or 1",
     "rt_cut_triangles: max_tris = 0 needs count_all", "rt_cut_triangles: a counting query needs a count output"},
    {rtq::CLEARANCE, "rt_clearance_triangles: no scene uploaded", "rt_clearance_triangles: null tris / results",
     "rt_clearance_triangles: bad kernel", "rt_clearance_triangles: negative triangle count", nullptr, nullptr, nullptr,
     nullptr},
};

// a check's status and message in one; "" with RT_OK, and then err must be left as it was
struct Got {
    int rc;
    std::string err;
};
static const char* const UNTOUCHED = "(untouched)";
static Got enter(rtq::Fam f, bool has_scene, bool have_args) {
    Got g{0, UNTOUCHED};
    g.rc = rtq::check_enter(f, has_scene, have_args, g.err);
    return g;
}
static Got args(rtq::Fam f, int kernel, int n, int cap, int count_all) {
    Got g{0, UNTOUCHED};
    g.rc = rtq::FAMILY[f].cap ? rtq::check_args(f, kernel, n, cap, count_all, g.err) : rtq::check_args(f, kernel, n, g.err);
    return g;
}
static Got count_out(rtq::Fam f, int n, int cap, bool has_count) {
    Got g{0, UNTOUCHED};
    g.rc = rtq::check_count_out(f, n, cap, has_count, g.err);
    return g;
}
static bool ok(const Got& g) { return g.rc == RT_OK && g.err == UNTOUCHED; }
static bool refused(const Got& g, int rc, const char* msg) { return g.rc == rc && g.err == msg; }

static void test_messages() {
    for (int i = 0; i < rtq::NFAM; i++) {
        const Expect& e = EXPECT[i];
        const rtq::Fam f = e.f;
        CHECK((int)f == i);
        const bool list = rtq::FAMILY[f].cap != nullptr;
        CHECK(list == (e.cap_range != nullptr));
        // scene before arguments
        CHECK(ok(enter(f, true, true)));
        CHECK(refused(enter(f, false, true), RT_E_STATE, e.no_scene));
        CHECK(refused(enter(f, false, false), RT_E_STATE, e.no_scene));
        CHECK(refused(enter(f, true, false), RT_E_ARG, e.null_args));
        // kernel: RT_KERNEL_AUTO .. RT_KERNEL_FAST
        for (int k : {RT_KERNEL_AUTO, RT_KERNEL_STRICT, RT_KERNEL_FAST}) CHECK(ok(args(f, k, 5, 4, 0)));
        CHECK(refused(args(f, RT_KERNEL_AUTO - 1, 5, 4, 0), RT_E_ARG, e.bad_kernel));
        CHECK(refused(args(f, RT_KERNEL_FAST + 1, 5, 4, 0), RT_E_ARG, e.bad_kernel));
        // n >= 0; the kernel is checked first
        CHECK(ok(args(f, RT_KERNEL_FAST, 0, 4, 0)));
        CHECK(ok(args(f, RT_KERNEL_FAST, INT_MAX, 4, 0)));
        CHECK(refused(args(f, RT_KERNEL_FAST, -1, 4, 0), RT_E_ARG, e.negative));
        CHECK(refused(args(f, 3, -1, 4, 0), RT_E_ARG, e.bad_kernel));
        if (!list) {
            CHECK(std::string(rtq::FAMILY[f].fn) + ": bad kernel" == e.bad_kernel);
            continue;
        }
        // capacity 0..16, then count_all 0 / 1, then capacity 0 only with count_all; n is checked before them
        CHECK(ok(args(f, RT_KERNEL_FAST, 5, 16, 1)));
        CHECK(ok(args(f, RT_KERNEL_FAST, 5, 0, 1)));
        CHECK(ok(args(f, RT_KERNEL_FAST, 5, 1, 0)));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, -1, 1), RT_E_ARG, e.cap_range));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, 17, 1), RT_E_ARG, e.cap_range));
        CHECK(refused(args(f, RT_KERNEL_FAST, -1, 17, 1), RT_E_ARG, e.negative));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, 4, 2), RT_E_ARG, e.count_all));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, 4, -1), RT_E_ARG, e.count_all));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, 17, 2), RT_E_ARG, e.cap_range));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, 0, 0), RT_E_ARG, e.needs_count_all));
        CHECK(refused(args(f, RT_KERNEL_FAST, 5, 0, 2), RT_E_ARG, e.count_all));
        // a counting query (capacity 0) of n > 0 needs its count output
        CHECK(refused(count_out(f, 1, 0, false), RT_E_ARG, e.count_out));
        CHECK(ok(count_out(f, 1, 0, true)));
        CHECK(ok(count_out(f, 0, 0, false)));
        CHECK(ok(count_out(f, 1, 1, false)));
    }
}

// ---------------------------------------------------------------- list capacity
static void test_capacity() {
    const int cap[7] = {0, 1, 4, 5, 8, 9, 16}, built[7] = {0, 4, 4, 8, 8, 16, 16};
    for (int i = 0; i < 7; i++) CHECK(rtq::list_capacity(cap[i]) == built[i]);
    for (int c = 0; c <= rtq::LIST_MAX; c++) CHECK(rtq::list_capacity(c) >= c && (c == 0) == (rtq::list_capacity(c) == 0));
    static_assert(rtq::list_capacity(16) == rtq::LIST_MAX, "the largest build holds the largest list");
}

// ---------------------------------------------------------------- grid
static void test_grid() {
    const int CHUNK = 256, RES = 2048;  // (256 CUs x 8)
    // four chunks per workgroup: 1 .. 1024 queries one workgroup, 1025 two
    CHECK(rtq::grid_blocks(1, CHUNK, RES) == 1);
    CHECK(rtq::grid_blocks(1024, CHUNK, RES) == 1);
    CHECK(rtq::grid_blocks(1025, CHUNK, RES) == 2);
    // never more than the resident workgroups, which 4 x resident - 3 chunks already fill
    const int full = 4 * RES * CHUNK;
    CHECK(rtq::grid_blocks(full - 4 * CHUNK, CHUNK, RES) == RES - 1);      // 4 x resident - 4 chunks
    CHECK(rtq::grid_blocks(full - 4 * CHUNK + 1, CHUNK, RES) == RES);      // 4 x resident - 3
    CHECK(rtq::grid_blocks(full - CHUNK, CHUNK, RES) == RES);              // 4 x resident - 1
    CHECK(rtq::grid_blocks(full, CHUNK, RES) == RES);                      // 4 x resident
    CHECK(rtq::grid_blocks(full + 1, CHUNK, RES) == RES);                  // 4 x resident + 1
    CHECK(rtq::grid_blocks(full + 64 * CHUNK, CHUNK, RES) == RES);
    // the chunk count is computed in 64 bits: INT_MAX + 255 does not wrap
    CHECK(rtq::grid_blocks(INT_MAX, CHUNK, RES) == RES);
    CHECK(rtq::grid_blocks(INT_MAX, CHUNK, INT_MAX) == (INT_MAX / CHUNK + 1 + 3) / 4);
    // at least one workgroup, whatever the occupancy query said
    CHECK(rtq::grid_blocks(1, CHUNK, 0) == 1);
    CHECK(rtq::grid_blocks(5000, CHUNK, 1) == 1);
}

int main() {
    test_messages();
    test_capacity();
    test_grid();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
