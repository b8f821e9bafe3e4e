// Host-only checks of a render launch's decisions (parallel-ray-tracer_amd/csrc/hip/rt_launch_logic.hpp), compiled
// with plain g++ by tests/test_launch_logic.py: no GPU, no HIP.
//   * check_frame: every rejected edge next to its accepted neighbour, the messages verbatim;
//   * centre_out / region_layout: permutations, SUPER runs, region partitions that keep the order;
//   * the static default rule as a table (variant asked, capabilities) -> variant run; the shape keys;
//   * the trial scheduler in both loop orders, event-slot reuse, the two deciders;
//   * the hybrid rule's tile lists on a 20 x 12 frame (3 x 2 tiles, right column and bottom row partial);
//   * the hybrid launch's grid split.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "rt_launch_logic.hpp"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                                   \
        }                                                                 \
    } while (0)

// ---------------------------------------------------------------- frame checks
static rt_frame frame(int W, int H, int off, int stride, int rows) {
    rt_frame f;
    std::memset(&f, 0, sizeof f);
    f.width = W;
    f.height = H;
    f.row_offset = off;
    f.row_stride = stride;
    f.n_rows = rows;
    f.bounces = 4;
    f.spp = 1;
    return f;
}
static std::string why(const rt_frame& f, int n_frames = 1, int* grid = nullptr) {
    int g = 0;
    const char* w = rtl::check_frame(f, n_frames, g);
    if (grid) *grid = g;
    return w ? w : "";
}

static void test_check_frame() {
    const std::string ROWS = "rt_render: rows outside the frame";
    const std::string SPP = "rt_render: spp must be a square 1..256";
    const std::string BOUNCES = "rt_render: bounces must be 1..8";
    const std::string FRAMES = "rt_render_frames: n_frames must be 1..4096";
    const std::string SHIFT = "rt_render: frame_shift needs RT_KERNEL_FAST";
    const std::string PIXELS = "rt_render: the launch's frames x pixels exceed 2^31 - 1";
    const std::string WIDE = "rt_render: spp > 1 frames are at most 65535 pixels wide and 65535 rows high";
    const std::string CONFIG = "rt_render: bad launch configuration (variant / tune / waves_cap / dealing / regroup)";
    rt_frame f = frame(16, 16, 0, 1, 16);
    int g = 0;
    CHECK(why(f, 1, &g) == "" && g == 1);
    // spp: a square 1..256
    const int spps[5] = {0, 2, 4, 256, 289}, grids[5] = {0, 0, 2, 16, 0};
    for (int i = 0; i < 5; i++) {
        rt_frame s = f;
        s.spp = spps[i];
        CHECK(why(s, 1, &g) == (grids[i] ? "" : SPP));
        if (grids[i]) CHECK(g == grids[i]);
    }
    // bounces 1..8
    const int bs[4] = {0, 1, 8, 9};
    for (int i = 0; i < 4; i++) {
        rt_frame s = f;
        s.bounces = bs[i];
        CHECK(why(s) == (i == 1 || i == 2 ? "" : BOUNCES));
    }
    // the last row: rows 0, 2, ..., 14 (single rows); rows 0 1 2, 6 7 (blocks of 3, stride 6): last row 7
    rt_frame r1 = frame(16, 15, 0, 2, 8);
    CHECK(why(r1) == "");  // last row 14 = height - 1
    r1.height = 14;
    CHECK(why(r1) == ROWS);  // last row 14 = height
    rt_frame r3 = frame(16, 8, 0, 6, 5);
    r3.row_block = 3;
    CHECK(why(r3) == "");
    r3.height = 7;
    CHECK(why(r3) == ROWS);
    r3.height = 8;
    r3.row_stride = 2;  // blocks of 3 overlap at stride 2
    CHECK(why(r3) == ROWS);
    // frame_shift: the offset is a residue of the stride; fast kernels only
    rt_frame fs = frame(16, 16, 1, 2, 8);
    fs.frame_shift = 1;
    fs.kernel = RT_KERNEL_FAST;
    CHECK(why(fs, 4) == "");
    fs.row_offset = 2;
    CHECK(why(fs, 4) == ROWS);
    fs.row_offset = 1;
    fs.kernel = RT_KERNEL_STRICT;
    CHECK(why(fs, 4) == SHIFT);
    fs.kernel = RT_KERNEL_AUTO;
    CHECK(why(fs, 4) == "");
    // n_frames 1..4096
    CHECK(why(f, 0) == FRAMES);
    CHECK(why(f, 1) == "");
    CHECK(why(f, 4096) == "");
    CHECK(why(f, 4097) == FRAMES);
    // frames x pixels: 2^31 - 1 (a prime: one row of that many pixels) and one more
    CHECK(why(frame(INT_MAX, 1, 0, 1, 1)) == "");
    CHECK(why(frame(65536, 32768, 0, 1, 32768)) == PIXELS);
    CHECK(why(frame(32768, 32768, 0, 1, 32768), 1) == "");
    CHECK(why(frame(32768, 32768, 0, 1, 32768), 2) == PIXELS);
    // spp > 1: 16-bit x and row
    rt_frame w = frame(65535, 1, 0, 1, 1);
    w.spp = 4;
    CHECK(why(w) == "");
    w.width = 65536;
    CHECK(why(w) == WIDE);
    w.spp = 1;
    CHECK(why(w) == "");
    // the launch configuration
    rt_frame c = f;
    c.variant = 3;  // (a removed variant)
    CHECK(why(c) == CONFIG);
    c.variant = RT_VARIANT_SHDEFER;
    CHECK(why(c) == "");
    c.waves_cap = 9;
    CHECK(why(c) == CONFIG);
    c.waves_cap = 8;
    c.dealing = RT_DEAL_ROW_MAJOR + 1;
    CHECK(why(c) == CONFIG);
    c.dealing = RT_DEAL_ROW_MAJOR;
    c.hot_pct = 101;
    CHECK(why(c) == CONFIG);
    c.hot_pct = 100;
    CHECK(why(c) == "");
    c.kernel = 3;
    CHECK(why(c) == "rt_render: bad kernel");
}

// ---------------------------------------------------------------- tile orders
static bool is_permutation(const std::vector<int>& v, int n) {
    std::set<int> s(v.begin(), v.end());
    return (int)v.size() == n && (int)s.size() == n && (n == 0 || (*s.begin() == 0 && *s.rbegin() == n - 1));
}

static void test_centre_out() {
    const int grids[4][2] = {{1, 1}, {3, 2}, {5, 3}, {9, 8}};
    for (const auto& gr : grids) {
        const int tx = gr[0], ty = gr[1];
        const std::vector<int> ord = rtl::centre_out(tx, ty);
        CHECK(is_permutation(ord, tx * ty));
        // the tiles of one SUPER run of a row: adjacent in the order, left to right
        std::vector<int> pos(ord.size());
        for (size_t i = 0; i < ord.size(); i++) pos[ord[i]] = (int)i;
        for (int y = 0; y < ty; y++)
            for (int x = 0; x + 1 < tx; x++)
                if (x / rtl::SUPER == (x + 1) / rtl::SUPER) CHECK(pos[y * tx + x + 1] == pos[y * tx + x] + 1);
    }
    // 9 x 8: the first tile belongs to the run whose centre is nearest the grid's (4.5, 4)
    const std::vector<int> ord = rtl::centre_out(9, 8);
    auto run_d2 = [](int t) {
        const int x0 = (t % 9) / rtl::SUPER * rtl::SUPER, x1 = std::min(9, x0 + rtl::SUPER);
        const double dx = 0.5 * (x0 + x1) - 4.5, dy = t / 9 + 0.5 - 4.0;
        return dx * dx + dy * dy;
    };
    for (int t = 0; t < 72; t++) CHECK(run_d2(ord[0]) <= run_d2(t));
    CHECK(ord[0] == 3 * 9 + 4);  // (the runs at columns 4..7 of rows 3 and 4 tie: the upper row first)
}

static int region_of(int t, int tx, int ty, int mode) {
    const int x = t % tx, y = t / tx;
    if (mode == 1) return y * 8 / ty;
    if (mode == 2) return x * 8 / tx;
    return x * 4 / tx + 4 * (y * 2 / ty);
}
// is `lay` the region layout of the tiles of `ord` (a subset of a tx x ty grid), each region in ord's order?
static void check_layout(const std::vector<int>& lay, const std::vector<int>& ord, int tx, int ty, int mode) {
    const int n = (int)ord.size();
    CHECK((int)lay.size() == 9 + n);
    if ((int)lay.size() != 9 + n) return;
    CHECK(lay[0] == 0 && lay[8] == n);
    for (int r = 0; r < 8; r++) CHECK(lay[r] <= lay[r + 1]);
    std::vector<int> pos(tx * ty, -1);
    for (int i = 0; i < n; i++) pos[ord[i]] = i;
    std::set<int> seen;
    for (int r = 0; r < 8; r++)
        for (int i = lay[r]; i < lay[r + 1]; i++) {
            const int t = lay[9 + i];
            CHECK(t >= 0 && t < tx * ty && pos[t] >= 0);
            if (t < 0 || t >= tx * ty) continue;
            CHECK(seen.insert(t).second);
            CHECK(region_of(t, tx, ty, mode) == r);
            if (i > lay[r]) CHECK(pos[lay[9 + i - 1]] < pos[t]);
        }
    CHECK((int)seen.size() == n);
}

static void test_region_layout() {
    for (int mode = 1; mode <= 3; mode++) {
        check_layout(rtl::region_layout(rtl::centre_out(3, 2), 3, 2, mode), rtl::centre_out(3, 2), 3, 2, mode);
        check_layout(rtl::region_layout(rtl::centre_out(9, 8), 9, 8, mode), rtl::centre_out(9, 8), 9, 8, mode);
    }
    // two tile rows in 8 row bands: rows 0 and 1 fall in bands 0 and 4, the others stay empty
    const std::vector<int> lay = rtl::region_layout(rtl::centre_out(3, 2), 3, 2, 1);
    const int want[9] = {0, 3, 3, 3, 3, 6, 6, 6, 6};
    for (int r = 0; r <= 8; r++) CHECK(lay[r] == want[r]);
    // dealing -> layout mode
    CHECK(rtl::xcd_mode_of(RT_DEAL_DEFAULT, 16, true) == 3);
    CHECK(rtl::xcd_mode_of(RT_DEAL_DEFAULT, 16, false) == 1);
    CHECK(rtl::xcd_mode_of(RT_DEAL_DEFAULT, 1, true) == 1);
    CHECK(rtl::xcd_mode_of(RT_DEAL_ROWS, 16, true) == 1);
    CHECK(rtl::xcd_mode_of(RT_DEAL_COLUMNS, 1, false) == 2);
    CHECK(rtl::xcd_mode_of(RT_DEAL_BLOCKS, 1, false) == 3);
    CHECK(rtl::xcd_mode_of(RT_DEAL_GLOBAL, 16, true) == 0);
    CHECK(rtl::xcd_mode_of(RT_DEAL_ROW_MAJOR, 16, true) == 0);
    int tw = 0, th = 0;
    rtl::hot_tile(2, tw, th);
    CHECK(tw == 8 && th == 4);
    rtl::hot_tile(4, tw, th);
    CHECK(tw == 4 && th == 4);
}

// ---------------------------------------------------------------- the default rule
static rtl::Caps caps(bool wide, bool shp, bool shd, int lights, int frames, int spp = 1, int shift = 0,
                      bool trace = false) {
    rtl::Caps c;
    c.wide = wide;
    c.shp_ok = shp;
    c.shd_ok = shd;
    c.tile_trace = trace;
    c.n_lights = lights;
    c.n_frames = frames;
    c.frame_shift = shift;
    c.spp = spp;
    return c;
}

static void test_default_rule() {
    using rtl::resolve_variant;
    // default, a batch, two lights, room for the pool: one pool for all levels where it fits, else one per level
    CHECK(resolve_variant(caps(true, true, true, 2, 16), RT_VARIANT_DEFAULT) == RT_VARIANT_SHDEFER);
    CHECK(resolve_variant(caps(true, true, false, 2, 16), RT_VARIANT_DEFAULT) == RT_VARIANT_SHPOOL);
    CHECK(resolve_variant(caps(true, true, true, 2, 1, 4), RT_VARIANT_DEFAULT) == RT_VARIANT_SHDEFER);  // spp > 1
    // one light leaves nothing to pool; no room for the pool
    CHECK(resolve_variant(caps(true, true, true, 1, 16), RT_VARIANT_DEFAULT) == RT_VARIANT_PERSIST4);
    CHECK(resolve_variant(caps(true, false, false, 2, 16), RT_VARIANT_DEFAULT) == RT_VARIANT_PERSIST4);
    // a single 1-spp frame: the hybrid launch (k_persist where it cannot run)
    CHECK(resolve_variant(caps(true, true, true, 2, 1), RT_VARIANT_DEFAULT) == RT_VARIANT_HYBRID);
    CHECK(resolve_variant(caps(false, false, false, 2, 1), RT_VARIANT_DEFAULT) == RT_VARIANT_PERSIST);
    // hybrid asked for where it cannot run
    CHECK(resolve_variant(caps(true, true, true, 2, 1, 1, 1), RT_VARIANT_HYBRID) == RT_VARIANT_PERSIST);
    CHECK(resolve_variant(caps(true, true, true, 2, 1, 4), RT_VARIANT_HYBRID) == RT_VARIANT_PERSIST);
    CHECK(resolve_variant(caps(true, true, true, 2, 2), RT_VARIANT_HYBRID) == RT_VARIANT_PERSIST);
    CHECK(resolve_variant(caps(true, true, true, 2, 1), RT_VARIANT_HYBRID) == RT_VARIANT_HYBRID);
    // the pools without room: PERSIST4
    CHECK(resolve_variant(caps(true, false, false, 2, 1), RT_VARIANT_SHPOOL) == RT_VARIANT_PERSIST4);
    CHECK(resolve_variant(caps(true, true, false, 2, 1), RT_VARIANT_SHDEFER) == RT_VARIANT_PERSIST4);
    CHECK(resolve_variant(caps(true, true, false, 2, 1), RT_VARIANT_SHPOOL) == RT_VARIANT_SHPOOL);
    // k_coop walks the wide view
    CHECK(resolve_variant(caps(false, false, false, 2, 1), RT_VARIANT_COOP2) == RT_VARIANT_PERSIST);
    CHECK(resolve_variant(caps(false, false, false, 2, 1), RT_VARIANT_COOP4) == RT_VARIANT_PERSIST);
    CHECK(resolve_variant(caps(true, false, false, 2, 1), RT_VARIANT_COOP4) == RT_VARIANT_COOP4);
    // a tile trace runs the 3-wave kernel, whatever was asked
    for (int v : {RT_VARIANT_DEFAULT, RT_VARIANT_PERSIST, RT_VARIANT_PERSIST4, RT_VARIANT_COOP2, RT_VARIANT_HYBRID,
                  RT_VARIANT_SHPOOL, RT_VARIANT_SHDEFER})
        CHECK(resolve_variant(caps(true, true, true, 2, 1, 1, 0, true), v) == RT_VARIANT_PERSIST);
    CHECK(resolve_variant(caps(false, false, false, 1, 1), RT_VARIANT_PERSIST4) == RT_VARIANT_PERSIST4);
    // the whole-frame kernel of a single frame while the hybrid rule measures
    CHECK(rtl::single_rule(caps(true, true, true, 2, 1)) == RT_VARIANT_SHDEFER);
    CHECK(rtl::single_rule(caps(true, true, false, 2, 1)) == RT_VARIANT_SHPOOL);
    CHECK(rtl::single_rule(caps(true, true, true, 1, 1)) == RT_VARIANT_PERSIST);
    CHECK(rtl::single_rule(caps(true, false, false, 2, 1)) == RT_VARIANT_PERSIST);
    // the hybrid rule's candidates: the pool candidate is the rule's pool kernel, and only where it can run
    rtl::HotCand hc[rtl::NCAND];
    CHECK(rtl::hybrid_candidates(caps(true, true, true, 2, 1), 0, 0, hc) == 5);
    CHECK(hc[0].cold == RT_VARIANT_SHDEFER && hc[0].pct == 0 && hc[0].lpt);
    CHECK(rtl::hybrid_candidates(caps(true, true, false, 2, 1), 0, 0, hc) == 5 && hc[0].cold == RT_VARIANT_SHPOOL);
    CHECK(rtl::hybrid_candidates(caps(true, false, false, 2, 1), 0, 0, hc) == 4 && hc[0].cold == RT_VARIANT_PERSIST);
    CHECK(rtl::hybrid_candidates(caps(true, true, true, 2, 1), 30, RT_HOT_COOP2, hc) == 1);
    CHECK(hc[0].pct == 30 && hc[0].lanes == 2 && hc[0].cold == RT_VARIANT_PERSIST && !hc[0].lpt);
    CHECK(rtl::hybrid_candidates(caps(true, true, true, 2, 1), 30, RT_HOT_COOP4, hc) == 1 && hc[0].lanes == 4);
}

static void test_shape_key() {
    rt_frame f = frame(64, 64, 0, 1, 64);
    const rtl::ShapeKey b = rtl::batch_key(7, f, 16), h = rtl::hybrid_key(7, f);
    CHECK(b == rtl::batch_key(7, f, 16) && h == rtl::hybrid_key(7, f));
    CHECK(!(rtl::ShapeKey() == b) && !(rtl::ShapeKey() == h));  // (a fresh state matches no shape)
    CHECK(!(b == rtl::batch_key(8, f, 16)) && !(h == rtl::hybrid_key(8, f)));
    CHECK(!(b == rtl::batch_key(7, f, 17)));
    rt_frame g = f;
    g.row_block = 1;  // 0 and 1 both mean single rows
    CHECK(b == rtl::batch_key(7, g, 16) && h == rtl::hybrid_key(7, g));
    // the fields both rules look at
    int rt_frame::*both[] = {&rt_frame::width, &rt_frame::n_rows, &rt_frame::row_offset, &rt_frame::row_stride,
                             &rt_frame::bounces, &rt_frame::dealing};
    for (auto m : both) {
        g = f;
        g.*m += 1;
        CHECK(!(b == rtl::batch_key(7, g, 16)) && !(h == rtl::hybrid_key(7, g)));
    }
    g = f;
    g.row_block = 2;
    CHECK(!(b == rtl::batch_key(7, g, 16)) && !(h == rtl::hybrid_key(7, g)));
    // the batch rule's own: frame_shift, spp, waves_cap; the hybrid rule's own: hot_pct, hot_kernel
    int rt_frame::*batch_only[] = {&rt_frame::frame_shift, &rt_frame::spp, &rt_frame::waves_cap};
    for (auto m : batch_only) {
        g = f;
        g.*m += 1;
        CHECK(!(b == rtl::batch_key(7, g, 16)) && h == rtl::hybrid_key(7, g));
    }
    int rt_frame::*hybrid_only[] = {&rt_frame::hot_pct, &rt_frame::hot_kernel};
    for (auto m : hybrid_only) {
        g = f;
        g.*m += 1;
        CHECK(b == rtl::batch_key(7, g, 16) && !(h == rtl::hybrid_key(7, g)));
    }
    // neither looks at the height, the kernel, the variant or regroup
    int rt_frame::*neither[] = {&rt_frame::height, &rt_frame::kernel, &rt_frame::variant, &rt_frame::regroup};
    for (auto m : neither) {
        g = f;
        g.*m += 1;
        CHECK(b == rtl::batch_key(7, g, 16) && h == rtl::hybrid_key(7, g));
    }
}

// ---------------------------------------------------------------- trials
static void test_trials() {
    {  // two candidates x three rounds, round by round; one launch per call
        long long l[2 * 3] = {-1, -1, -1, -1, -1, -1};
        const int want[7] = {0, 1, 0, 1, 0, 1, -1};
        for (int i = 0; i < 7; i++) CHECK(rtl::next_trial(l, 2, 3, true, 100 + i) == want[i]);
        const long long marks[6] = {100, 102, 104, 101, 103, 105};  // [candidate][round]
        for (int i = 0; i < 6; i++) CHECK(l[i] == marks[i]);
        CHECK(rtl::latest_trial(l, 2, 3) == 105);
        // a trial whose event pair has been reused (NEV launches later) is tried again: first the oldest
        CHECK(rtl::next_trial(l, 2, 3, true, 100 + rtl::NEV - 1) == -1);
        CHECK(rtl::next_trial(l, 2, 3, true, 100 + rtl::NEV) == 0 && l[0] == 100 + rtl::NEV);
        CHECK(rtl::next_trial(l, 2, 3, true, 101 + rtl::NEV) == 1 && l[3] == 101 + rtl::NEV);
        CHECK(rtl::latest_trial(l, 2, 3) == 101 + rtl::NEV);
    }
    {  // five candidates x four rounds, candidate by candidate
        long long l[5 * 4];
        for (long long& x : l) x = -1;
        for (int i = 0; i < 20; i++) CHECK(rtl::next_trial(l, 5, 4, false, i) == i / 4);
        CHECK(rtl::next_trial(l, 5, 4, false, 20) == -1);
        for (int i = 0; i < 20; i++) CHECK(l[i] == i);
        CHECK(rtl::latest_trial(l, 5, 4) == 19);
        // (the rows of a wider array: the first three candidates only)
        CHECK(rtl::latest_trial(l, 3, 4) == 11);
        CHECK(rtl::next_trial(l, 5, 4, false, 1 + rtl::NEV) == 0 && l[0] == 1 + rtl::NEV && l[1] == 1);
    }
    {  // the latest is the maximum, wherever it stands
        const long long l[4] = {9, 3, 12, 5};
        CHECK(rtl::latest_trial(l, 2, 2) == 12);
    }
}

static void test_deciders() {
    float ms[rtl::NCAND];
    {  // short launches: the minimum (candidate 0: 10 < 20); its median (50, not over LONG_MS) would lose to 21
        float t[6] = {51.0f, 10.0f, rtl::LONG_MS, 22.0f, 20.0f, 21.0f};
        CHECK(rtl::batch_decide(t, 2, ms) == 0 && ms[0] == 10.0f && ms[1] == 20.0f);
    }
    {  // one candidate's median just over LONG_MS: the median for both (candidate 1: 21 < 50.00...)
        const float over = std::nextafter(rtl::LONG_MS, 100.0f);
        float t[6] = {51.0f, 10.0f, over, 22.0f, 20.0f, 21.0f};
        CHECK(rtl::batch_decide(t, 2, ms) == 1 && ms[0] == over && ms[1] == 21.0f);
    }
    {  // the long candidate second: still one statistic for both
        float t[6] = {22.0f, 20.0f, 21.0f, 10.0f, 60.0f, 61.0f};
        CHECK(rtl::batch_decide(t, 2, ms) == 0 && ms[0] == 21.0f && ms[1] == 60.0f);
    }
    {  // ties keep the earlier candidate
        float t[6] = {3.0f, 2.0f, 4.0f, 4.0f, 3.0f, 2.0f};
        CHECK(rtl::batch_decide(t, 2, ms) == 0);
        float u[6] = {70.0f, 60.0f, 80.0f, 80.0f, 70.0f, 60.0f};
        CHECK(rtl::batch_decide(u, 2, ms) == 0);
    }
    {  // hybrid: the median of the rounds after the warm one (with it, candidate 0 would show 2 and win)
        const float t[8] = {0.0f, 8.0f, 2.0f, 8.0f, 9.0f, 5.0f, 5.0f, 5.0f};
        CHECK(rtl::hybrid_decide(t, 2, ms) == 1 && ms[0] == 8.0f && ms[1] == 5.0f);
    }
    {  // ties keep the earlier candidate; the first strictly smaller wins
        const float t[12] = {1.0f, 4.0f, 6.0f, 5.0f, 0.0f, 5.0f, 5.0f, 9.0f, 0.0f, 4.0f, 9.0f, 1.0f};
        CHECK(rtl::hybrid_decide(t, 3, ms) == 2 && ms[0] == 5.0f && ms[1] == 5.0f && ms[2] == 4.0f);
        CHECK(rtl::hybrid_decide(t, 2, ms) == 0);
    }
}

// ---------------------------------------------------------------- the hybrid rule's tile lists
// 20 x 12 pixels: 3 x 2 tiles of 8 x 8, the right column 4 pixels wide, the bottom row 4 pixels high
constexpr int FW = 20, FH = 12, TX = 3, TY = 2, NT = 6;

// the hot 8x8 tiles by the rule's definition: over pct % of the maximum AND over twice the mean; hottest first (ties
// by index), at most half the tiles
static std::vector<int> hot_set(const std::vector<long long>& dur, int pct) {
    long long mx = 1, sum = 0;
    for (long long d : dur) {
        mx = std::max(mx, d);
        sum += d;
    }
    std::vector<int> hot;
    for (int t = 0; t < NT && pct > 0; t++)
        if (dur[t] * 100 > pct * mx && dur[t] * NT > 2 * sum) hot.push_back(t);
    std::stable_sort(hot.begin(), hot.end(), [&](int a, int b) { return dur[a] > dur[b]; });
    if (hot.size() > NT / 2) hot.resize(NT / 2);
    return hot;
}

static void check_lists(const std::vector<long long>& dur, const std::vector<int>& ord, int lanes, int cold_mode,
                        const std::vector<int>& want_hot) {
    const rtl::HotCand cand[4] = {{0, 0, RT_VARIANT_PERSIST, false},
                                  {45, lanes, RT_VARIANT_PERSIST, true},
                                  {45, lanes, RT_VARIANT_PERSIST, false},
                                  {0, 0, RT_VARIANT_PERSIST, true}};
    rtl::CandLists cl[4];
    const std::vector<int> lists = rtl::build_lists(dur, TX, TY, FW, FH, ord, cold_mode, cand, 4, cl);
    // the whole frame in plain order: no list
    CHECK(cl[0].at == 0 && cl[0].n_hot == 0 && cl[0].n_cold == 0 && cl[1].at == 0);
    int tw, th;
    rtl::hot_tile(lanes, tw, th);
    const int ctw = (FW + tw - 1) / tw, cth = (FH + th - 1) / th;
    std::vector<int> pos(NT);
    for (int i = 0; i < NT; i++) pos[ord[i]] = i;
    for (int c = 1; c < 4; c++) {
        const std::vector<int> hot8 = cand[c].pct ? hot_set(dur, cand[c].pct) : std::vector<int>();
        CHECK(hot8 == want_hot || !cand[c].pct);
        const size_t cold_len = (size_t)cl[c].n_cold + (cold_mode ? 9 : 0);
        CHECK(cl[c].at + cl[c].n_hot + cold_len == (c < 3 ? cl[c + 1].at : lists.size()));
        if (cl[c].at + cl[c].n_hot + cold_len > lists.size()) return;
        // the hot kernel's tiles: inside its grid, none twice, exactly the sub-tiles of the hot 8x8 tiles that hold
        // a pixel, the 8x8 tiles hottest first
        std::set<int> subs;
        std::vector<int> seq;  // the 8x8 tiles in the order their sub-tiles appear
        for (int i = 0; i < cl[c].n_hot; i++) {
            const int s = lists[cl[c].at + i];
            CHECK(s >= 0 && s < ctw * cth);
            CHECK(subs.insert(s).second);
            const int t = (s / ctw) * th / 8 * TX + (s % ctw) * tw / 8;
            if (seq.empty() || seq.back() != t) seq.push_back(t);
        }
        CHECK(seq == hot8);
        int want_subs = 0;
        for (int t : hot8)
            for (int y = t / TX * 8; y < std::min(FH, t / TX * 8 + 8); y += th)
                for (int x = t % TX * 8; x < std::min(FW, t % TX * 8 + 8); x += tw) {
                    want_subs++;
                    CHECK(subs.count(y / th * ctw + x / tw) == 1);
                }
        CHECK(cl[c].n_hot == want_subs);
        // the cold tiles: the rest of the grid
        std::vector<int> rest;
        for (int t : ord)
            if (std::find(hot8.begin(), hot8.end(), t) == hot8.end()) rest.push_back(t);
        CHECK(cl[c].n_cold == (int)rest.size());
        const int* cold = lists.data() + cl[c].at + cl[c].n_hot;
        std::vector<int> want = rest;  // the order within the list (within each region of a layout)
        if (cand[c].lpt) std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return dur[a] > dur[b]; });
        if (cold_mode) {
            check_layout(std::vector<int>(cold, cold + cold_len), want, TX, TY, cold_mode);
        } else {
            CHECK(std::vector<int>(cold, cold + cold_len) == want);
        }
        // costliest first, ties in the dealing order (within each region of a layout)
        const int* tiles = cold + (cold_mode ? 9 : 0);
        for (int r = 0; r < (cold_mode ? 8 : 1) && cand[c].lpt; r++) {
            const int i0 = cold_mode ? cold[r] : 0, i1 = cold_mode ? cold[r + 1] : cl[c].n_cold;
            for (int i = i0 + 1; i < i1; i++) {
                const int a = tiles[i - 1], b = tiles[i];
                CHECK(dur[a] > dur[b] || (dur[a] == dur[b] && pos[a] < pos[b]));
            }
        }
    }
}

static void test_lists() {
    // A: tile 3 is over 45 % of the maximum (60 > 45) but not over twice the mean (60 x 6 = 360 <= 2 x 200): cold
    const std::vector<long long> A = {100, 10, 10, 60, 10, 10};
    // B: two hot tiles, the hotter one second by index; a full tile and one of the bottom row; equal cold durations
    const std::vector<long long> B = {90, 10, 10, 100, 5, 5};
    // C: the corner tile (4 x 4 pixels) and its neighbour in the bottom row
    const std::vector<long long> C = {5, 5, 10, 10, 90, 100};
    // D: nothing stands out: no hot tile
    const std::vector<long long> D = {10, 10, 10, 10, 10, 10};
    // The half-the-tiles cap cannot bite while a hot tile must be over twice the mean: k tiles over 2 x mean hold
    // more than 2k / n of the sum, so k < n / 2. E is the densest case, two of six tiles (three would need more than
    // the whole sum); the cap's arithmetic is checked on hot_set's side only.
    const std::vector<long long> E = {100, 100, 1, 1, 1, 1};
    std::vector<int> row_major(NT);
    for (int i = 0; i < NT; i++) row_major[i] = i;
    for (int lanes : {4, 2})
        for (const std::vector<int>& ord : {rtl::centre_out(TX, TY), row_major})
            for (int mode = 0; mode <= 3; mode++) {
                check_lists(A, ord, lanes, mode, {0});
                check_lists(B, ord, lanes, mode, {3, 0});
                check_lists(C, ord, lanes, mode, {5, 4});
                check_lists(D, ord, lanes, mode, {});
                check_lists(E, ord, lanes, mode, {0, 1});
            }
    // the clipped sub-tiles by number: k_coop<4> has 4 x 4 tiles (5 x 3 of them), k_coop<2> 8 x 4 (3 x 3)
    const rtl::HotCand c4 = {45, 4, RT_VARIANT_PERSIST, false}, c2 = {45, 2, RT_VARIANT_PERSIST, false};
    rtl::CandLists cl;
    std::vector<int> l = rtl::build_lists(C, TX, TY, FW, FH, row_major, 0, &c4, 1, &cl);
    CHECK(cl.n_hot == 3 && l[0] == 2 * 5 + 4 && l[1] == 2 * 5 + 2 && l[2] == 2 * 5 + 3);
    l = rtl::build_lists(C, TX, TY, FW, FH, row_major, 0, &c2, 1, &cl);
    CHECK(cl.n_hot == 2 && l[0] == 2 * 3 + 2 && l[1] == 2 * 3 + 1);
    l = rtl::build_lists(B, TX, TY, FW, FH, row_major, 0, &c4, 1, &cl);
    CHECK(cl.n_hot == 6 && cl.n_cold == 4 && l.size() == 10);
    CHECK(l[0] == 2 * 5 && l[1] == 2 * 5 + 1 && l[2] == 0 && l[3] == 1 && l[4] == 5 && l[5] == 6);
}

static void test_grids() {
    int nc = -1, np = -1;
    rtl::hybrid_grids(1024, 512, 0, 100, nc, np);  // no hot tiles: no hot grid, the cold one by its tiles
    CHECK(nc == 0 && np == 25);
    rtl::hybrid_grids(1024, 512, 0, 100000, nc, np);
    CHECK(nc == 0 && np == 1024);
    rtl::hybrid_grids(1024, 512, 1, 100000, nc, np);  // one hot tile: one workgroup, its share off the cold grid
    CHECK(nc == 1 && np == 1024 - 2);
    rtl::hybrid_grids(1024, 512, 40, 100000, nc, np);
    CHECK(nc == 10 && np == 1024 - 20);
    rtl::hybrid_grids(1024, 512, 100000, 100000, nc, np);  // at most half the hot kernel's resident grid
    CHECK(nc == 256 && np == 512);
    rtl::hybrid_grids(768, 513, 100000, 100000, nc, np);
    CHECK(nc == 256 && np == 768 - 256 * 768 / 513);
    rtl::hybrid_grids(1024, 512, 100000, 0, nc, np);  // never an empty cold grid
    CHECK(nc == 256 && np == 1);
    rtl::hybrid_grids(1, 2, 100000, 100000, nc, np);
    CHECK(nc == 1 && np == 1);
    for (int rcp : {2, 3, 256, 1024})
        for (int n_hot : {1, 7, 5000}) {
            rtl::hybrid_grids(1024, rcp, n_hot, 5000, nc, np);
            CHECK(nc >= 1 && nc <= std::max(1, rcp / 2) && np >= 1 && np <= 1024);
        }
}

int main() {
    test_check_frame();
    test_centre_out();
    test_region_layout();
    test_default_rule();
    test_shape_key();
    test_trials();
    test_deciders();
    test_lists();
    test_grids();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
