// rt_launch_logic.hpp — the host-side decisions of a render launch (render_batch and its steps, rt_hip.hip), kept free
// of HIP so that tests/c/launch_logic_test.cpp can check them with g++ alone:
//   * check_frame: the rt_frame / n_frames argument checks and their messages;
//   * centre_out, region_layout, xcd_mode_of, hot_tile: the tile dealing orders and their XCD-region layout;
//   * Caps and the static default rule: which variant a request runs, given what the scene and the frame allow;
//   * ShapeKey: the shape a measured rule's state belongs to (batch rule and hybrid rule);
//   * next_trial / latest_trial, batch_decide / hybrid_decide: the trial scheduler and the two deciders;
//   * hybrid_candidates, build_lists: the hybrid rule's candidate table and their hot / cold tile lists;
//   * hybrid_grids: the split of the chip between the hot and the cold kernel's grid.
// Reading HIP events, allocating and launching stay in rt_hip.hip.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

#include "rt_hip.h"

namespace rtl {

// ---------------------------------------------------------------- frame checks
// What is wrong with a render call's frame (rt_render / rt_render_frames), or null when it is good; spp_grid: the
// side of the spp sample grid.
inline const char* check_frame(const rt_frame& f, int n_frames, int& spp_grid) {
    spp_grid = 1;
    if (n_frames < 1 || n_frames > 4096) return "rt_render_frames: n_frames must be 1..4096";
    const int rb = f.row_block > 1 ? f.row_block : 1;
    const int fs = f.frame_shift;
    if (f.width <= 0 || f.height <= 0 || f.row_stride <= 0 || f.n_rows <= 0 || f.row_offset < 0 || f.row_block < 0 ||
        fs < 0 || (f.n_rows > rb && f.row_stride < rb) ||
        (fs == 0 && (long long)f.row_offset + (long long)((f.n_rows - 1) / rb) * f.row_stride + (f.n_rows - 1) % rb >=
                        f.height) ||
        (fs > 0 && (f.row_offset >= f.row_stride || f.row_offset >= f.height ||
                    (long long)f.n_rows > (long long)f.row_stride * f.height)))
        return "rt_render: rows outside the frame";
    if (fs > 0 && f.kernel != RT_KERNEL_FAST && f.kernel != RT_KERNEL_AUTO)
        return "rt_render: frame_shift needs RT_KERNEL_FAST";
    if (f.bounces < 1 || f.bounces > 8) return "rt_render: bounces must be 1..8";
    int g = 1;
    while (g * g < f.spp) g++;
    if (f.spp < 1 || g * g != f.spp || g > 16) return "rt_render: spp must be a square 1..256";
    spp_grid = g;
    if (f.kernel < RT_KERNEL_AUTO || f.kernel > RT_KERNEL_FAST) return "rt_render: bad kernel";
    if (f.spp > 1 && (f.width > 65535 || f.n_rows > 65535))  // (k_persist's multi-sample slots pack x and the row)
        return "rt_render: spp > 1 frames are at most 65535 pixels wide and 65535 rows high";
    // (variants 3, 6, 7, 8, 9, 10, 12, 14 -- the split pipeline, k_coop<8>, k_fan, k_chain, k_pool, k_relay, k_stream
    // -- measured slower than k_persist and were removed: refused)
    const bool known = f.variant == RT_VARIANT_DEFAULT || f.variant == RT_VARIANT_PERSIST ||
                       f.variant == RT_VARIANT_PERSIST4 || f.variant == RT_VARIANT_COOP2 ||
                       f.variant == RT_VARIANT_COOP4 || f.variant == RT_VARIANT_HYBRID ||
                       f.variant == RT_VARIANT_SHPOOL || f.variant == RT_VARIANT_SHDEFER;
    if (!known || f.hot_pct < 0 || f.hot_pct > 100 || f.hot_kernel < RT_HOT_COOP4 || f.hot_kernel > RT_HOT_COOP2 ||
        f.tune < 0 || f.tune > 1 || f.waves_cap < 0 || f.waves_cap > 8 || f.dealing < RT_DEAL_DEFAULT ||
        f.dealing > RT_DEAL_ROW_MAJOR || f.regroup < 0 || f.regroup > 64)
        return "rt_render: bad launch configuration (variant / tune / waves_cap / dealing / regroup)";
    // (the kernels index a launch's output pixels with 32-bit integers)
    if ((size_t)f.width * f.n_rows * (size_t)n_frames > (size_t)INT_MAX)
        return "rt_render: the launch's frames x pixels exceed 2^31 - 1";
    return nullptr;
}

// ---------------------------------------------------------------- tile orders
// Centre-out order of a tx x ty tile grid (the persistent kernels' default dealing order), by runs of SUPER tiles
// side by side in a row: an 8x8 tile of 4-B pixels stores 32-B row pieces, so SUPER = 4 neighbouring tiles fill
// whole 128-B lines, and dealt back to back they are written while the line is still in the XCD's L2 (a line
// left partly written leaves L2 once per piece: WRITE_SIZE).
constexpr int SUPER = 4;
inline std::vector<int> centre_out(int tx, int ty) {
    const int n = tx * ty;
    std::vector<int> ord(n);
    for (int i = 0; i < n; i++) ord[i] = i;
    const float cx = 0.5f * tx, cy = 0.5f * ty;
    auto d2 = [&](int t) {
        const int x0 = (t % tx) / SUPER * SUPER, x1 = std::min(tx, x0 + SUPER);
        const float dx = 0.5f * (x0 + x1) - cx, dy = t / tx + 0.5f - cy;
        return dx * dx + dy * dy;
    };
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
        const float da = d2(a), db = d2(b);
        if (da != db) return da < db;
        return a / tx != b / tx ? a / tx < b / tx : a < b;  // a run's tiles together, left to right
    });
    return ord;
}

// XCD-aware layout of a dealing order (rtd::next_item): 9 region offsets into the tile part, then the tiles of
// region 0..7, each region in the order's order. mode 1: 8 bands of tile rows, 2: 8 bands of tile columns,
// 3: 4 x 2 blocks.
inline std::vector<int> region_layout(const std::vector<int>& ord, int tx, int ty, int mode) {
    std::vector<int> dev(9 + ord.size());
    int at = 9;
    for (int r = 0; r < 8; r++) {
        dev[r] = at;
        for (int t : ord) {
            const int reg = mode == 1 ? (t / tx) * 8 / ty : mode == 2 ? (t % tx) * 8 / tx
                                                                    : (t % tx) * 4 / tx + 4 * ((t / tx) * 2 / ty);
            if (reg == r) dev[at++] = t;
        }
    }
    dev[8] = at;
    for (int r = 0; r <= 8; r++) dev[r] -= 9;  // offsets into the order part
    return dev;
}

// XCD-aware dealing of k_persist: the centre-out order split into 8 spatial regions, region r drained first by
// the workgroups on XCD r (rtd::next_item), so each XCD's L2 holds the part of the scene its region's rays
// touch. rt_frame.dealing: BLOCKS = 4 x 2 blocks of tiles, ROWS = 8 bands of tile rows, COLUMNS = 8 bands of
// tile columns, GLOBAL = one counter. Same-box, ms per frame: 16-frame batches of the full frame, dragon 1.060
// (global) / 0.938 (blocks) / 0.980 (rows) / 0.942 (columns), sportscar 0.599 / 0.504, car_boxed 1.067 / 1.041;
// a single frame 1.862 / 1.871 (blocks) / 1.732 (rows); an 8-GPU rank's rows, batched, 0.220 / 0.208 (blocks) /
// 0.202 (rows). Default: blocks for batches of the full frame, row bands otherwise. The region_layout mode (0: none).
inline int xcd_mode_of(int dealing, int n_frames, bool full_frame) {
    return dealing == RT_DEAL_DEFAULT ? (n_frames > 1 && full_frame ? 3 : 1)
           : dealing == RT_DEAL_ROWS    ? 1
           : dealing == RT_DEAL_COLUMNS ? 2
           : dealing == RT_DEAL_BLOCKS  ? 3
                                        : 0;
}

// pixel tile of a group kernel (rtd::GTile): k_coop<2> 8x4, k_coop<4> 4x4
inline void hot_tile(int g, int& tw, int& th) {
    tw = g == 2 ? 8 : 4;
    th = 4;
}

// ---------------------------------------------------------------- the static default rule
// What a launch's scene and frame allow: a wide view to walk (and RT_KERNEL_FAST), room for the per-level shadow pool
// (1..32 lights, packed builds, its LDS path buffer at 4 workgroups per CU) and for the all-levels one (<= 8 lights,
// its larger LDS layout), a diagnostics tile trace
struct Caps {
    bool wide = false, shp_ok = false, shd_ok = false, tile_trace = false;
    int n_lights = 0, n_frames = 1, frame_shift = 0, spp = 1;
};

inline bool usable(const Caps& c, int v) {
    if (c.tile_trace) return v == RT_VARIANT_PERSIST;  // (diagnostics: the 3-wave kernel's tile trace)
    if (v == RT_VARIANT_COOP2 || v == RT_VARIANT_COOP4) return c.wide;
    if (v == RT_VARIANT_SHPOOL) return c.shp_ok;
    if (v == RT_VARIANT_SHDEFER) return c.shd_ok;
    if (v == RT_VARIANT_HYBRID) return c.wide && c.n_frames == 1 && c.frame_shift == 0 && c.spp == 1;
    return true;
}
// The default rule (measured): frame batches and spp > 1 fill the chip, so the kernel with the best
// throughput — the shadow pool for scenes of 2+ lights whose LDS path buffer fits (dragon 0.708 -> 0.666 ms per
// frame in 20-frame batches; one light leaves nothing to pool: car_boxed 0.868 vs 0.902), else k_persist at 4
// waves; a single 1-spp frame is tail-bound: the hybrid launch, which measures its candidates on the frames of
// the shape and keeps the fastest (k_persist where it cannot run).
inline bool pool_rule(const Caps& c) { return c.shp_ok && c.n_lights >= 2; }
// the pool kernel of the rules: one pool for all levels where its larger LDS path buffer fits (dragon 20-frame
// batches 0.655 -> 0.639 ms per frame, single frames 1.145 -> 1.091 ms; SIMD efficiency 0.59 -> 0.68), else one
// per level
inline int pool_v(const Caps& c) { return c.shd_ok ? RT_VARIANT_SHDEFER : RT_VARIANT_SHPOOL; }
// the static rule of frame batches and spp > 1 (what the measured batch rule starts from)
inline int batch_default(const Caps& c) { return pool_rule(c) ? pool_v(c) : RT_VARIANT_PERSIST4; }
// the variant a request (rt_frame.variant) runs
inline int resolve_variant(const Caps& c, int asked) {
    int mode = asked;
    if (mode == RT_VARIANT_DEFAULT) mode = (c.n_frames > 1 || c.spp > 1) ? batch_default(c) : RT_VARIANT_HYBRID;
    if ((mode == RT_VARIANT_SHPOOL && !c.shp_ok) || (mode == RT_VARIANT_SHDEFER && !c.shd_ok))
        mode = RT_VARIANT_PERSIST4;  // (no room for the pool: PERSIST4 itself)
    if (!usable(c, mode)) mode = RT_VARIANT_PERSIST;  // (no wide view, or a diagnostics trace)
    return mode;
}
// the whole-frame kernel of a single frame while the hybrid launch measures or tries its candidates
inline int single_rule(const Caps& c) { return pool_rule(c) ? pool_v(c) : RT_VARIANT_PERSIST; }

// ---------------------------------------------------------------- the shape a measured rule's state belongs to
// The batch rule keys on the first eight fields and shift, spp, frames, cap_req; the hybrid rule (single 1-spp frames
// without frame_shift) on the first eight and pct_req, hk_req. The other rule's fields stay 0 (batch_key, hybrid_key).
struct ShapeKey {
    long long scene = -1;  // rt_ctx::scene_gen of the upload
    int W = 0, rows = 0, off = 0, stride = 0, block = 0, bounces = 0, dealing = 0;
    int shift = 0, spp = 0, frames = 0, cap_req = 0;
    int pct_req = 0, hk_req = 0;
    bool operator==(const ShapeKey& o) const {
        return scene == o.scene && W == o.W && rows == o.rows && off == o.off && stride == o.stride &&
               block == o.block && bounces == o.bounces && dealing == o.dealing && shift == o.shift && spp == o.spp &&
               frames == o.frames && cap_req == o.cap_req && pct_req == o.pct_req && hk_req == o.hk_req;
    }
};
inline ShapeKey frame_key(long long scene, const rt_frame& f) {
    ShapeKey k;
    k.scene = scene;
    k.W = f.width;
    k.rows = f.n_rows;
    k.off = f.row_offset;
    k.stride = f.row_stride;
    k.block = f.row_block > 1 ? f.row_block : 1;
    k.bounces = f.bounces;
    k.dealing = f.dealing;
    return k;
}
inline ShapeKey batch_key(long long scene, const rt_frame& f, int n_frames) {
    ShapeKey k = frame_key(scene, f);
    k.shift = f.frame_shift;
    k.spp = f.spp;
    k.frames = n_frames;
    k.cap_req = f.waves_cap;
    return k;
}
inline ShapeKey hybrid_key(long long scene, const rt_frame& f) {
    ShapeKey k = frame_key(scene, f);
    k.pct_req = f.hot_pct;
    k.hk_req = f.hot_kernel;
    return k;
}

// ---------------------------------------------------------------- trials
// A rule's trials are timed by their launches' own HIP event pairs, a ring of NEV (rt_kernel_times): a trial's
// launch number names its pair for the NEV launches after it.
constexpr int NEV = 64;

// The next trial to launch: the first slot of launch[n_cand][rounds] (launch numbers, -1 = untried) that is untried
// or whose event pair has been reused since -- round by round over the candidates (round_major: 0, 1, 0, 1, ...) or
// candidate by candidate (0, 0, ..., 1, 1, ...). Marks the slot with launch number `now` and returns its candidate;
// -1 when every trial is enqueued.
inline int next_trial(long long* launch, int n_cand, int rounds, bool round_major, long long now) {
    const int n_outer = round_major ? rounds : n_cand, n_inner = round_major ? n_cand : rounds;
    for (int o = 0; o < n_outer; o++)
        for (int i = 0; i < n_inner; i++) {
            const int c = round_major ? i : o, r = round_major ? o : i;
            long long& l = launch[c * rounds + r];
            if (l < 0 || now - l >= NEV) {  // untried (or events reused)
                l = now;
                return c;
            }
        }
    return -1;
}
// the latest enqueued trial (the rule decides once it has run)
inline long long latest_trial(const long long* launch, int n_cand, int rounds) {
    long long last = 0;
    for (int i = 0; i < n_cand * rounds; i++) last = std::max(last, launch[i]);
    return last;
}

// The batch rule (frame batches and spp > 1: PERSIST4 or the pool kernel), trials per candidate: 3, decided by the
// minimum -- or, for launches longer than LONG_MS, the median (the 64-spp configuration's 190-ms launches of one
// kernel ranged 186-199 ms on one box; the minimum of two trials picked either kernel)
constexpr int BATCH_ROUNDS = 3;
constexpr float LONG_MS = 50.0f;
// t[n_cand][BATCH_ROUNDS]: the trials' times (sorted in place); ms[n_cand]: each candidate's statistic. One statistic
// for every candidate (like with like): the median when the launches are long (some candidate's median over LONG_MS),
// else the minimum. The first strictly smaller wins.
inline int batch_decide(float* t, int n_cand, float* ms) {
    constexpr int R = BATCH_ROUNDS;
    float med_max = 0.0f;
    for (int c = 0; c < n_cand; c++) {
        std::sort(t + c * R, t + (c + 1) * R);
        med_max = std::max(med_max, t[c * R + R / 2]);
    }
    const bool by_median = med_max > LONG_MS;
    for (int c = 0; c < n_cand; c++) ms[c] = by_median ? t[c * R + R / 2] : t[c * R];
    int choice = 0;
    for (int c = 1; c < n_cand; c++)
        if (ms[c] < ms[choice]) choice = c;
    return choice;
}

// The hybrid rule (single 1-spp frames), trial frames per candidate, back to back: the first untimed (its per-tile
// times feed the next one's lists), the best median of the other three chosen (single frames are noisy, and some
// two-stream launches bimodal). Back to back, not round robin: a hybrid candidate's lists are built from the frame
// before it, and after another candidate's frame they are not the lists it renders with once chosen (a car_boxed
// walkthrough priced its hot candidates 30-60 % slow and settled on none of them)
constexpr int HYBRID_ROUNDS = 4;
constexpr int HYBRID_WARM = 1;
// t[n_cand][HYBRID_ROUNDS]: the trials' times (the first HYBRID_WARM of a candidate are not looked at); ms[n_cand]:
// the median of each candidate's timed trials. The first strictly smaller wins.
inline int hybrid_decide(const float* t, int n_cand, float* ms) {
    constexpr int NT = HYBRID_ROUNDS - HYBRID_WARM;
    int best = 0;
    for (int c = 0; c < n_cand; c++) {
        float s[NT];
        std::copy(t + c * HYBRID_ROUNDS + HYBRID_WARM, t + (c + 1) * HYBRID_ROUNDS, s);
        std::sort(s, s + NT);
        ms[c] = s[NT / 2];
        if (ms[c] < ms[best]) best = c;
    }
    return best;
}

// ---------------------------------------------------------------- the hybrid rule's candidates and tile lists
// RT_VARIANT_HYBRID candidates: pct = 0: the cold kernel over the whole frame; else the 8x8 tiles slower than pct % of the
// slowest tile of the measuring frame go to k_coop with `lanes` lanes per ray while the cold kernel renders the rest
// (each candidate is tried HYBRID_ROUNDS times). Measured: car_boxed hot > 45 % k_coop<4>,
// sportscar hot > 60 % k_coop<2> / <4>, dragon the whole-frame kernels; k_fan and k_relay hot tiles never won
// (both removed).
// lpt: the cold tiles dealt costliest first by the measuring frame's per-tile times (longest processing time first,
// the classic makespan heuristic: a single frame ends with its slowest tile) instead of centre-out; with pct = 0 the
// whole frame that way.
struct HotCand {
    int pct, lanes, cold;
    bool lpt;
};
// The candidates are the configurations that won on some BASELINE scene (dragon the shadow pool in LPT
// order, car_boxed hot > 45 % k_coop<4> with LPT cold tiles, sportscar hot > 60 % k_coop<4> / <2>) plus k_persist in
// LPT order: few candidates keep the trial frames few (3 each) and the choice robust to frame-to-frame noise (a moving
// camera changes every trial frame's cost; nine candidates picked a 12 % slower one on a walkthrough).
// (RT_VARIANT_SHPOOL here stands for the rule's pool kernel: RT_VARIANT_SHDEFER where its path buffer fits.)
constexpr HotCand HYBRID_CANDS[] = {{0, 0, RT_VARIANT_SHPOOL, true},   {0, 0, RT_VARIANT_PERSIST, true},
                                    {45, 4, RT_VARIANT_PERSIST, true}, {60, 4, RT_VARIANT_PERSIST, false},
                                    {60, 2, RT_VARIANT_PERSIST, false}};
constexpr int NCAND = 12;  // candidates of a shape at most

// The candidates of a shape into out[NCAND]: rt_frame.hot_pct > 0 fixes one (no trials), else HYBRID_CANDS -- those
// whose cold kernel can run. Returns their number.
inline int hybrid_candidates(const Caps& caps, int hot_pct, int hot_kernel, HotCand* out) {
    int nc = 0;
    auto add = [&](HotCand hc) {
        if (hc.cold == RT_VARIANT_SHPOOL) hc.cold = pool_v(caps);  // (HYBRID_CANDS: "the pool kernel")
        if (nc >= NCAND || !usable(caps, hc.cold)) return;
        out[nc++] = hc;
    };
    if (hot_pct > 0) {
        add(HotCand{hot_pct, hot_kernel == RT_HOT_COOP2 ? 2 : 4, RT_VARIANT_PERSIST, false});
    } else {
        for (const HotCand& hc : HYBRID_CANDS) add(hc);
    }
    return nc;
}

// a candidate's lists within the concatenation: [n_hot tiles of the hot kernel][the cold 8x8 tiles: n_cold of them in
// dealing order, or their region layout (9 offsets first)] at `at`
struct CandLists {
    size_t at = 0;
    int n_hot = 0, n_cold = 0;
};

// The tile lists of every candidate, one after another, from a measuring frame's per-tile durations dur[tx * ty] of a
// W x n_rows frame. ord: the dealing order of the 8x8 tiles; cold_mode: the cold lists' region_layout mode (0: plain
// order). A tile is hot when its duration is over pct % of the maximum and over twice the mean (rt_feedback.hpp
// fb_tile); the costliest half of the tiles at most (k_coop costs ~2x the wave time). A whole-frame candidate in
// plain order (pct = 0, !lpt) has no list.
inline std::vector<int> build_lists(const std::vector<long long>& dur, int tx, int ty, int W, int n_rows,
                                    const std::vector<int>& ord, int cold_mode, const HotCand* cand, int nc,
                                    CandLists* out) {
    const size_t n_tiles = dur.size();
    long long cmax = 1, dsum = 0;
    for (size_t t = 0; t < n_tiles; t++) {
        cmax = std::max(cmax, dur[t]);
        dsum += dur[t];
    }
    std::vector<int> lists;
    for (int c = 0; c < nc; c++) {
        out[c].at = lists.size();
        out[c].n_hot = out[c].n_cold = 0;
        if (cand[c].pct == 0 && !cand[c].lpt) continue;
        std::vector<int> hot8;
        for (size_t t = 0; t < n_tiles && cand[c].pct > 0; t++)
            if (dur[t] * 100 > (long long)cand[c].pct * cmax && dur[t] * (long long)n_tiles > 2 * dsum)
                hot8.push_back((int)t);
        std::stable_sort(hot8.begin(), hot8.end(), [&](int a, int b) { return dur[a] > dur[b]; });
        if (hot8.size() > n_tiles / 2) hot8.resize(n_tiles / 2);
        std::vector<char> is_hot(n_tiles, 0);
        // each 8x8 tile = (8 / TW) x (8 / TH) tiles of the hot kernel (rtd::GTile), hottest first
        int tw, th;
        hot_tile(cand[c].lanes, tw, th);
        const int ctw = (W + tw - 1) / tw, cth = (n_rows + th - 1) / th;
        for (int t : hot8) {
            is_hot[t] = 1;
            for (int qy = 0; qy < 8 / th; qy++)
                for (int qx = 0; qx < 8 / tw; qx++) {
                    const int cx = (t % tx) * (8 / tw) + qx, cy = (t / tx) * (8 / th) + qy;
                    if (cx < ctw && cy < cth) lists.push_back(cy * ctw + cx);
                }
        }
        out[c].n_hot = (int)(lists.size() - out[c].at);
        std::vector<int> cold;
        for (int t : ord)
            if (!is_hot[t]) cold.push_back(t);
        if (cand[c].lpt)  // costliest first (ties: the dealing order)
            std::stable_sort(cold.begin(), cold.end(), [&](int a, int b) { return dur[a] > dur[b]; });
        out[c].n_cold = (int)cold.size();
        if (cold_mode) cold = region_layout(cold, tx, ty, cold_mode);
        lists.insert(lists.end(), cold.begin(), cold.end());
    }
    return lists;
}

// The hybrid launch's two persistent grids: nc workgroups of the hot kernel (rcp resident at most) for n_hot of its
// tiles -- sized to start every hot tile at once, at most half the chip; none without hot tiles -- and np of the cold
// kernel (rp resident at most) for n_cold 8x8 tiles on the share of the chip the hot grid leaves.
inline void hybrid_grids(int rp, int rcp, int n_hot, int n_cold, int& nc, int& np) {
    nc = n_hot > 0 ? std::max(1, std::min((n_hot + 3) / 4, rcp / 2)) : 0;
    np = std::max(1, std::min(rp - (int)((long long)nc * rp / rcp), (n_cold + 3) / 4));
}

}  // namespace rtl
