// librt_hip.so — the rt_* C-ABI (include/rt_hip.h) over the HIP kernels in rt_kernels.hpp.
//
// Replaces load_to_gpu / render_frame / load_from_gpu (gpu/include/gpu.cuh:23-26, gpu/src/gpu.cu:98-228)
// and the CPU render_frame (cpu/src/main.c:214-264). All state is per context; every call returns a
// status; HIP errors are captured into rt_last_error() instead of being printed and ignored.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <type_traits>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "rt_hip.h"
#include "rt_host.h"
#include "rt_kernels.hpp"
#include "rt_shpool.hpp"
#include "rt_coop.hpp"
#include "rt_output.hpp"
#include "rt_build.hpp"
#include "rt_comm_logic.hpp"
#include "rt_launch_logic.hpp"
#include "rt_query_logic.hpp"
#include "rt_treelet.hpp"
#include "rt_feedback.hpp"
#include "rt_query.hpp"
#include "rt_shade.hpp"
#include "rt_hits.hpp"
#include "rt_nearest.hpp"
#include "rt_neighbours.hpp"
#include "rt_overlap.hpp"
#include "rt_sweep.hpp"
#include "rt_contacts.hpp"
#include "rt_cut.hpp"
#include "rt_clearance.hpp"
#include "rt_proximity.hpp"
#include "rt_trisweep.hpp"
#include "rt_tricontacts.hpp"
#include "rt_refit.hpp"
#include "rt_collapse.hpp"
#ifndef PRT_TREELET
#define PRT_TREELET 2  // treelet-restructuring passes over the GPU-built binary tree (0: none)
#endif

#include <chrono>
#include <hipcub/hipcub.hpp>

#include <cstdlib>

namespace {

// One BVH view in device memory (rt_device.hpp DBvh) and its host-side build.
struct DevView {
    float4* nodes = nullptr;
    int2* leaves = nullptr;
    float4* tris = nullptr;
    int* orig = nullptr;
    int* path = nullptr;  // [n_tris: original triangle -> its leaf][n_leaves: leaf -> parent record] (ref view)
    int root = 0, n_inner = 0, n_leaves = 0;
    size_t bytes = 0;
};

struct HostView {
    std::vector<float4> nodes, tris;
    std::vector<int2> leaves;
    std::vector<int> orig;
    std::vector<int> path;  // DevView::path
    int root = 0;
};

// The multi-process communicator whose send / recv groups a context's stream holds (rt_ctx::comm_link): shared by both,
// so that a host wait on that stream (rt_sync, rt_download, rt_destroy, ...) first waits, bounded, for the
// communicator's outstanding groups -- a peer that never joins turns into RT_E_TIMEOUT there too, not into a hang --
// and so that either side may be destroyed first (rt_comm_destroy clears cm).
struct CommLink {
    rt_comm* cm = nullptr;
};

// One 8-wide quantised view (rt_wide.cpp; rt_device.hpp DWide) on the host and on the device; nodes empty / null:
// none. tris_n: the triangles it was built over (a subset for the unit and the primary view).
struct HostWide {
    std::vector<float4> nodes, tris;
    std::vector<int> orig;
    int depth = 0, tris_n = 0;
};
struct DevWide {
    float4 *nodes = nullptr, *tris = nullptr;
    int* orig = nullptr;
    int n = 0, depth = 0, tris_n = 0;
    rtd::DWide view() const { return rtd::DWide{nodes, tris, orig, n}; }
};

// What a refit (rt_update_vertices) keeps per topology, made at the first update after the view was built.
// A binary view: its records by tree level (d_list: all records, level l at [off[l], off[l + 1]), root level first).
// A wide view: its levels as ranges of the breadth-first node array (off), and the bitmap of the triangles it holds.
// Both: the scratch array of exact boxes (two float4 per record / node).
struct RefitTopo {
    bool made = false;
    std::vector<int> off;
    int* d_list = nullptr;
    unsigned* d_bits = nullptr;
    float4* d_exact = nullptr;
};

}  // namespace

struct rt_ctx {
    int device = 0;
    unsigned flags = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // device scene
    DevView ref, acc;  // acc.nodes == nullptr: acc aliases ref
    // the 8-wide quantised views: wide, of acc's triangles; unit (rtd::DScene::unit), over the triangles a unit-length
    // ray can hit; prim (rtd::DScene::prim), over those a direction of length <= PRIMARY_D can hit
    DevWide wide, unit, prim;
    float4* d_shade = nullptr;
    float4* d_mats = nullptr;
    float4* d_lights = nullptr;
    int n_lights = 0, n_tris = 0;
    // the packed builds' bounds: 5-byte stack entries hold a 24-bit child base (rtd::WIDE_MAX_NODES wide nodes per
    // view), packed triangle-test jobs a 26-bit triangle (rtd::TQ_MAX_TRIS); larger scenes run the unpacked builds
    bool pk_ok = true, tq_ok = true;
    bool list_ok = true;  // the pool kernels may take their job-list hand-out (off: RT_FLAG_POOL_CURSOR)
    float amb[3] = {0.5f, 0.5f, 0.5f};
    // every face coordinate of the reference tree's child boxes, per axis, sorted, one axis after another
    // (rtd::DScene::faces; n_face below)
    float* d_faces = nullptr;
    bool has_scene = false;
    rt_scene_info info{};  // what the last upload built (rt_get_scene_info)
    float t_ploc = 0.0f, t_treelet = 0.0f, t_collapse = 0.0f;  // the upload's build stages (ms; rt_scene_info)
    // outputs / bookkeeping
    float* d_rgb_own = nullptr;
    size_t rgb_cap = 0;
    float* last_rgb = nullptr;
    unsigned* last_bgra = nullptr;  // the last render's BGRA8 output (rt_outputs.bgra), or a gathered full frame
    int* last_hit = nullptr;
    size_t last_pixels = 0;
    int last_W = 0, last_H = 0, last_off = 0, last_stride = 1, last_rows = 0, last_block = 1;  // the last frame's rows
    int last_shift = 0;
    int last_frames = 1;     // frames of the last render (rt_render_frames)
    bool batch_sum = false;  // set while rt_render_frames launches frames one by one (counters add up)
    // frame batches: the cameras on the device (d_cams, read by the kernels in stream order) and a ring of pinned host
    // slots they are copied from (upload_cams): a slot is rewritten only once its earlier copy has run, so a changed
    // camera set never waits for the renders in flight
    static constexpr int CAM_SLOTS = 8;
    float* d_cams = nullptr;
    hipEvent_t cam_ev[CAM_SLOTS] = {};
    int cam_slot = 0;
    std::vector<float> cams_last;  // the set d_cams holds (after its copy)
    rt_launch_info last_launch{};  // rt_get_launch_info
    float4* d_pathbuf = nullptr;  // PB kernels: per-wave path levels (rtd::KArgs::pathbuf)
    float4* d_lanebuf = nullptr;  // k_persist's multi-sample builds: one slot per resident lane (rtd::KArgs::lanebuf)
    int* d_gstack = nullptr;      // DYN kernels: the binary walks' stacks (rtd::KArgs::gstack)
    float* h_cams = nullptr;  // pinned: CAM_SLOTS x cams_cap cameras
    int cams_cap = 0;
    // output stage (rt_gather, rt_download_bmp)
    float* d_full = nullptr;
    int* d_full_hit = nullptr;
    size_t full_cap = 0, full_hit_cap = 0;
    char* d_stage = nullptr;
    size_t stage_cap = 0;
    unsigned* d_bmp = nullptr;
    size_t bmp_cap = 0;
    unsigned* d_full_bgra = nullptr;  // gathered BGRA8 frames (rt_gather / rt_comm_gather of bgra renders)
    size_t full_bgra_cap = 0;
    unsigned long long* d_counters = nullptr;  // rtd::NCOUNT
    unsigned long long* h_err = nullptr;       // pinned: the last render's error counter (rtd::C_ERR), read by rt_sync / rt_download
    std::unordered_map<long long, int*> orders;  // tile dealing orders (rt_frame.dealing), per tx x ty tile grid
    unsigned int* d_work = nullptr;
    static constexpr int NEV = rtl::NEV;  // ring of per-launch event pairs (rt_kernel_times)
    hipEvent_t ev0s[NEV] = {}, ev1s[NEV] = {};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // the last launch's pair
    // a finished launch's time, read from its pair once and kept (launch_ms): ms_of[slot] is the time of launch
    // ms_launch[slot] - 1 (0: none read yet)
    float ms_of[NEV] = {};
    long long ms_launch[NEV] = {};
    hipEvent_t gather_ev = nullptr;           // completion of the last rt_gather into this (root) context
    hipEvent_t copy_ev = nullptr;             // rt_gather: this (source) context's peer copies issued
    long long launches = 0;
    bool rendered = false;
    std::shared_ptr<CommLink> comm_link;  // the communicator with a send / recv group on this stream (CommLink)
    // the default rule of frame batches and spp > 1 (PERSIST4 or SHPOOL), measured per shape (batch_rule_pick): the
    // trials' launch numbers (rtl::next_trial, rtl::batch_decide) and the choice
    struct BatchRule {
        rtl::ShapeKey key;
        long long launch[2][rtl::BATCH_ROUNDS] = {{-1, -1, -1}, {-1, -1, -1}};
        int choice = -1;
    };
    std::vector<BatchRule> brules;
    long long scene_gen = 0;  // bumped by every upload
    // vertex updates (rt_update_vertices, rt_refit.hpp): what the upload built and how (a view's rebuild repeats it),
    // the per-topology refit data of the five views, the plan pass's words, the face lists' sort buffers
    int built_accel = 0, ploc_radius = 0;
    float collapse_cost = 0.0f;
    int n_face[3] = {0, 0, 0};  // rtd::DScene::n_face (the upload's distinct faces; after an update all 4 per record)
    RefitTopo tp_ref, tp_acc, tp_wide, tp_unit, tp_prim;
    unsigned* d_plan = nullptr;  // [rtr::P_WORDS]
    unsigned* h_plan = nullptr;  // pinned
    double* d_area = nullptr;    // [5]: the full view's decoded child-box area when it was built, and now (then the rebuilds')
    bool area_base = false;      // d_area[0] holds the current build's
    float* d_face_tmp = nullptr; // unsorted faces [3][4 records]
    void* d_sort_tmp = nullptr;
    size_t sort_bytes = 0;
    bool faces_own = false;      // d_faces has room for every record's faces (set by the first update)
    hipEvent_t u_ev0 = nullptr, u_ev1 = nullptr;  // around the last update made
    hipEvent_t u_evs = nullptr;                   // the start of the update under way (u_ev0 once it is made)
    bool updated = false;
    rt_update_info uinfo{};
    // view rebuilds (rt_rebuild_views, rt_collapse.hpp): the binary tree the last device rebuild collapsed per view (test
    // read-back, rt_debug_read_build_tree), the events around the last rebuild and its report. d_area[2], [3]: the full
    // view's area just after the last rebuild and just before it; [4]: the accumulator of the rebuild under way
    struct BuildTree {
        int *left = nullptr, *right = nullptr, *leaf = nullptr;
        int n = 0, root = 0;
    } bt[3];
    hipEvent_t r_ev0 = nullptr, r_ev1 = nullptr;  // around the last rebuild made
    hipEvent_t r_evs = nullptr;                   // the start of the rebuild under way (r_ev0 once it is made)
    bool rebuilt = false;
    rt_rebuild_info rinfo{};
    float4* h_lights = nullptr;  // pinned staging of rt_update_lights, 2 x n_lights (freed with the scene)
    hipEvent_t lights_ev = nullptr;
    float scene_mx = 16.0f;  // the scene's coordinate magnitude, as the boxes' inflation uses it (rt_upload_scene)
    // the queries (rt_trace_rays ... rt_sweep_triangles): one slot per family (rtq::Fam), so that a query touches
    // neither a render's state nor another family's info. counters: the family's [NCOUNT] counters, then its chunk
    // counter (made by the family's first query); ev0, ev1: around its last launch; run: a query was accepted (its info
    // can be read); launched: that query had n > 0, so the events were recorded
    struct QuerySlot {
        unsigned long long* counters = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        bool run = false, launched = false;
    } slots[rtq::NFAM_END];
    // resident workgroups of each query kernel, by its address (query_resident; 0: a k_shade build that does not fit)
    std::unordered_map<const void*, int> residents;
    // original triangle index -> position in the reference tree's records (ensure_ref_inv: made by the first neighbour,
    // contact, proximity or triangle contact query of a scene that asks for points, freed with the scene)
    int* d_ref_inv = nullptr;
    // RT_VARIANT_HYBRID (single 1-spp frames), keyed by the frame's SHAPE: the per-tile times of a measuring k_persist
    // frame, the candidates' tile lists they give (the hot kernel's tiles of the costliest 8x8 tiles; the rest for the
    // cold kernel), the trials and the choice
    struct Hybrid {
        rtl::ShapeKey key;
        int state = 0;  // 0: measure next; 1: a measuring frame's tile times are on their way to h_tr; 2: lists ready
        long long frames = 0;  // frames since the choice or the last list refresh
        static constexpr int NCAND = rtl::NCAND;
        static constexpr int ROUNDS = rtl::HYBRID_ROUNDS;  // trial frames per candidate (rtl::hybrid_decide)
        static constexpr int REFRESH = 64;  // frames of a shape between measuring frames once it is decided
        // candidates (rtl::HotCand: hot threshold, 0 = the cold kernel over the whole frame; lanes per ray of k_coop
        // for the hot tiles; the cold tiles' kernel), their lists at d_lists + cl[c].at, their trials and times
        int nc = 0, choice = -1;
        rtl::HotCand cand[NCAND] = {};
        rtl::CandLists cl[NCAND];
        long long launch[NCAND][ROUNDS] = {};
        float ms[NCAND] = {};
        unsigned long long* d_tr = nullptr;  // [tiles][4], rtd::k_persist's TRACE records
        unsigned long long* h_tr = nullptr;  // pinned
        size_t tr_cap = 0, n_tiles = 0;
        int* d_lists = nullptr;  // per candidate: [hot tiles][cold 8x8 tiles: XCD region layout or order]
        int* h_lists = nullptr;  // pinned staging of d_lists (stream-ordered copies)
        size_t lists_cap = 0, hl_cap = 0;
        bool cold_regions = false;
        int cold_mode = 0;  // the cold lists' region layout (xcd_mode) when cold_regions
        hipEvent_t ev = nullptr, fork = nullptr, join = nullptr;
        hipStream_t s2 = nullptr;
        // per-frame feedback (rt_feedback.hpp): every frame of the shape records its 8x8 tiles' durations in d_cost (and
        // their maximum after them); a decided shape's frames build their lists from the previous frame's on the device
        // (d_fb: [hot: 4 x n_tiles][cold: 9 + n_tiles][counts: 4][the builder's table: FB_G x FB_TK][its partials:
        // 3 FB_G]); h_fb_cnt: a
        // recent frame's hot count, read back without waiting (grid sizes)
        unsigned* d_cost = nullptr;  // two buffers of fb_cap + 1 words: the last frame's (cost_at(cost_cur)), the next
        int cost_cur = 0;            // frame's (cleared by the list builder, k_fb_max: no memset launch per frame)
        unsigned* cost_at(int i) const { return d_cost + (size_t)i * (fb_cap + 1); }
        int* d_fb = nullptr;
        unsigned char* d_info = nullptr;  // rtd::fb_tile_info of every tile, for info_mode
        int info_mode = -1;
        size_t fb_cap = 0;
        bool fb_ok = false;  // d_cost holds a whole frame of this shape (stream order)
        int* h_fb_cnt = nullptr;
        hipEvent_t fb_ev = nullptr;
        bool fb_pending = false;
        int fb_est_c = -1, fb_pend_c = -1;  // the candidates whose hot counts fb_hot_est / the pending copy hold
        float fb_cam[12] = {};  // the last feedback frame's camera (pos, ul, ix, iy)
        bool fb_cam_ok = false;
        int fb_hot_est = -1;
    } hy;
};

namespace {

// Per-frame feedback (rt_feedback.hpp) for a decided shape: its frames deal their tiles by the previous frame's
// per-tile durations, the lists built on the device, instead of a measuring frame's every REFRESH frames
#ifndef PRT_FEEDBACK
#define PRT_FEEDBACK 1
#endif
using rtl::hot_tile;

const char* variant_name(int v) {
    switch (v) {
        case RT_VARIANT_PERSIST: return "persist";
        case RT_VARIANT_PERSIST4: return "persist4";
        case RT_VARIANT_COOP2: return "coop2";
        case RT_VARIANT_COOP4: return "coop4";
        case RT_VARIANT_HYBRID: return "hybrid";
        case RT_VARIANT_SHPOOL: return "shpool";
        case RT_VARIANT_SHDEFER: return "shdefer";
        default: return "default";
    }
}

int fail(rt_ctx* c, hipError_t e, const char* what) {
    if (c) c->err = std::string(what) + ": " + hipGetErrorString(e);
    return RT_E_HIP;
}
#define HIPC(call)                                          \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return fail(ctx, e_, #call); \
    } while (0)

int arg_err(rt_ctx* c, const char* msg) {
    if (c) c->err = msg;
    return RT_E_ARG;
}

void free_view(DevView& v) {
    for (void* p : {(void*)v.nodes, (void*)v.leaves, (void*)v.tris, (void*)v.orig, (void*)v.path})
        if (p) (void)hipFree(p);
    v = DevView();
}

void free_wide(DevWide& w) {
    for (void* p : {(void*)w.nodes, (void*)w.tris, (void*)w.orig})
        if (p) (void)hipFree(p);
    w = DevWide();
}

void free_topo(RefitTopo& t) {
    for (void* p : {(void*)t.d_list, (void*)t.d_bits, (void*)t.d_exact})
        if (p) (void)hipFree(p);
    t = RefitTopo();
}

void free_build_tree(rt_ctx::BuildTree& b) {
    for (void* p : {(void*)b.left, (void*)b.right, (void*)b.leaf})
        if (p) (void)hipFree(p);
    b = rt_ctx::BuildTree();
}

void free_scene(rt_ctx* ctx) {
    for (rt_ctx::BuildTree& b : ctx->bt) free_build_tree(b);
    ctx->rebuilt = false;
    for (RefitTopo* t : {&ctx->tp_ref, &ctx->tp_acc, &ctx->tp_wide, &ctx->tp_unit, &ctx->tp_prim}) free_topo(*t);
    for (void* p : {(void*)ctx->d_face_tmp, ctx->d_sort_tmp})
        if (p) (void)hipFree(p);
    ctx->d_face_tmp = nullptr;
    ctx->d_sort_tmp = nullptr;
    ctx->sort_bytes = 0;
    ctx->faces_own = false;
    ctx->area_base = false;
    ctx->updated = false;
    if (ctx->h_lights) {  // rt_update_lights' staging is sized for this scene's lights (its last copy has run first)
        if (ctx->lights_ev) (void)hipEventSynchronize(ctx->lights_ev);
        (void)hipHostFree(ctx->h_lights);
        ctx->h_lights = nullptr;
    }
    free_view(ctx->ref);
    free_view(ctx->acc);
    if (ctx->d_ref_inv) (void)hipFree(ctx->d_ref_inv);
    ctx->d_ref_inv = nullptr;
    for (DevWide* w : {&ctx->wide, &ctx->unit, &ctx->prim}) free_wide(*w);
    for (void* p : {(void*)ctx->d_shade, (void*)ctx->d_mats, (void*)ctx->d_lights, (void*)ctx->d_faces})
        if (p) (void)hipFree(p);
    ctx->d_faces = nullptr;
    for (int& f : ctx->n_face) f = 0;
    ctx->d_shade = nullptr;
    ctx->d_mats = nullptr;
    ctx->d_lights = nullptr;
    ctx->has_scene = false;
}

template <class T>
int upload(rt_ctx* ctx, T** dst, const std::vector<T>& src, size_t* bytes = nullptr) {
    size_t b = sizeof(T) * (src.empty() ? 1 : src.size());
    HIPC(hipMalloc((void**)dst, b));
    if (!src.empty()) HIPC(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    if (bytes) *bytes += b;
    return RT_OK;
}

// a wide view to the device (none: d stays empty)
int upload_wide(rt_ctx* ctx, const HostWide& h, DevWide& d) {
    if (h.nodes.empty()) return RT_OK;
    int rc;
    if ((rc = upload(ctx, &d.nodes, h.nodes)) || (rc = upload(ctx, &d.tris, h.tris)) ||
        (rc = upload(ctx, &d.orig, h.orig)))
        return rc;
    d.n = (int)(h.nodes.size() / 5);
    d.depth = h.depth;
    d.tris_n = h.tris_n;
    return RT_OK;
}

inline float i2f(int i) {
    float f;
    std::memcpy(&f, &i, 4);
    return f;
}

// leaf-ordered triangle planes: v0, e1, e2, n = e1 x e2 (raytracer.c:36-38, same roundings)
void tri_records(const rt_triangle* T, const int* order, int n, std::vector<float4>& tris, std::vector<int>& orig) {
    tris.resize(3 * (size_t)n);
    orig.resize(n);
    for (int i = 0; i < n; i++) {
        const rt_triangle& t = T[order[i]];
        orig[i] = order[i];
        const rt_vec3 &a = t.coords[0], &b = t.coords[1], &c = t.coords[2];
        const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
        const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        tris[3 * i + 0] = make_float4(a.x, a.y, a.z, e1x);
        tris[3 * i + 1] = make_float4(e1y, e1z, e2x, e2y);
        tris[3 * i + 2] = make_float4(e2z, nx, ny, nz);
    }
}

// Reference-layout BVH (bvh_t[], tri_idx) -> device view. `inflate` > 0 grows every child box by that
// absolute amount (acceleration BVH: keeps the reciprocal-FMA slab test conservative); 0 keeps the
// reference's boxes bit-for-bit (strict walk).
int build_view(rt_ctx* ctx, const rt_bvh_node* B, int nn, const int* tri_idx, const rt_triangle* T, int n,
               float inflate, HostView& v) {
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; i++) {
        int t = tri_idx[i];
        if (t < 0 || t >= n || seen[t]) return arg_err(ctx, "rt_upload_scene: tri_idx is not a permutation");
        seen[t] = 1;
    }
    // refs: interior -> record index (DFS preorder), leaf -> ~leaf id, empty -> EMPTY_REF
    std::vector<int> ref(nn, rtd::EMPTY_REF);
    std::vector<int> inner;
    std::vector<int> st{0};
    std::vector<char> visited(nn, 0);
    while (!st.empty()) {
        int i = st.back();
        st.pop_back();
        if (i < 0 || i >= nn || visited[i]) return arg_err(ctx, "rt_upload_scene: malformed bvh (child index)");
        visited[i] = 1;
        const rt_bvh_node& b = B[i];
        if (b.tr_len > 0) {
            if (b.child < 0 || (long long)b.child + b.tr_len > n)
                return arg_err(ctx, "rt_upload_scene: leaf range outside tri_idx");
            ref[i] = ~(int)v.leaves.size();
            v.leaves.push_back(make_int2(b.child, b.tr_len));
        } else if (b.child != 0) {
            if (b.child < 1 || b.child + 1 >= nn) return arg_err(ctx, "rt_upload_scene: child index out of range");
            ref[i] = (int)inner.size();
            inner.push_back(i);
            st.push_back(b.child + 1);
            st.push_back(b.child);  // left first: preorder, near-first locality
        }
    }
    if (ref[0] == rtd::EMPTY_REF) return arg_err(ctx, "rt_upload_scene: empty root");
    v.root = ref[0];
    v.nodes.resize(4 * inner.size());
    // parents: a record's in its 4th float4's z (-1: the root), a leaf's in path[n + leaf]; path[t]: triangle t's leaf
    std::vector<int> parent(inner.size(), -1);
    v.path.assign((size_t)n + v.leaves.size(), -1);
    for (size_t r = 0; r < inner.size(); r++) {
        const rt_bvh_node& p = B[inner[r]];
        for (int k = 0; k < 2; k++) {
            const int c = ref[p.child + k];
            if (c >= 0) parent[c] = (int)r;
            else if (c != rtd::EMPTY_REF) v.path[(size_t)n + ~c] = (int)r;
        }
    }
    for (size_t l = 0; l < v.leaves.size(); l++)
        for (int i = v.leaves[l].x; i < v.leaves[l].x + v.leaves[l].y; i++) v.path[tri_idx[i]] = (int)l;
    for (size_t r = 0; r < inner.size(); r++) {
        const rt_bvh_node& p = B[inner[r]];
        rt_bvh_node L = B[p.child], R = B[p.child + 1];
        if (inflate > 0)
            for (rt_bvh_node* c : {&L, &R}) {
                c->min.x -= inflate;
                c->min.y -= inflate;
                c->min.z -= inflate;
                c->max.x += inflate;
                c->max.y += inflate;
                c->max.z += inflate;
            }
        v.nodes[4 * r + 0] = make_float4(L.min.x, L.min.y, L.min.z, L.max.x);
        v.nodes[4 * r + 1] = make_float4(L.max.y, L.max.z, R.min.x, R.min.y);
        v.nodes[4 * r + 2] = make_float4(R.min.z, R.max.x, R.max.y, R.max.z);
        v.nodes[4 * r + 3] = make_float4(i2f(ref[p.child]), i2f(ref[p.child + 1]), i2f(parent[r]), 0.0f);
    }
    tri_records(T, tri_idx, n, v.tris, v.orig);
    return RT_OK;
}

int upload_view(rt_ctx* ctx, const HostView& h, DevView& d) {
    int rc;
    d.bytes = 0;
    if ((rc = upload(ctx, &d.nodes, h.nodes, &d.bytes)) || (rc = upload(ctx, &d.leaves, h.leaves, &d.bytes)) ||
        (rc = upload(ctx, &d.tris, h.tris, &d.bytes)) || (rc = upload(ctx, &d.orig, h.orig, &d.bytes)) ||
        (rc = upload(ctx, &d.path, h.path, &d.bytes)))
        return rc;
    d.root = h.root;
    d.n_inner = (int)(h.nodes.size() / 4);
    d.n_leaves = (int)h.leaves.size();
    return RT_OK;
}

}  // namespace

extern "C" int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char* rt_version(void) { return "prt-mi355x 0.2 (gfx950)"; }

extern "C" int rt_create(const rt_opts* opts, rt_ctx** out) {
    if (!out) return RT_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RT_E_NODEVICE;
    rt_ctx* ctx = new rt_ctx();
    if (opts) {
        ctx->device = opts->device;
        ctx->flags = opts->flags;
        ctx->list_ok = !(opts->flags & RT_FLAG_POOL_CURSOR);
        ctx->stream = (hipStream_t)opts->stream;
    }
    if (ctx->device < 0 || ctx->device >= n) {
        delete ctx;
        return RT_E_ARG;
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess && !ctx->stream) {
        e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        ctx->own_stream = true;
    }
    for (int i = 0; i < rt_ctx::NEV && e == hipSuccess; i++) {
        e = hipEventCreate(&ctx->ev0s[i]);
        if (e == hipSuccess) e = hipEventCreate(&ctx->ev1s[i]);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_counters, sizeof(unsigned long long) * rtd::NCOUNT);
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_work, 1024);
    if (e == hipSuccess) e = hipMemset(ctx->d_counters, 0, sizeof(unsigned long long) * rtd::NCOUNT);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->h_err, sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
        rt_destroy(ctx);
        return RT_E_HIP;
    }
    *out = ctx;
    return RT_OK;
}

// load_to_gpu (gpu/src/gpu.cu:129-201): reference layouts -> device layout (rt_device.hpp).
namespace {
// host threads of the acceleration build's CPU stages (the treelet passes, rt_treelet.hpp): the machine's, at most 16
// (the GPU box's CPU quota; nproc there reports the whole host)
int build_threads() {
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(16u, hc));
}
// PLOC's device arrays (rt_build.hpp) for n triangles: what the build proper (ploc_build) works in and leaves -- the
// binary tree in left / right (children of node n + j), every node's box (nlo / nhi) and triangle count (cnt), the
// leaves' triangles (sorted) and the root's id in C[0].
struct PlocDev {
    int n = 0;
    float4 *plo = nullptr, *phi = nullptr, *nlo = nullptr, *nhi = nullptr;
    unsigned *keys = nullptr, *keys2 = nullptr;
    int *vals = nullptr, *sorted = nullptr, *cb = nullptr, *C = nullptr, *C2 = nullptr, *nnb = nullptr, *mflag = nullptr,
        *keep = nullptr, *moff = nullptr, *koff = nullptr, *left = nullptr, *right = nullptr, *cnt = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    int* tot = nullptr;  // pinned: a merge round's merge and survivor totals
    int rounds = 0;
    void release() {
        if (tot) (void)hipHostFree(tot);
        for (void* p : {(void*)plo, (void*)phi, (void*)nlo, (void*)nhi, (void*)keys, (void*)keys2, (void*)vals,
                        (void*)sorted, (void*)cb, (void*)C, (void*)C2, (void*)nnb, (void*)mflag, (void*)keep, (void*)moff,
                        (void*)koff, (void*)left, (void*)right, (void*)cnt, tmp})
            if (p) (void)hipFree(p);
        *this = PlocDev();
    }
};

int ploc_alloc(rt_ctx* ctx, PlocDev& P, int n) {
    P.n = n;
    const size_t nn2 = 2 * (size_t)n;
    HIPC(hipMalloc((void**)&P.plo, sizeof(float4) * n));
    HIPC(hipMalloc((void**)&P.phi, sizeof(float4) * n));
    HIPC(hipMalloc((void**)&P.nlo, sizeof(float4) * nn2));
    HIPC(hipMalloc((void**)&P.nhi, sizeof(float4) * nn2));
    HIPC(hipMalloc((void**)&P.keys, sizeof(unsigned) * n));
    HIPC(hipMalloc((void**)&P.keys2, sizeof(unsigned) * n));
    for (int** p : {&P.vals, &P.sorted, &P.C, &P.C2, &P.nnb, &P.mflag, &P.keep, &P.moff, &P.koff})
        HIPC(hipMalloc((void**)p, sizeof(int) * n));
    HIPC(hipMalloc((void**)&P.left, sizeof(int) * std::max(1, n - 1)));
    HIPC(hipMalloc((void**)&P.right, sizeof(int) * std::max(1, n - 1)));
    HIPC(hipMalloc((void**)&P.cnt, sizeof(int) * nn2));
    HIPC(hipMalloc((void**)&P.cb, sizeof(int) * 8));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, P.keys, P.keys2, P.vals, P.sorted, n, 0, 30, ctx->stream));
    HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, P.mflag, P.moff, n, ctx->stream));
    P.tmp_bytes = std::max(sort_bytes, scan_bytes);
    HIPC(hipMalloc(&P.tmp, P.tmp_bytes));
    HIPC(hipHostMalloc((void**)&P.tot, sizeof(int) * 4, hipHostMallocDefault));
    return RT_OK;
}

// The device build proper over the device vertex array dv (9 floats per triangle), in stream order; waits for the
// stream once per merge round (the round's totals). RT_E_STATE: no progress (never expected).
int ploc_build(rt_ctx* ctx, PlocDev& P, const float* dv, int R) {
    hipStream_t st = ctx->stream;
    const int n = P.n;
    const int cb_init[6] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, (int)0x80000000, (int)0x80000000, (int)0x80000000};
    HIPC(hipMemcpyAsync(P.cb, cb_init, sizeof cb_init, hipMemcpyHostToDevice, st));
    const int g = (n + 255) / 256;
    rtb::k_prim_boxes<<<g, 256, 0, st>>>(dv, n, P.plo, P.phi, P.cb);
    rtb::k_morton<<<g, 256, 0, st>>>(P.plo, P.phi, n, P.cb, P.keys, P.vals);
    HIPC(hipGetLastError());
    size_t sort_bytes = P.tmp_bytes;
    HIPC(hipcub::DeviceRadixSort::SortPairs(P.tmp, sort_bytes, P.keys, P.keys2, P.vals, P.sorted, n, 0, 30, st));
    rtb::k_leaves<<<g, 256, 0, st>>>(P.sorted, P.plo, P.phi, n, P.nlo, P.nhi, P.C, P.cnt);
    HIPC(hipGetLastError());
    int m = n, next = n;
    P.rounds = 0;
    while (m > 1) {
        const int gm = (m + 255) / 256;
        rtb::k_nn<<<gm, 256, 0, st>>>(P.C, m, P.nlo, P.nhi, P.nnb, R);
        rtb::k_flags<<<gm, 256, 0, st>>>(P.nnb, m, P.mflag, P.keep);
        size_t b1 = P.tmp_bytes, b2 = P.tmp_bytes;
        HIPC(hipcub::DeviceScan::ExclusiveSum(P.tmp, b1, P.mflag, P.moff, m, st));
        HIPC(hipcub::DeviceScan::ExclusiveSum(P.tmp, b2, P.keep, P.koff, m, st));
        HIPC(hipMemcpyAsync(P.tot, P.moff + m - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(P.tot + 1, P.mflag + m - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(P.tot + 2, P.koff + m - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(P.tot + 3, P.keep + m - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        rtb::k_merge<<<gm, 256, 0, st>>>(P.C, P.nnb, P.mflag, P.moff, m, n, next, P.nlo, P.nhi, P.left, P.right, P.cnt);
        rtb::k_compact<<<gm, 256, 0, st>>>(P.C, P.keep, P.koff, m, P.C2);
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(st));
        const int merges = P.tot[0] + P.tot[1], survivors = P.tot[2] + P.tot[3];
        if (merges <= 0 || survivors != m - merges) return RT_E_STATE;  // no progress: a mutual pair always exists
        next += merges;
        m = survivors;
        std::swap(P.C, P.C2);
        P.rounds++;
    }
    return RT_OK;
}

// GPU-built acceleration BVH (rt_build.hpp, PLOC) in the reference layout: children of a node at child and
// child + 1, single-triangle leaves numbered depth-first (every subtree's triangles are one range of idx).
// Returns RT_OK, or RT_E_STATE when the tree is unusable (the caller falls back to the host build).
int gpu_ploc(rt_ctx* ctx, const rt_triangle* T, int n, int R, std::vector<rt_bvh_node>& out, std::vector<int>& idx,
             int& depth_out) {
    hipStream_t st = ctx->stream;
    const auto t_gpu = std::chrono::steady_clock::now();
    std::vector<float> hv(9 * (size_t)n);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            hv[9 * (size_t)i + 3 * k] = T[i].coords[k].x;
            hv[9 * (size_t)i + 3 * k + 1] = T[i].coords[k].y;
            hv[9 * (size_t)i + 3 * k + 2] = T[i].coords[k].z;
        }
    const size_t nn2 = 2 * (size_t)n;
    float* dv = nullptr;
    PlocDev P;
    int rc = RT_OK;
    auto done = [&]() {
        if (dv) (void)hipFree(dv);
        P.release();
        return rc;
    };
#define PLOC(call)                                   \
    do {                                             \
        hipError_t e_ = (call);                      \
        if (e_ != hipSuccess) {                      \
            rc = fail(ctx, e_, #call);               \
            return done();                           \
        }                                            \
    } while (0)
    PLOC(hipMalloc((void**)&dv, sizeof(float) * hv.size()));
    if ((rc = ploc_alloc(ctx, P, n))) return done();
    PLOC(hipMemcpyAsync(dv, hv.data(), sizeof(float) * hv.size(), hipMemcpyHostToDevice, st));
    if ((rc = ploc_build(ctx, P, dv, R))) return done();
    const int *C = P.C, *left = P.left, *right = P.right, *sorted = P.sorted;
    const float4 *nlo = P.nlo, *nhi = P.nhi;
    // the tree back to the host
    const int ni = n - 1;
    std::vector<int> hl(std::max(ni, 1)), hr(std::max(ni, 1)), hs(n);
    std::vector<float4> hlo(nn2), hhi(nn2);
    int root = 0;
    PLOC(hipMemcpyAsync(&root, C, sizeof(int), hipMemcpyDeviceToHost, st));
    if (ni > 0) {
        PLOC(hipMemcpyAsync(hl.data(), left, sizeof(int) * ni, hipMemcpyDeviceToHost, st));
        PLOC(hipMemcpyAsync(hr.data(), right, sizeof(int) * ni, hipMemcpyDeviceToHost, st));
    }
    PLOC(hipMemcpyAsync(hs.data(), sorted, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    PLOC(hipMemcpyAsync(hlo.data(), nlo, sizeof(float4) * nn2, hipMemcpyDeviceToHost, st));
    PLOC(hipMemcpyAsync(hhi.data(), nhi, sizeof(float4) * nn2, hipMemcpyDeviceToHost, st));
    PLOC(hipStreamSynchronize(st));
#undef PLOC
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); };
    ctx->t_ploc += since(t_gpu);
    auto t_host = clk::now();
    if (PRT_TREELET > 0 && n >= 3) {  // treelet restructuring on the host (rt_treelet.hpp)
        rtt::Tree T;
        T.n = n;
        T.root = root;
        T.left.assign(hl.begin(), hl.begin() + ni);
        T.right.assign(hr.begin(), hr.begin() + ni);
        T.box.resize(2 * (size_t)n - 1);
        for (size_t i = 0; i < T.box.size(); i++)
            T.box[i] = rtt::Box{{hlo[i].x, hlo[i].y, hlo[i].z}, {hhi[i].x, hhi[i].y, hhi[i].z}};
        for (int p = 0; p < PRT_TREELET; p++) rtt::optimize_pass(T, build_threads());
        std::copy(T.left.begin(), T.left.end(), hl.begin());
        std::copy(T.right.begin(), T.right.end(), hr.begin());
        for (size_t i = (size_t)n; i < T.box.size(); i++) {
            hlo[i] = make_float4(T.box[i].lo[0], T.box[i].lo[1], T.box[i].lo[2], hlo[i].w);
            hhi[i] = make_float4(T.box[i].hi[0], T.box[i].hi[1], T.box[i].hi[2], hhi[i].w);
        }
    }
    ctx->t_treelet += since(t_host);
    t_host = clk::now();
    // reference layout, depth-first: children at consecutive indices, leaves numbered left to right
    out.clear();
    out.reserve(nn2);
    idx.assign(n, 0);
    out.push_back(rt_bvh_node{});
    struct Item {
        int node, at, depth;
    };
    std::vector<Item> stack{{root, 0, 0}};
    int pos = 0, depth = 0;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        depth = std::max(depth, it.depth);
        rt_bvh_node& o = out[it.at];
        const float4 l = hlo[it.node], h = hhi[it.node];
        o.min = rt_vec3{l.x, l.y, l.z};
        o.max = rt_vec3{h.x, h.y, h.z};
        if (it.node < n) {  // leaf: one triangle
            o.tr_len = 1;
            o.child = pos;
            idx[pos++] = hs[it.node];
        } else {
            const int c = (int)out.size();
            out[it.at].tr_len = 0;
            out[it.at].child = c;
            out.push_back(rt_bvh_node{});
            out.push_back(rt_bvh_node{});
            stack.push_back({hr[it.node - n], c + 1, it.depth + 1});  // right after left: depth-first, left first
            stack.push_back({hl[it.node - n], c, it.depth + 1});
        }
    }
    depth_out = depth;
    ctx->t_collapse += since(t_host);
    return done();
}
}  // namespace

namespace {
// Reflection and shadow rays have unit-length directions (raytracer.c:153,166), and hit_triangle culls
// |det| < EPSILON with det = -d . n (raytracer.c:41-45): in float, |det| <= |n| |d| (1 + 7 u) with |d| <= 1 + 3 u,
// so a triangle whose (precomputed, tri_records) |n| is below EPS (1 - 1e-5) can never be hit by such a ray. On the
// BASELINE scenes that is 22 % (dragon stand-in), 23 % (car_boxed), 28 % (two_cars), 81 % (sportscar stand-in) and
// 99.7 % (dragon871k) of the triangles: the wide view built without them serves the unit-direction walks, the
// full one the primary rays (whose directions are not normalised, main.c:229-233).
// Primary rays are not normalised (main.c:229-233): a launch whose primary directions are all at most PRIMARY_D
// long (the reference camera's are 1.87-2.77) walks a view without the triangles no such direction can hit.
constexpr double UNIT_KEEP = 1.0 - 1e-5;  // x EPSILON (1e-3f, raytracer.c:19)
constexpr double PRIMARY_D = 3.0;
// can a direction of length <= dmax hit the triangle (|n| >= EPSILON (1 - 1e-5) / dmax)?
bool hittable(const rt_triangle& t, double dmax) {
    const rt_vec3 &a = t.coords[0], &b = t.coords[1], &c = t.coords[2];  // n as tri_records forms it
    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
    const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    return std::sqrt((double)nx * nx + (double)ny * ny + (double)nz * nz) >= UNIT_KEEP * (double)rtd::EPS / dmax;
}

// Upper bound on |d| of every primary ray of a frame, d = ((ul - pos) + inc_x * fx) + inc_y * fy for
// fx in [0, W], fy in [0, H] (main.c:229-233; spp samples stay inside their pixel): |d| is convex in (fx, fy), so
// its maximum is at a corner; the float evaluation adds at most a few ulp of the terms' magnitudes (1e-5 of them
// here, ~80x that).
double primary_dmax(const rt_camera* c, int W, int H) {
    const double bx = (double)c->ul.x - c->pos.x, by = (double)c->ul.y - c->pos.y, bz = (double)c->ul.z - c->pos.z;
    double m = 0.0;
    for (int cx = 0; cx < 2; cx++)
        for (int cy = 0; cy < 2; cy++) {
            const double x = cx ? W : 0, y = cy ? H : 0;
            const double dx = bx + c->inc_x.x * x + c->inc_y.x * y, dy = by + c->inc_x.y * x + c->inc_y.y * y,
                         dz = bz + c->inc_x.z * x + c->inc_y.z * y;
            m = std::max(m, std::sqrt(dx * dx + dy * dy + dz * dz));
        }
    const double terms = std::sqrt(bx * bx + by * by + bz * bz) +
                         W * std::sqrt((double)c->inc_x.x * c->inc_x.x + (double)c->inc_x.y * c->inc_x.y +
                                       (double)c->inc_x.z * c->inc_x.z) +
                         H * std::sqrt((double)c->inc_y.x * c->inc_y.x + (double)c->inc_y.y * c->inc_y.y +
                                       (double)c->inc_y.z * c->inc_y.z);
    return m * (1.0 + 1e-5) + 1e-5 * terms;
}

// max(16, max |coordinate|) of a scene: the boxes' inflation is 2^-16 of it (rt_upload_scene), the ray queries' origin
// bound 4x it (rt_trace_rays)
float scene_magnitude(const rt_triangle* T, int n) {
    float mx = 16.0f;
    for (int i = 0; i < n; i++)
        for (const rt_vec3& c : T[i].coords)
            mx = std::max(mx, std::max(std::fabs(c.x), std::max(std::fabs(c.y), std::fabs(c.z))));
    return mx;
}

// A binary tree in the reference layout collapsed to the 8-wide quantised form (rt_wide.cpp; boxes inflated, planes
// rounded outward) over its n triangles; false: none (the collapse failed, its product does not pass rth_wbvh_check --
// every triangle in exactly one leaf slot of 1..4, every node but the root with one parent -- or has fewer nodes than
// n triangles need at 32 a node, or is too deep for the wide walk's stack). The check is one pass over the words.
bool collapse_wide(rt_ctx* ctx, const rt_bvh_node* nodes, int nlen, const int* idx, const rt_triangle* T, int n,
                   float inflate, float cnode, HostWide& w) {
    uint32_t* words = nullptr;
    int* order = nullptr;
    rth_wbvh_info wi{};
    const auto t_c = std::chrono::steady_clock::now();
    bool built = rth_wbvh_build_cost(nodes, nlen, idx, T, n, inflate, cnode, &words, &order, &wi) == RT_OK;
    ctx->t_collapse += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_c).count();
    built = built && wi.n_tris == n && (long long)wi.n_nodes * 32 >= n &&
            rth_wbvh_check(words, wi.n_nodes, order, n, 0, nullptr) == RT_OK;
    const bool ok = built && wi.depth <= rtd::WSTACK;
    if (ok) {
        w.nodes.resize(5 * (size_t)wi.n_nodes);
        std::memcpy(w.nodes.data(), words, sizeof(uint32_t) * 20 * (size_t)wi.n_nodes);
        tri_records(T, order, n, w.tris, w.orig);
        w.depth = wi.depth;
        w.tris_n = n;
    }
    rth_free(words);
    rth_free(order);
    return ok;
}

// The 8-wide quantised view of a triangle set, built as the full view was (`method`: RT_ACCEL_GPU = PLOC on the
// device, else the host binned SAH), same inflation and node price. RT_E_STATE: none (too deep for the wide walk).
int wide_view(rt_ctx* ctx, const rt_triangle* T, int n, int method, int R, float inflate, float cnode, HostWide& w) {
    rt_bvh_node* nodes = nullptr;
    int nlen = 0;
    int* idx = nullptr;
    std::vector<rt_bvh_node> gnodes;
    std::vector<int> gidx;
    bool gpu = false;
    if (method == RT_ACCEL_GPU) {
        int gdepth = 0;
        const int rc = gpu_ploc(ctx, T, n, R, gnodes, gidx, gdepth);
        if (rc == RT_E_HIP) return rc;
        gpu = rc == RT_OK;
    }
    if (gpu) {
        nodes = gnodes.data();
        nlen = (int)gnodes.size();
        idx = gidx.data();
    } else if (rth_bvh_build(T, (size_t)n, RTH_BVH_BINNED_SAH, nullptr, &nodes, &nlen, &idx, nullptr) != RT_OK) {
        return RT_E_STATE;
    }
    const int rc = collapse_wide(ctx, nodes, nlen, idx, T, n, inflate, cnode, w) ? RT_OK : RT_E_STATE;
    if (!gpu) {
        rth_free(nodes);
        rth_free(idx);
    }
    return rc;
}

// The wide view over the triangles of the scene a direction of length <= dmax can hit, built as the full view was
// (`built`, `inflate`: the full view's) -- when there are any and fewer than `fewer_than` (else the full view serves).
// v.orig maps to the scene's triangle indices. RT_E_HIP aborts the upload; any other failure leaves v empty.
int subset_view(rt_ctx* ctx, const rt_scene* sc, double dmax, size_t fewer_than, int built, float inflate, HostWide& v) {
    std::vector<rt_triangle> sub;
    std::vector<int> sub_id;
    for (int i = 0; i < sc->n_triangles; i++)
        if (hittable(sc->triangles[i], dmax)) {
            sub.push_back(sc->triangles[i]);
            sub_id.push_back(i);
        }
    if (sub.empty() || sub.size() >= fewer_than) return RT_OK;
    const int R = sc->ploc_radius > 0 ? std::min(sc->ploc_radius, rtb::PLOC_R_MAX) : rtb::PLOC_R;
    const int rc = wide_view(ctx, sub.data(), (int)sub.size(), built, R, inflate, sc->collapse_node_cost, v);
    if (rc == RT_E_HIP) return rc;
    if (rc == RT_OK)
        for (int& o : v.orig) o = sub_id[o];  // subset position -> original triangle index
    else
        v = HostWide();  // no usable view: the full one serves every ray
    return RT_OK;
}
}  // namespace

extern "C" int rt_upload_scene(rt_ctx* ctx, const rt_scene* sc) {
    if (!ctx) return RT_E_ARG;
    if (!sc || !sc->triangles || !sc->bvh || !sc->tri_idx || sc->n_triangles <= 0 || sc->n_nodes <= 0)
        return arg_err(ctx, "rt_upload_scene: empty scene or missing bvh");
    if (sc->n_lights < 0 || (sc->n_lights > 0 && !sc->lights)) return arg_err(ctx, "rt_upload_scene: bad lights");
    if (sc->accel < RT_ACCEL_AUTO || sc->accel > RT_ACCEL_HOST) return arg_err(ctx, "rt_upload_scene: bad accel");
    HIPC(hipSetDevice(ctx->device));
    const int n = sc->n_triangles;
    HostView hr, ha;
    HostWide wide, unit, prim;
    // the boxes' inflation: 2^-16 of the scene's coordinate magnitude (>= 20x the slab tests' rounding reach)
    const float scene_mx = scene_magnitude(sc->triangles, n);
    if (!(scene_mx <= RT_COORD_MAX)) return arg_err(ctx, "rt_upload_scene: a coordinate is beyond RT_COORD_MAX");
    const float inflate = std::ldexp(scene_mx, -16);
    int rc = build_view(ctx, sc->bvh, sc->n_nodes, sc->tri_idx, sc->triangles, n, 0.0f, hr);
    if (rc) return rc;
    // the reference tree's child-box faces per axis, sorted (rtd::DScene::faces), uploaded with the scene below
    std::vector<float> faces[3], all_faces;
    for (size_t r = 0; r + 3 < hr.nodes.size(); r += 4) {  // node record: L.min, L.max, R.min, R.max (build_view)
        const float4 p = hr.nodes[r], q = hr.nodes[r + 1], e = hr.nodes[r + 2];
        const float fx[4] = {p.x, p.w, q.z, e.y}, fy[4] = {p.y, q.x, q.w, e.z}, fz[4] = {p.z, q.y, e.x, e.w};
        for (int k = 0; k < 4; k++) {
            faces[0].push_back(fx[k]);
            faces[1].push_back(fy[k]);
            faces[2].push_back(fz[k]);
        }
    }
    for (int a = 0; a < 3; a++) {
        std::sort(faces[a].begin(), faces[a].end());
        faces[a].erase(std::unique(faces[a].begin(), faces[a].end()), faces[a].end());
        all_faces.insert(all_faces.end(), faces[a].begin(), faces[a].end());
    }
    bool own_acc = sc->accel != RT_ACCEL_REFERENCE;
    int built = sc->accel == RT_ACCEL_REFERENCE ? RT_ACCEL_REFERENCE : RT_ACCEL_HOST;
    float gpu_ms = 0.0f;
    ctx->t_ploc = ctx->t_treelet = ctx->t_collapse = 0.0f;
    const auto t_build = std::chrono::steady_clock::now();
    std::vector<rt_bvh_node> gnodes;
    std::vector<int> gidx;
    // The default (AUTO) is the GPU build: measured same box, 16-frame batches, the PLOC tree collapsed to 8-wide
    // renders faster than the host binned SAH's (dragon 0.847 vs 0.911 ms per frame, dragon871k 0.588 vs 0.640,
    // sportscar 1.370 vs 1.435) and builds in 58 vs 86 ms (dragon; 444 vs 883 ms at 871k triangles)
    if (sc->accel == RT_ACCEL_GPU || sc->accel == RT_ACCEL_AUTO) {  // PLOC on the device; its binary tree is not traversed
        int gdepth = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const int R = sc->ploc_radius > 0 ? std::min(sc->ploc_radius, rtb::PLOC_R_MAX) : rtb::PLOC_R;
        rc = gpu_ploc(ctx, sc->triangles, n, R, gnodes, gidx, gdepth);
        gpu_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc == RT_E_HIP) return rc;
        if (rc == RT_OK) built = RT_ACCEL_GPU;
        rc = RT_OK;
    }
    if (own_acc) {
        // the fast walk's BVH: binned SAH over the same triangles (librt_host.so), boxes inflated; or the GPU-built tree
        rt_bvh_node* nodes = nullptr;
        int nlen = 0;
        int* idx = nullptr;
        if (built == RT_ACCEL_GPU) {
            nodes = (rt_bvh_node*)std::malloc(sizeof(rt_bvh_node) * gnodes.size());
            idx = (int*)std::malloc(sizeof(int) * gidx.size());
            if (!nodes || !idx) {
                std::free(nodes);
                std::free(idx);
                return arg_err(ctx, "rt_upload_scene: out of host memory");
            }
            std::memcpy(nodes, gnodes.data(), sizeof(rt_bvh_node) * gnodes.size());
            std::memcpy(idx, gidx.data(), sizeof(int) * gidx.size());
            nlen = (int)gnodes.size();
        } else if (rth_bvh_build(sc->triangles, (size_t)n, RTH_BVH_BINNED_SAH, nullptr, &nodes, &nlen, &idx, nullptr) != RT_OK) {
            return arg_err(ctx, "rt_upload_scene: acceleration BVH build failed");
        }
        // the binary fast walk's view (used only without a wide view): not for a GPU-built tree, whose depth is
        // not bounded by the binary walks' 34-entry stack (the reference tree serves instead)
        if (built != RT_ACCEL_GPU) rc = build_view(ctx, nodes, nlen, idx, sc->triangles, n, inflate, ha);
        // ... and its 8-wide quantised form (same inflation, planes rounded outward)
        if (!rc) (void)collapse_wide(ctx, nodes, nlen, idx, sc->triangles, n, inflate, sc->collapse_node_cost, wide);
        if (built == RT_ACCEL_GPU) {
            std::free(nodes);
            std::free(idx);
        } else {
            rth_free(nodes);
            rth_free(idx);
        }
        if (rc) return rc;
        if (built == RT_ACCEL_GPU && wide.nodes.empty()) {  // too deep for the wide walk's stack: host build instead
            rt_scene s2 = *sc;
            s2.accel = RT_ACCEL_HOST;
            const int r2 = rt_upload_scene(ctx, &s2);
            if (r2 == RT_OK) ctx->info.gpu_build_ms = gpu_ms;
            return r2;
        }
        own_acc = built != RT_ACCEL_GPU;  // (no binary acceleration view for a GPU-built tree)
    }
    // the unit-direction view (reflection and shadow rays): the same build over the triangles such a ray can hit; the
    // primary view: over those a direction of length <= PRIMARY_D can hit (only when that leaves out at least 2 % of
    // them). Both with the full view's inflation.
    if (!wide.nodes.empty()) {
        if ((rc = subset_view(ctx, sc, 1.0, (size_t)n, built, inflate, unit))) return rc;
        if ((rc = subset_view(ctx, sc, PRIMARY_D, (size_t)n - (size_t)n / 50, built, inflate, prim))) return rc;
    }
    const float build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_build).count();
    // materials: distinct (ks, kd, kr) triples of triangle_t (the reference stores them per triangle)
    std::unordered_map<std::string, int> mat_id;
    std::vector<float4> mats;
    std::vector<float4> shade(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const rt_triangle& t = sc->triangles[i];
        std::string key((const char*)&t.ks, 36);
        auto it = mat_id.find(key);
        int m;
        if (it == mat_id.end()) {
            m = (int)(mats.size() / 3);
            mat_id.emplace(key, m);
            mats.push_back(make_float4(t.ks.x, t.ks.y, t.ks.z, 0.0f));
            mats.push_back(make_float4(t.kd.x, t.kd.y, t.kd.z, 0.0f));
            mats.push_back(make_float4(t.kr.x, t.kr.y, t.kr.z, 0.0f));
        } else {
            m = it->second;
        }
        shade[2 * i + 0] = make_float4(t.norm[0].x, t.norm[0].y, t.norm[0].z, i2f(m));
        shade[2 * i + 1] = make_float4(t.norm[1].x, t.norm[1].y, t.norm[1].z, 0.0f);
    }
    std::vector<float4> lights(2 * (size_t)sc->n_lights);
    for (int j = 0; j < sc->n_lights; j++) {
        const rt_light& l = sc->lights[j];
        lights[2 * j] = make_float4(l.pos.x, l.pos.y, l.pos.z, 0.0f);
        lights[2 * j + 1] = make_float4(l.kl.x, l.kl.y, l.kl.z, 0.0f);
    }
    free_scene(ctx);
    if ((rc = upload_view(ctx, hr, ctx->ref)) || (own_acc && (rc = upload_view(ctx, ha, ctx->acc))) ||
        (rc = upload(ctx, &ctx->d_shade, shade)) || (rc = upload(ctx, &ctx->d_mats, mats)) ||
        (rc = upload(ctx, &ctx->d_lights, lights)) || (rc = upload(ctx, &ctx->d_faces, all_faces)) ||
        (rc = upload_wide(ctx, wide, ctx->wide)) || (rc = upload_wide(ctx, unit, ctx->unit)) ||
        (rc = upload_wide(ctx, prim, ctx->prim))) {
        free_scene(ctx);
        return rc;
    }
    for (int a = 0; a < 3; a++) ctx->n_face[a] = (int)faces[a].size();
    ctx->built_accel = built;
    ctx->ploc_radius = sc->ploc_radius;
    ctx->collapse_cost = sc->collapse_node_cost;
    ctx->n_lights = sc->n_lights;
    ctx->n_tris = n;
    ctx->pk_ok = std::max(ctx->wide.n, std::max(ctx->unit.n, ctx->prim.n)) <= rtd::WIDE_MAX_NODES &&
                 !(ctx->flags & RT_FLAG_UNPACKED_STACK);
    ctx->tq_ok = n < rtd::TQ_MAX_TRIS && !(ctx->flags & RT_FLAG_UNPACKED_TRIS);
    ctx->amb[0] = sc->amb.x;
    ctx->amb[1] = sc->amb.y;
    ctx->amb[2] = sc->amb.z;
    ctx->has_scene = true;
    ctx->scene_gen++;
    ctx->scene_mx = scene_mx;
    ctx->info = rt_scene_info{};
    ctx->info.n_triangles = n;
    ctx->info.n_lights = sc->n_lights;
    ctx->info.wide_nodes = ctx->wide.n;
    ctx->info.wide_depth = ctx->wide.depth;
    ctx->info.unit_triangles = ctx->unit.tris_n;
    ctx->info.unit_nodes = ctx->unit.n;
    ctx->info.unit_depth = ctx->unit.depth;
    ctx->info.primary_triangles = ctx->prim.tris_n;
    ctx->info.primary_nodes = ctx->prim.n;
    ctx->info.accel_built = built;
    ctx->info.build_ms = build_ms;
    ctx->info.gpu_build_ms = gpu_ms;
    ctx->info.ploc_ms = ctx->t_ploc;
    ctx->info.treelet_ms = ctx->t_treelet;
    ctx->info.collapse_ms = ctx->t_collapse;
    return RT_OK;
}

extern "C" int rt_get_scene_info(rt_ctx* ctx, rt_scene_info* info) {
    if (!ctx || !info) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_get_scene_info: no scene uploaded";
        return RT_E_STATE;
    }
    *info = ctx->info;
    return RT_OK;
}

namespace {

// The kernels are built for MAXB = 4 bounce levels (the reference's BOUNCES) and for 8: fn<MAXB>(...) of the build that
// serves a frame's bounces.
#define FOR_MAXB(bounces, fn, ...) ((bounces) <= 4 ? fn<4>(__VA_ARGS__) : fn<8>(__VA_ARGS__))

// resident workgroups per CU of a persistent kernel (occupancy API, capped at 8)
template <class K>
int resident(K kernel, int device, int cap = 8, size_t dyn_lds = 0, int block = rtd::BLOCK) {
    if (cap <= 0) cap = 8;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, dyn_lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    return std::max(1, std::min(per_cu, cap)) * cus;
}

// The persistent kernels run their frame-batch builds for single frames too: with KArgs::cams null a BATCH kernel
// takes its one camera from the kernel arguments (rt_kernels.hpp cam_of), so one instantiation serves both.
using KFn = void (*)(rtd::KArgs);

// the 4-wave k_persist instantiation of a launch: path buffer in LDS (pbl) or global memory, the spp = 1 build,
// counters; SHP: the per-wave shadow pool (rt_shpool.hpp; 1: one pool per level, 2: one for all levels), which needs
// the LDS path buffer
// list (the pool kernels): the pool's job-list hand-out (its LDS sized by pbl_bytes), else the cursor's
template <int MAXB, int SHP>
KFn persist4(bool pbl, bool spp1, bool count, bool list = false) {
    using rtd::k_persist;
    if (pbl) {
        if constexpr (SHP == 1 || SHP == 2) {
            if (!list) {
                if (spp1) return count ? k_persist<MAXB, false, true, true, 4, false, true, 2, true, true, SHP, false>
                                       : k_persist<MAXB, false, false, true, 4, false, true, 2, true, true, SHP, false>;
                return count ? k_persist<MAXB, false, true, true, 4, false, true, 2, true, false, SHP, false>
                             : k_persist<MAXB, false, false, true, 4, false, true, 2, true, false, SHP, false>;
            }
        }
        if (spp1) return count ? k_persist<MAXB, false, true, true, 4, false, true, 2, true, true, SHP>
                               : k_persist<MAXB, false, false, true, 4, false, true, 2, true, true, SHP>;
        return count ? k_persist<MAXB, false, true, true, 4, false, true, 2, true, false, SHP>
                     : k_persist<MAXB, false, false, true, 4, false, true, 2, true, false, SHP>;
    }
    if constexpr (!SHP) {  // (deep trees: the LDS holds no path buffer next to the stack)
        if (spp1) return count ? k_persist<MAXB, false, true, true, 4, false, true, 1, false, true>
                               : k_persist<MAXB, false, false, true, 4, false, true, 1, false, true>;
        return count ? k_persist<MAXB, false, true, true, 4, false, true, 1, false, false>
                     : k_persist<MAXB, false, false, true, 4, false, true, 1, false, false>;
    }
    return nullptr;
}

// the spp > 1 sample-sum slots of an LDS-path-buffer launch (one float4 per lane, after the rest of its layout)
size_t slot_bytes(const rtd::KArgs& A) { return A.spp > 1 ? sizeof(float4) * rtd::BLOCK : 0; }
// the kernel arguments of a launch with `dyn` bytes of dynamic LDS: its slots' offset (ints) when it has them
rtd::KArgs with_slots(const rtd::KArgs& A, size_t dyn) {
    rtd::KArgs B = A;
    B.slot_off = dyn && slot_bytes(A) ? (int)((dyn - slot_bytes(A)) / sizeof(int)) : -1;
    return B;
}

// dynamic LDS of the 4-wave kernels' LDS layout: the wide stack sized to the scene's wide depth, then the path levels
// (and, for the all-levels pool, each level's hit triangle)
// (and, for spp > 1, the lanes' sample-sum slots at the end: rtd::KArgs::slot_off)
// (and, for a pool kernel with the job-list hand-out, the waves' lists after the queues: rt_pool_list.hpp)
template <int MAXB>
size_t pbl_bytes(const rtd::KArgs& A, int shp = 0, bool list = false) {
    const size_t jl = list && (shp == 1 || shp == 2)
                          ? sizeof(int) * (rtd::BLOCK / 64) * (size_t)rtp::list_words(shp == 2 ? MAXB : 1, A.s.n_lights)
                          : 0;
    return sizeof(int) * (size_t)rtd::wstack_words(A.wcap, shp > 0) * rtd::BLOCK + sizeof(float4) * rtd::BLOCK * MAXB +
           (shp == 2 ? sizeof(int) * (rtd::BLOCK * MAXB + rtd::BLOCK / 64 * rtd::TQ_WORDS) : 0) +
           (shp == 1 || shp == 3 ? sizeof(int) * (rtd::BLOCK / 64 * rtd::TQ_WORDS) : 0) + jl + slot_bytes(A);
}
// Does that layout fit 4 workgroups per CU for this scene? (the LDS path buffer measured 1.2 % faster than the global
// slab on dragon, 2.3 % on car_boxed; the shadow pool needs it)
template <int MAXB>
bool pbl_fits(const rtd::KArgs& A, int device, int shp = 0, bool list = false) {
    if (!A.gstack || A.wcap <= 0) return false;
    // asked once per (device, layout size): the query runs between a launch's start event and its kernel, and the
    // list's extra question must not count against the pool in the batch rule's trials (a process-wide memo; contexts
    // may be driven from distinct threads)
    static std::mutex mx;
    static std::map<std::pair<int, size_t>, bool> memo;
    const size_t bytes = pbl_bytes<MAXB>(A, shp, list);
    const std::pair<int, size_t> key(device, bytes);
    {
        std::lock_guard<std::mutex> g(mx);
        const auto it = memo.find(key);
        if (it != memo.end()) return it->second;
    }
    int per_cu = 0;
    const bool fits = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist4<MAXB, 0>(true, true, false),
                                                                   rtd::BLOCK, bytes) == hipSuccess &&
                      per_cu >= 4;
    std::lock_guard<std::mutex> g(mx);
    memo[key] = fits;
    return fits;
}
bool pbl_fits(const rtd::KArgs& A, int device, int shp) { return FOR_MAXB(A.bounces, pbl_fits, A, device, shp); }

// k_tiles (RT_KERNEL_STRICT): one thread per pixel of a 16x16 tile, the reference's walk
template <int MAXB>
KFn tiles_kernel_of(bool count) {
    return count ? rtd::k_tiles<MAXB, true, true> : rtd::k_tiles<MAXB, true, false>;
}
KFn tiles_kernel(int bounces, bool count) { return FOR_MAXB(bounces, tiles_kernel_of, count); }

// k_coop (rt_coop.hpp): G = 2 or 4 lanes per ray; one wave per tile of 64 / G pixels
template <int MAXB>
KFn coop_kernel_of(int G, bool count) {
    using rtd::k_coop;
    if (G == 2) return count ? k_coop<MAXB, true, 2, 3, false, true> : k_coop<MAXB, false, 2, 3, false, true>;
    return count ? k_coop<MAXB, true, 4, 3, false, true> : k_coop<MAXB, false, 4, 3, false, true>;
}
KFn coop_kernel(int bounces, int G, bool count) { return FOR_MAXB(bounces, coop_kernel_of, G, count); }

// k_persist (the persistent one-lane-per-path kernel) in configuration `variant`, and its dynamic LDS:
//   RT_VARIANT_PERSIST   <= 168 VGPRs (3 waves per SIMD), path levels in registers (spp = 1: packed triangle tests);
//   RT_VARIANT_PERSIST4  <= 128 VGPRs (4 waves per SIMD), path levels in a path buffer: in LDS after the wide stack
//                        (packed stack entries and triangle tests, SHP = 3) when 4 workgroups of that fit a CU, else
//                        a global slab;
//   RT_VARIANT_SHPOOL    PERSIST4 with each bounce level's shadow rays walked as a per-wave pool (rt_shpool.hpp);
//                        PERSIST4 where the LDS path buffer does not fit;
//   RT_VARIANT_SHDEFER   PERSIST4 with every level's shadow rays walked as ONE per-wave pool after the closest hits
//                        (the path buffer plus a hit-triangle array in LDS; else PERSIST4);
// a tile trace (A.tile_trace: the hybrid launch's measuring frame, PRT_TILE_TRACE) runs the 3-wave build with
// per-tile timestamps.
template <int MAXB>
KFn persist_kernel_of(const rtd::KArgs& A, int variant, bool count, int device, size_t& dyn, bool pk_ok, bool tq_ok,
                      bool list_ok, unsigned* build) {
    dyn = 0;
    unsigned bd = 0;  // rt_launch_info.build of the instantiation returned (RT_BUILD_*)
    struct Report {
        unsigned* out;
        unsigned& v;
        ~Report() {
            if (out) *out = v;
        }
    } report{build, bd};
    // (the k_persist builds are made either for spp = 1 (SPP1) or for spp > 1 only: each launch takes the one its spp
    // needs; a tile trace -- the hybrid rule's measuring frame, PRT_TILE_TRACE -- is single-sample)
    if (A.tile_trace) {
        bd = RT_BUILD_TRACE;
        return count ? rtd::k_persist<MAXB, false, true, true, 3, true, true, 0, false, true>
                     : rtd::k_persist<MAXB, false, false, true, 3, true, true, 0, false, true>;
    }
    if ((variant == RT_VARIANT_SHPOOL || variant == RT_VARIANT_SHDEFER) && pk_ok && tq_ok) {
        const int shp = variant == RT_VARIANT_SHDEFER ? 2 : 1;
        if (pbl_fits<MAXB>(A, device, shp)) {
            // the job-list hand-out where its lists fit too (dragon, car_boxed, two_cars: 1-4 KB per workgroup), else
            // the cursor's (many lights, MAXB = 8, deep stacks; RT_FLAG_POOL_CURSOR)
            const bool list = list_ok && pbl_fits<MAXB>(A, device, shp, true);
            dyn = pbl_bytes<MAXB>(A, shp, list);
            bd = RT_BUILD_WAVES4 | RT_BUILD_PACKED_STACK | RT_BUILD_PACKED_TRIS | RT_BUILD_LDS_PATHS |
                 (shp == 2 ? RT_BUILD_POOL_ALL : RT_BUILD_POOL_LEVEL) | (list ? RT_BUILD_POOL_LIST : 0u);
            return shp == 2 ? persist4<MAXB, 2>(true, A.spp <= 1, count, list)
                            : persist4<MAXB, 1>(true, A.spp <= 1, count, list);
        }
    }
    // PERSIST4 with packed stack entries and packed triangle tests (SHP = 3) where its LDS fits: sportscar 20-frame
    // batches 0.922 -> 0.895 ms per frame, car_boxed 0.860 -> 0.841; car_boxed 4K at 64 spp 194.3 -> 191.6 ms per
    // frame although that build spills 144 B (same box)
    if ((variant == RT_VARIANT_PERSIST4 || variant == RT_VARIANT_SHPOOL || variant == RT_VARIANT_SHDEFER) && pk_ok &&
        tq_ok && pbl_fits<MAXB>(A, device, 3)) {
        dyn = pbl_bytes<MAXB>(A, 3);
        bd = RT_BUILD_WAVES4 | RT_BUILD_PACKED_STACK | RT_BUILD_PACKED_TRIS | RT_BUILD_LDS_PATHS;
        return persist4<MAXB, 3>(true, A.spp <= 1, count);
    }
    if (variant == RT_VARIANT_PERSIST4 || variant == RT_VARIANT_SHPOOL || variant == RT_VARIANT_SHDEFER) {
        const bool pbl = pbl_fits<MAXB>(A, device);
        if (pbl) dyn = pbl_bytes<MAXB>(A);
        bd = RT_BUILD_WAVES4 | (pbl ? RT_BUILD_LDS_PATHS : 0u);
        // (the bench's batches: the spp = 1 build)
        return persist4<MAXB, 0>(pbl, A.spp <= 1, count);
    }
    // the 3-wave kernel's spp = 1 build with packed triangle tests (queues in static LDS): same box, single frames
    // dragon 1.27 -> 1.16 ms, sportscar 2.40 -> 2.29, car_boxed 1.96 -> 1.84; the default rule's single frames (its
    // cold tiles) sportscar 1.708 -> 1.671, car_boxed 1.210 -> 1.183
    if (A.spp <= 1 && tq_ok) {
        bd = RT_BUILD_PACKED_TRIS;
        return count ? rtd::k_persist<MAXB, false, true, true, 3, false, true, 0, false, true, 3>
                     : rtd::k_persist<MAXB, false, false, true, 3, false, true, 0, false, true, 3>;
    }
    if (A.spp <= 1)  // (scenes past the packed tests' triangle bound)
        return count ? rtd::k_persist<MAXB, false, true, true, 3, false, true, 0, false, true>
                     : rtd::k_persist<MAXB, false, false, true, 3, false, true, 0, false, true>;
    return count ? rtd::k_persist<MAXB, false, true, true, 3, false, true> : rtd::k_persist<MAXB, false, false, true, 3, false, true>;
}

KFn persist_kernel(const rtd::KArgs& A, int variant, bool count, int device, size_t& dyn, bool pk_ok, bool tq_ok,
                   bool list_ok, unsigned* build = nullptr) {
    return FOR_MAXB(A.bounces, persist_kernel_of, A, variant, count, device, dyn, pk_ok, tq_ok, list_ok, build);
}

// `cap`: workgroups per CU at most (0: the occupancy limit); the grid never exceeds the tiles / 4.
void launch_paths(const rtd::KArgs& A, int variant, bool count, int device, hipStream_t s, int cap, bool pk_ok,
                  bool tq_ok, bool list_ok, unsigned* build = nullptr) {
    size_t dyn = 0;
    const KFn k = persist_kernel(A, variant, count, device, dyn, pk_ok, tq_ok, list_ok, build);
    const int blocks = std::max(1, std::min(resident(k, device, cap > 0 ? cap : 8, dyn), (A.n_tiles * A.n_frames + 3) / 4));
    k<<<blocks, rtd::BLOCK, dyn, s>>>(with_slots(A, dyn));
}

rtd::DBvh dview(const DevView& v) { return rtd::DBvh{v.nodes, v.leaves, v.tris, v.orig, v.root}; }

// the uploaded scene as the kernels take it (the renders' KArgs::s, the ray queries' QArgs::s)
rtd::DScene scene_args(const rt_ctx* ctx) {
    rtd::DScene s;
    std::memset(&s, 0, sizeof s);
    s.ref = dview(ctx->ref);
    s.acc = ctx->acc.nodes ? dview(ctx->acc) : s.ref;
    s.wide = ctx->wide.view();
    s.unit = ctx->unit.view();
    s.prim = ctx->prim.view();
    s.shade = ctx->d_shade;
    s.mats = ctx->d_mats;
    s.lights = ctx->d_lights;
    s.n_lights = ctx->n_lights;
    s.amb_x = ctx->amb[0];
    s.amb_y = ctx->amb[1];
    s.amb_z = ctx->amb[2];
    s.faces = ctx->d_faces;  // (rt_kernels.hpp degenerate_ok)
    s.ref_path = ctx->ref.path;  // (rt_kernels.hpp ref_reaches)
    s.n_tris = ctx->n_tris;
    for (int a = 0; a < 3; a++) s.n_face[a] = ctx->n_face[a];
    return s;
}

// k_coop over the whole frame: never more workgroups than tiles / 4
int launch_group(const rtd::KArgs& A, int g, bool count, int device, hipStream_t s, int cap) {
    const KFn k = coop_kernel(A.bounces, g, count);
    const int blocks = std::max(1, std::min(resident(k, device, cap), (A.n_tiles * A.n_frames + 3) / 4));
    k<<<blocks, rtd::BLOCK, 0, s>>>(A);
    return RT_OK;
}

}  // namespace

namespace {
using rtl::centre_out;
using rtl::region_layout;

// A frame batch's cameras to d_cams when they differ from the set it holds. The copy runs in stream order (after the
// renders in flight, which read the old set) from a ring of pinned slots; only a slot whose previous copy has not
// run yet -- CAM_SLOTS camera sets in flight -- makes the host wait.
int upload_cams(rt_ctx* ctx, const rt_camera* cams, int n_frames) {
    static_assert(sizeof(rt_camera) == 48, "rt_camera = 4 x rt_vec3");
    const size_t nf = 12 * (size_t)n_frames;
    if ((int)ctx->cams_last.size() == (int)nf && std::memcmp(ctx->cams_last.data(), cams, sizeof(float) * nf) == 0)
        return RT_OK;
    if (ctx->cams_cap < n_frames) {  // (rare: a larger batch; hipFree waits for the device)
        if (ctx->d_cams) HIPC(hipFree(ctx->d_cams));
        if (ctx->h_cams) {
            HIPC(hipStreamSynchronize(ctx->stream));
            HIPC(hipHostFree(ctx->h_cams));
        }
        ctx->d_cams = nullptr;
        ctx->h_cams = nullptr;
        ctx->cams_cap = 0;
        const int cap = std::max(n_frames, 32);
        HIPC(hipMalloc((void**)&ctx->d_cams, sizeof(float) * 12 * cap));
        HIPC(hipHostMalloc((void**)&ctx->h_cams, sizeof(float) * 12 * cap * rt_ctx::CAM_SLOTS, hipHostMallocDefault));
        ctx->cams_cap = cap;
    }
    const int sl = ctx->cam_slot;
    ctx->cam_slot = (sl + 1) % rt_ctx::CAM_SLOTS;
    if (!ctx->cam_ev[sl]) HIPC(hipEventCreateWithFlags(&ctx->cam_ev[sl], hipEventDisableTiming));
    else HIPC(hipEventSynchronize(ctx->cam_ev[sl]));  // done long ago unless CAM_SLOTS sets are in flight
    float* h = ctx->h_cams + (size_t)sl * 12 * ctx->cams_cap;
    std::memcpy(h, cams, sizeof(float) * nf);
    HIPC(hipMemcpyAsync(ctx->d_cams, h, sizeof(float) * nf, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipEventRecord(ctx->cam_ev[sl], ctx->stream));
    ctx->cams_last.assign(reinterpret_cast<const float*>(cams), reinterpret_cast<const float*>(cams) + nf);
    return RT_OK;
}

// One render call (render_batch): what its steps share
struct Launch {
    const rt_frame* f = nullptr;
    const rt_camera* cams = nullptr;
    int n_frames = 1;
    int kernel = RT_KERNEL_FAST;  // rt_frame.kernel, RT_KERNEL_AUTO resolved
    bool count = false;           // RT_FLAG_COUNTERS: the kernels' counting builds
    rtd::KArgs A;
    // Tile dealing order of the persistent kernels: centre-out (default). The frame ends when the slowest
    // tile does (PRT_TILE_TRACE: 8x8 tiles range from 2 us to ~1.9 ms; expensive ones are deep reflection
    // chains, usually on the object in view); dealing from the centre starts them first (bench frame
    // -7 %). RT_DEAL_ROW_MAJOR: row-major.
    bool centre_out = false;
    int xcd_mode = 0;  // the order's XCD-region layout (rtl::xcd_mode_of), and that layout on the device (null: none)
    const int *region_off = nullptr, *region_order = nullptr;
    rtl::Caps caps;       // what the scene and the frame allow (launch_caps)
    rt_launch_info li{};  // what this render runs (rt_get_launch_info)
};

// the context's own f32 pixels, for a call that names no output (a quantised-only frame writes no f32 pixels at all)
int own_rgb(rt_ctx* ctx, size_t all_px, float*& rgb) {
    if (ctx->rgb_cap < all_px) {
        if (ctx->d_rgb_own) HIPC(hipFree(ctx->d_rgb_own));
        ctx->d_rgb_own = nullptr;
        ctx->rgb_cap = 0;
        HIPC(hipMalloc((void**)&ctx->d_rgb_own, sizeof(float) * 3 * all_px));
        ctx->rgb_cap = all_px;
    }
    rgb = ctx->d_rgb_own;
    return RT_OK;
}

// the kernel arguments of the call's first frame: scene, camera, rows, outputs
void fill_args(const rt_ctx* ctx, Launch& L, const rt_outputs* out, float* rgb, unsigned* bgra, int spp_grid) {
    const rt_frame* f = L.f;
    rtd::KArgs& A = L.A;
    std::memset(&A, 0, sizeof A);
    A.s = scene_args(ctx);
    // the primary view when every primary direction of every frame of the launch is short enough for it
    bool prim_ok = ctx->prim.nodes != nullptr;
    for (int i = 0; i < L.n_frames && prim_ok; i++) prim_ok = primary_dmax(L.cams + i, f->width, f->height) <= PRIMARY_D;
    if (!prim_ok) A.s.prim = rtd::DWide{nullptr, nullptr, nullptr, 0};
    const rt_camera* cam = L.cams;
    const rt_vec3* cv[4] = {&cam->pos, &cam->ul, &cam->inc_x, &cam->inc_y};
    float* dst[4] = {A.pos, A.ul, A.ix, A.iy};
    for (int i = 0; i < 4; i++) {
        dst[i][0] = cv[i]->x;
        dst[i][1] = cv[i]->y;
        dst[i][2] = cv[i]->z;
    }
    A.W = f->width;
    A.H = f->height;
    A.row_offset = f->row_offset;
    A.row_stride = f->row_stride;
    A.row_block = f->row_block > 1 ? f->row_block : 1;
    A.frame_shift = f->frame_shift;
    A.n_rows = f->n_rows;
    A.bounces = f->bounces;
    A.spp = f->spp;
    A.spp_grid = spp_grid;
    A.rgb = rgb;
    A.bgra = bgra;
    A.hit = out ? out->hit : nullptr;
    A.t = out ? out->t : nullptr;
    A.bounce_hit = out ? out->bounce_hit : nullptr;
    A.counters = ctx->d_counters;
    A.work = ctx->d_work;
    A.tiles_x = (f->width + 7) / 8;
    A.n_tiles = A.tiles_x * ((f->n_rows + 7) / 8);
    A.tiles_x8 = A.tiles_x;
}

// the fast kernels' per-wave buffers, allocated on the first fast render
int walk_buffers(rt_ctx* ctx) {
    if (ctx->d_pathbuf && ctx->d_gstack && ctx->d_lanebuf) return RT_OK;
    // (each buffer its own check: a failed allocation of one of them leaves the others, and the next render
    // retries the missing one instead of launching with a null buffer)
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    const size_t waves = (size_t)cus * 8 * (rtd::BLOCK / 64);  // <= 8 workgroups per CU (resident() cap)
    // path buffer of the PB kernels: every resident wave, MAXB <= 8 levels
    if (!ctx->d_pathbuf) HIPC(hipMalloc((void**)&ctx->d_pathbuf, sizeof(float4) * waves * 8 * 64));
    // DYN kernels' binary-walk stacks: STACK ints per lane of every resident workgroup (<= 8 per CU)
    if (!ctx->d_gstack) HIPC(hipMalloc((void**)&ctx->d_gstack, sizeof(int) * (size_t)cus * 8 * rtd::STACK * rtd::BLOCK));
    // the multi-sample builds' per-lane slots (the running sum and the pixel between samples): every resident lane
    if (!ctx->d_lanebuf) HIPC(hipMalloc((void**)&ctx->d_lanebuf, sizeof(float4) * (size_t)cus * 8 * rtd::BLOCK));
    return RT_OK;
}

// A tile list of the context's cache (rt_ctx::orders), made and copied to the device on its first use
template <class Make>
int cached_list(rt_ctx* ctx, long long key, Make make, const int*& list) {
    auto it = ctx->orders.find(key);
    if (it == ctx->orders.end()) {
        const std::vector<int> v = make();
        int* d = nullptr;
        HIPC(hipMalloc((void**)&d, sizeof(int) * v.size()));
        HIPC(hipMemcpy(d, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
        it = ctx->orders.emplace(key, d).first;
    }
    list = it->second;
    return RT_OK;
}
// the dealing order of a tx x ty tile grid on the device: one cached permutation per grid (null: row-major)
int order_for(rt_ctx* ctx, const Launch& L, int tx, int ty, const int*& ord) {
    ord = nullptr;
    if (!L.centre_out) return RT_OK;
    return cached_list(ctx, ((long long)tx << 32) | (unsigned)ty, [&] { return centre_out(tx, ty); }, ord);
}
// the launch's tile order, and its XCD-region layout (device layout: 9 region offsets, then the concatenated regions'
// tiles)
int tile_orders(rt_ctx* ctx, Launch& L) {
    const rt_frame* f = L.f;
    const int tx = L.A.tiles_x, ty = L.A.n_tiles / L.A.tiles_x;
    L.centre_out = L.kernel == RT_KERNEL_FAST && f->dealing != RT_DEAL_ROW_MAJOR;
    if (int rc = order_for(ctx, L, tx, ty, L.A.tile_order)) return rc;
    L.xcd_mode = rtl::xcd_mode_of(f->dealing, L.n_frames, f->row_offset == 0 && f->n_rows == f->height);
    if (!(L.centre_out && L.xcd_mode >= 1 && L.xcd_mode <= 3)) return RT_OK;
    const long long key = ((long long)L.xcd_mode << 58) | ((long long)tx << 32) | (unsigned)ty;
    if (int rc = cached_list(ctx, key, [&] { return region_layout(centre_out(tx, ty), tx, ty, L.xcd_mode); }, L.region_off))
        return rc;
    L.region_order = L.region_off + 9;
    return RT_OK;
}

// RT_KERNEL_FAST launch configurations (rt_frame.variant; every one renders the same bits):
//   PERSIST / PERSIST4  k_persist, one lane per pixel path, walks in lockstep, 8x8 tiles;
//   SHPOOL              k_persist at 4 waves with each level's shadow rays walked as a per-wave pool;
//   COOP2/4             k_coop (rt_coop.hpp): G lanes per ray, 64/G-pixel tiles — shorter chains per tile,
//                       which is what a frame split over many GPUs (few tiles per wave) is bound by;
//   HYBRID              single frames: the costliest tiles through k_coop on a second stream (§3e).
// What this launch's scene and frame allow of them (rtl::resolve_variant)
rtl::Caps launch_caps(const rt_ctx* ctx, const Launch& L) {
    rtl::Caps c;
    c.wide = L.kernel == RT_KERNEL_FAST && ctx->wide.n > 0;
    // the shadow pool: 1..32 lights (a 32-bit visibility word per pixel) and the LDS path buffer at 4 workgroups per CU
    c.shp_ok = c.wide && ctx->n_lights >= 1 && ctx->n_lights <= 32 && ctx->pk_ok && ctx->tq_ok &&
               pbl_fits(L.A, ctx->device, 1);
    c.shd_ok = c.shp_ok && ctx->n_lights <= 8 && pbl_fits(L.A, ctx->device, 2);
    c.tile_trace = L.A.tile_trace != nullptr;
    c.n_lights = ctx->n_lights;
    c.n_frames = L.n_frames;
    c.frame_shift = L.f->frame_shift;
    c.spp = L.f->spp;
    return c;
}

bool tune_log() {
    const char* l = std::getenv("PRT_TUNE_LOG");
    return l && std::atoi(l) == 1;
}

// The default rule for frame batches and spp > 1 where the shadow pool can run: measured, not guessed. Whether the
// pool pays depends on the scene (dragon 20-frame batches 0.708 -> 0.666 ms per frame; two_cars 4K 1.881 vs 1.917,
// car_boxed 0.868 vs 0.902), so the first launches of a shape try PERSIST4 and SHPOOL ROUNDS times each (their own
// HIP events, read by a query once the last has run) and the faster per frame renders from then on. A context with
// traversal counters never tries (the counters of a trial would be another kernel's): it keeps the static rule.
int batch_rule_pick(rt_ctx* ctx, Launch& L, int& mode) {
    const rt_frame* f = L.f;
    const rtl::ShapeKey key = rtl::batch_key(ctx->scene_gen, *f, L.n_frames);
    rt_ctx::BatchRule* br = nullptr;
    for (auto& b : ctx->brules)
        if (b.key == key) br = &b;
    if (!br) {
        if (ctx->brules.size() >= 16) ctx->brules.erase(ctx->brules.begin());
        ctx->brules.emplace_back();
        br = &ctx->brules.back();
        br->key = key;
    }
    rt_ctx::BatchRule& b = *br;
    constexpr int nc = 2, R = rtl::BATCH_ROUNDS;
    const int cand[nc] = {RT_VARIANT_PERSIST4, rtl::pool_v(L.caps)};
    int pick = -1;
    if (b.choice < 0) {
        pick = rtl::next_trial(&b.launch[0][0], nc, R, true, ctx->launches);
        if (pick < 0) {  // every trial enqueued: decide once the last has run (a query, never a wait)
            const long long last = rtl::latest_trial(&b.launch[0][0], nc, R);
            const hipError_t q = hipEventQuery(ctx->ev1s[last % rt_ctx::NEV]);
            if (q == hipSuccess) {
                float t[nc * R], ms[nc];
                for (int c = 0; c < nc; c++)
                    for (int r = 0; r < R; r++) {
                        const int sl = (int)(b.launch[c][r] % rt_ctx::NEV);
                        HIPC(hipEventElapsedTime(&t[c * R + r], ctx->ev0s[sl], ctx->ev1s[sl]));
                    }
                b.choice = rtl::batch_decide(t, nc, ms);
                if (tune_log())
                    std::fprintf(stderr, "[prt batch] %dx%d f%d spp%d: persist4 %.3f ms, %s %.3f ms -> %s\n",
                                 f->width, f->n_rows, L.n_frames, f->spp, ms[0], variant_name(cand[1]), ms[1],
                                 variant_name(cand[b.choice]));
            } else if (q != hipErrorNotReady) {
                return fail(ctx, q, "rt_render: batch rule trials");
            } else {
                (void)hipGetLastError();  // not an error: the trials are still running
            }
        }
    }
    if (b.choice >= 0) {
        mode = cand[b.choice];
    } else {
        mode = pick >= 0 ? cand[pick] : rtl::batch_default(L.caps);
        L.li.trial = 1;
        L.li.settled = 0;
    }
    return RT_OK;
}

// RT_VARIANT_HYBRID: what this single frame runs. The state is keyed by the frame's SHAPE, not its camera (a
// walkthrough moves it every frame). The first frame of a shape measures: k_persist with per-tile times, copied to
// pinned host memory behind it. Once they have arrived (an event query, never a wait) the tile lists of every
// candidate are built and copied in stream order, and the next frames try the candidates ROUNDS times each,
// timed by their own HIP events; when the last trial has finished (a query) the fastest median renders from then
// on (PRT_TUNE_LOG=1 prints them). Every REFRESH frames of the shape a measuring frame renews the tile lists for
// a moving camera (the choice stays). While a measurement or the trials are in flight, a frame runs the static
// rule's whole-frame kernel. rt_frame.hot_pct > 0 fixes the threshold (no trials).
// kind 0: measuring frame; 1: whole-frame variant c; 2: hybrid candidate c's launch (lists at ctx->hy)
struct Pick {
    int kind, c;
};

// has the work before event e run? A query, never a wait
hipError_t in_flight(hipEvent_t e, bool& done) {
    const hipError_t q = hipEventQuery(e);
    done = q == hipSuccess;
    if (q == hipErrorNotReady) {
        (void)hipGetLastError();  // not an error: still running
        return hipSuccess;
    }
    return q;
}

// A new shape (no measurement in flight writes h_tr, no frame of the old shape runs now): its key, buffers for its
// tiles, and every piece of the old shape's state reset -- it is measured next
int hybrid_new_shape(rt_ctx* ctx, const rtl::ShapeKey& key, size_t n_tiles) {
    rt_ctx::Hybrid& h = ctx->hy;
    h.key = key;
    h.choice = -1;
    h.n_tiles = n_tiles;
    if (h.tr_cap < h.n_tiles) {
        if (h.d_tr) (void)hipFree(h.d_tr);
        if (h.h_tr) (void)hipHostFree(h.h_tr);
        h.d_tr = h.h_tr = nullptr;
        h.tr_cap = 0;
        hipError_t e = hipMalloc((void**)&h.d_tr, sizeof(unsigned long long) * 4 * h.n_tiles);
        if (e == hipSuccess) e = hipHostMalloc((void**)&h.h_tr, sizeof(unsigned long long) * 4 * h.n_tiles,
                                               hipHostMallocDefault);
        if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid tile times");
        h.tr_cap = h.n_tiles;
    }
    if (h.fb_cap < h.n_tiles) {  // the feedback's buffers (rt_feedback.hpp)
        if (h.fb_pending) (void)hipEventSynchronize(h.fb_ev);
        if (h.d_cost) (void)hipFree(h.d_cost);
        if (h.d_fb) (void)hipFree(h.d_fb);
        if (h.d_info) (void)hipFree(h.d_info);
        h.d_cost = nullptr;
        h.d_fb = nullptr;
        h.d_info = nullptr;
        h.fb_cap = 0;
        hipError_t e = hipMalloc((void**)&h.d_cost, sizeof(unsigned) * 2 * (h.n_tiles + 1));
        if (e == hipSuccess) e = hipMalloc((void**)&h.d_fb, sizeof(int) * (5 * h.n_tiles + 13 + rtd::FB_G * (rtd::FB_TK + 3)));
        if (e == hipSuccess) e = hipMalloc((void**)&h.d_info, h.n_tiles);
        if (e == hipSuccess && !h.h_fb_cnt) e = hipHostMalloc((void**)&h.h_fb_cnt, sizeof(int) * 4, hipHostMallocDefault);
        if (e == hipSuccess && !h.fb_ev) e = hipEventCreateWithFlags(&h.fb_ev, hipEventDisableTiming);
        if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid feedback buffers");
        h.fb_cap = h.n_tiles;
    }
    h.fb_ok = false;
    h.fb_cam_ok = false;
    h.fb_hot_est = -1;
    h.info_mode = -1;
    h.state = 0;
    return RT_OK;
}

// The measurement has landed in h_tr: the candidates (a refresh of a decided shape keeps them and the choice) and the
// tile lists of every one of them, [hot tiles][cold 8x8 tiles] one after another (rtl::build_lists), staged to the device
int hybrid_stage_lists(rt_ctx* ctx, const Launch& L) {
    rt_ctx::Hybrid& h = ctx->hy;
    const rt_frame* f = L.f;
    const int tx = L.A.tiles_x, ty = L.A.n_tiles / L.A.tiles_x;
    std::vector<long long> dur(h.n_tiles);
    for (size_t t = 0; t < h.n_tiles; t++) dur[t] = (long long)(h.h_tr[4 * t + 1] - h.h_tr[4 * t]);
    std::vector<int> ord = centre_out(tx, ty);
    if (!L.centre_out)
        for (int t = 0; t < (int)ord.size(); t++) ord[t] = t;  // RT_DEAL_ROW_MAJOR
    h.cold_regions = L.xcd_mode >= 1 && L.xcd_mode <= 3 && L.centre_out;
    h.cold_mode = h.cold_regions ? L.xcd_mode : 0;
    const bool keep = h.choice >= 0;  // a refresh: new lists, the same candidates and choice
    if (!keep) h.nc = rtl::hybrid_candidates(L.caps, f->hot_pct, f->hot_kernel, h.cand);
    const std::vector<int> lists =
        rtl::build_lists(dur, tx, ty, f->width, f->n_rows, ord, h.cold_mode, h.cand, h.nc, h.cl);
    if (!lists.empty()) {
        // pinned staging: the last copy out of it ran before the measuring frame (stream order), which has
        // finished; the device copy is stream-ordered after every frame that read the old lists
        if (h.hl_cap < lists.size()) {
            if (h.h_lists) (void)hipHostFree(h.h_lists);
            h.h_lists = nullptr;
            h.hl_cap = 0;
            const hipError_t e = hipHostMalloc((void**)&h.h_lists, sizeof(int) * lists.size(), hipHostMallocDefault);
            if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid lists");
            h.hl_cap = lists.size();
        }
        if (h.lists_cap < lists.size()) {  // (rare: a new shape; hipFree waits for the device)
            if (h.d_lists) (void)hipFree(h.d_lists);
            h.d_lists = nullptr;
            h.lists_cap = 0;
            const hipError_t e = hipMalloc((void**)&h.d_lists, sizeof(int) * lists.size());
            if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid lists");
            h.lists_cap = lists.size();
        }
        std::memcpy(h.h_lists, lists.data(), sizeof(int) * lists.size());
        const hipError_t e = hipMemcpyAsync(h.d_lists, h.h_lists, sizeof(int) * lists.size(), hipMemcpyHostToDevice,
                                            ctx->stream);
        if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid lists");
    }
    if (!keep) {
        for (int c = 0; c < h.nc; c++)
            for (int r = 0; r < rt_ctx::Hybrid::ROUNDS; r++) h.launch[c][r] = -1;
        h.choice = h.nc == 1 ? 0 : -1;
    }
    h.frames = 0;
    h.state = 2;
    return RT_OK;
}

// The lists are ready: the chosen candidate; else the next trial; else, once the last trial has run, the choice
int hybrid_choose(rt_ctx* ctx, Launch& L, Pick& pk) {
    rt_ctx::Hybrid& h = ctx->hy;
    constexpr int R = rt_ctx::Hybrid::ROUNDS;
    auto pick_of = [&](int c) { return h.cand[c].pct == 0 && !h.cand[c].lpt ? Pick{1, h.cand[c].cold} : Pick{2, c}; };
    if (h.choice < 0) {
        if (const int c = rtl::next_trial(&h.launch[0][0], h.nc, R, false, ctx->launches); c >= 0) {
            pk = pick_of(c);
            return RT_OK;
        }
        const long long last = rtl::latest_trial(&h.launch[0][0], h.nc, R);
        bool done = false;
        if (hipError_t e = in_flight(ctx->ev1s[last % rt_ctx::NEV], done); e != hipSuccess)
            return fail(ctx, e, "rt_render: hybrid trials");
        if (!done) return RT_OK;  // the trials are still running: the static rule's kernel
        float t[rt_ctx::Hybrid::NCAND * R] = {};
        for (int c = 0; c < h.nc; c++)
            for (int r = rtl::HYBRID_WARM; r < R; r++) {
                const int sl = (int)(h.launch[c][r] % rt_ctx::NEV);
                const hipError_t e = hipEventElapsedTime(&t[c * R + r], ctx->ev0s[sl], ctx->ev1s[sl]);
                if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid trials");
            }
        h.choice = rtl::hybrid_decide(t, h.nc, h.ms);
        h.frames = 0;
        if (tune_log()) {
            std::fprintf(stderr, "[prt hybrid] %dx%d b%d:", L.f->width, L.f->n_rows, L.f->bounces);
            for (int c = 0; c < h.nc; c++)
                std::fprintf(stderr, " %s%d/coop%d/%s%s %.3f ms", h.cand[c].pct ? "hot>" : "whole", h.cand[c].pct,
                             h.cand[c].lanes, variant_name(h.cand[c].cold), h.cand[c].lpt ? "/lpt" : "", h.ms[c]);
            std::fprintf(stderr, " -> %d\n", h.choice);
        }
    }
    L.li.settled = 1;
    L.li.trial = 0;
    pk = pick_of(h.choice);
    return RT_OK;
}

// pk: what this frame of RT_VARIANT_HYBRID runs (the static rule's whole-frame kernel unless the state says otherwise)
int hybrid_pick(rt_ctx* ctx, Launch& L, Pick& pk) {
    rt_ctx::Hybrid& h = ctx->hy;
    const rtl::ShapeKey key = rtl::hybrid_key(ctx->scene_gen, *L.f);
    const bool same = h.key == key;
    pk = Pick{1, rtl::single_rule(L.caps)};
    if (!h.ev) {
        hipError_t e = hipEventCreateWithFlags(&h.ev, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h.fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h.join, hipEventDisableTiming);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&h.s2, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(ctx, e, "rt_render: hybrid events / stream");
    }
    // a decided shape's frames -- its periodic refresh (a measuring frame, li.refresh) and the frames while that
    // measurement is in flight included -- are the rule's steady state (settled); a new shape's are trials
    const bool decided = same && h.choice >= 0;
    L.li.settled = decided ? 1 : 0;
    L.li.trial = decided ? 0 : 1;
    if (!same) {  // a new shape: measure it, once an earlier measurement in flight has landed in h_tr
        if (h.state == 1) {
            bool done = false;
            if (hipError_t e = in_flight(h.ev, done); e != hipSuccess) return fail(ctx, e, "rt_render: hybrid measurement");
            if (!done) return RT_OK;
        }
        if (int rc = hybrid_new_shape(ctx, key, (size_t)L.A.n_tiles)) return rc;
    }
    // renew a decided shape's lists with a measuring frame every REFRESH frames -- unless its frames feed their own
    // tile times forward (PRT_FEEDBACK), which keeps the lists one frame old
    if (!PRT_FEEDBACK && h.state == 2 && h.choice >= 0 && ++h.frames >= rt_ctx::Hybrid::REFRESH) h.state = 0;
    if (h.state == 0) {
        pk = Pick{0, 0};
        return RT_OK;
    }
    if (h.state == 1) {
        bool done = false;
        if (hipError_t e = in_flight(h.ev, done); e != hipSuccess) return fail(ctx, e, "rt_render: hybrid measurement");
        if (!done) {
            if (h.choice >= 0 && h.cand[h.choice].pct == 0) pk.c = h.cand[h.choice].cold;
            return RT_OK;
        }
        if (int rc = hybrid_stage_lists(ctx, L)) return rc;
    }
    return hybrid_choose(ctx, L, pk);
}

// The hot kernel's arguments of a hybrid launch: its own tiles (tiles_x wide, n_tiles of them in `order`, hottest
// first), dealt from their own work counter
rtd::KArgs hot_args(const rtd::KArgs& A, int tiles_x, int n_tiles, const int* order) {
    rtd::KArgs B = A;
    B.tiles_x = tiles_x;
    B.n_tiles = n_tiles;
    B.tile_order = order;
    B.region_off = nullptr;
    B.work = A.work + 224;
    return B;
}

// One persistent grid of a hybrid launch
struct Grid {
    KFn k;
    int blocks;  // 0: not launched
    size_t dyn;
    rtd::KArgs args;
};
// The two grids of a hybrid launch: the hot kernel on the context's second stream while the cold kernel runs on the
// context stream, which waits for both; without a hot grid the cold kernel alone.
int launch_hot_cold(rt_ctx* ctx, const Grid& hot, const Grid& cold) {
    rt_ctx::Hybrid& h = ctx->hy;
    auto run = [](const Grid& g, hipStream_t s) {
        if (g.blocks > 0) g.k<<<g.blocks, rtd::BLOCK, g.dyn, s>>>(g.args);
    };
    if (hot.blocks == 0) {
        run(cold, ctx->stream);
        HIPC(hipGetLastError());
        return RT_OK;
    }
    HIPC(hipEventRecord(h.fork, ctx->stream));  // after the lists, the work / counter and the durations' resets
    HIPC(hipStreamWaitEvent(h.s2, h.fork, 0));
    run(hot, h.s2);
    HIPC(hipGetLastError());
    run(cold, ctx->stream);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(h.join, h.s2));
    HIPC(hipStreamWaitEvent(ctx->stream, h.join, 0));
    return RT_OK;
}

// RT_VARIANT_HYBRID, one frame: the hot tiles (ctx->hy lists) through k_coop on the context's second stream
// while the cold kernel (k_persist, or the shadow pool) renders the cold 8x8 tiles on the context stream; both
// persistent grids together fill the chip (rtl::hybrid_grids).
int launch_hybrid(rt_ctx* ctx, const rtd::KArgs& A, bool count, int c, unsigned* build) {
    rt_ctx::Hybrid& h = ctx->hy;
    const int n_hot = h.cl[c].n_hot, n_cold = h.cl[c].n_cold;
    int* lists = h.d_lists + h.cl[c].at;
    const int g = h.cand[c].lanes;
    const KFn kc = coop_kernel(A.bounces, g, count);
    int tw, th;
    hot_tile(g, tw, th);
    const rtd::KArgs B = hot_args(A, (A.W + tw - 1) / tw, n_hot, lists);
    rtd::KArgs P = A;
    P.n_tiles = n_cold;
    P.region_off = h.cold_regions ? lists + n_hot : nullptr;
    P.tile_order = lists + n_hot + (h.cold_regions ? 9 : 0);
    size_t dyn = 0;
    const KFn kp = persist_kernel(P, h.cand[c].cold, count, ctx->device, dyn, ctx->pk_ok, ctx->tq_ok, ctx->list_ok, build);
    const int rp = resident(kp, ctx->device, 8, dyn);
    const int rcp = resident(kc, ctx->device);
    int nc, np;
    rtl::hybrid_grids(rp, rcp, n_hot, n_cold, nc, np);
    // (no hot tiles: a whole frame in the measured order)
    return launch_hot_cold(ctx, Grid{kc, nc, 0, B}, Grid{kp, n_cold > 0 ? np : 0, dyn, with_slots(P, dyn)});
}

// A decided shape's frame under the per-frame feedback (rt_feedback.hpp): candidate c's lists built on the device from
// the previous frame's tile durations (k_fb_max, k_fb_count, k_fb_place), the durations cleared, then c's kernels as launch_hybrid launches
// them, every one reading its list and count from the device and recording this frame's durations. The grids are sized
// by a recent frame's hot count, read back without a wait.
int launch_hybrid_fb(rt_ctx* ctx, const rtd::KArgs& A, bool count, int c, unsigned* build) {
    rt_ctx::Hybrid& h = ctx->hy;
    const int g = h.cand[c].lanes == 2 ? 2 : 4;
    const bool hot = h.cand[c].pct > 0;
    int tw, th;
    hot_tile(g, tw, th);
    const int ctw = (A.W + tw - 1) / tw, cth = (A.n_rows + th - 1) / th;
    int* d_hot = h.d_fb;
    int* d_cold = h.d_fb + 4 * h.n_tiles;
    int* d_cnt = d_cold + 9 + h.n_tiles;
    const int tx = A.tiles_x, ty = A.n_tiles / A.tiles_x;
    if (h.info_mode != h.cold_mode) {  // the shape's per-tile region and hot-kernel tile counts, once
        std::vector<unsigned char> info(h.n_tiles);
        for (int t = 0; t < A.n_tiles; t++) info[t] = rtd::fb_tile_info(t, tx, ty, h.cold_mode, A.W, A.n_rows);
        HIPC(hipMemcpy(h.d_info, info.data(), info.size(), hipMemcpyHostToDevice));
        h.info_mode = h.cold_mode;
    }
    // (hot set: at most half the 8x8 tiles, as the host's lists, counted in hot-kernel tiles)
    // (d_cost holds n_tiles + 1 words: A.n_tiles is this shape's n_tiles, the maximum's word right after the tiles)
    // the last frame's times in, this frame's buffer cleared by k_fb_max (with the frame's counters and work words)
    unsigned* const cost_in = h.cost_at(h.cost_cur);
    unsigned* const cost_out = h.cost_at(h.cost_cur ^ 1);
    rtd::FbArgs F{cost_in, A.n_tiles, tx, ty, h.cand[c].pct, (int)(h.n_tiles / 2) * (8 / tw) * (8 / th), tw, th, ctw, cth, h.cold_mode,
                  h.d_info, d_hot, d_cold, d_cnt, (unsigned*)(d_cnt + 4), (unsigned*)(d_cnt + 4) + rtd::FB_G * rtd::FB_TK, 0,
                  cost_out,
                  ctx->batch_sum ? nullptr : ctx->d_counters, rtd::NCOUNT, ctx->d_work, 1024 / 4};
    {  // the camera against the last feedback frame's (rt_feedback.hpp FbArgs::moved)
        float cam[12];
        std::memcpy(cam, A.pos, sizeof(float) * 3);
        std::memcpy(cam + 3, A.ul, sizeof(float) * 3);
        std::memcpy(cam + 6, A.ix, sizeof(float) * 3);
        std::memcpy(cam + 9, A.iy, sizeof(float) * 3);
        F.moved = h.fb_cam_ok && std::memcmp(cam, h.fb_cam, sizeof cam) != 0;
        std::memcpy(h.fb_cam, cam, sizeof cam);
        h.fb_cam_ok = true;
    }
    rtd::k_fb_max<<<rtd::FB_G, rtd::FB_THREADS, 0, ctx->stream>>>(F);
    rtd::k_fb_count<<<rtd::FB_G, rtd::FB_THREADS, 0, ctx->stream>>>(F);
    rtd::k_fb_place<<<rtd::FB_G, rtd::FB_THREADS, 0, ctx->stream>>>(F);
    HIPC(hipGetLastError());
    h.cost_cur ^= 1;
    if (h.fb_pending) {  // a recent frame's hot count (grid size), if its copy has landed: a query, never a wait
        const hipError_t q = hipEventQuery(h.fb_ev);
        if (q == hipSuccess) {
            h.fb_hot_est = h.h_fb_cnt[0];
            h.fb_est_c = h.fb_pend_c;
            h.fb_pending = false;
        } else if (q == hipErrorNotReady) {
            (void)hipGetLastError();
        } else {
            return fail(ctx, q, "rt_render: hybrid feedback count");
        }
    }
    if (hot && !h.fb_pending) {
        HIPC(hipMemcpyAsync(h.h_fb_cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPC(hipEventRecord(h.fb_ev, ctx->stream));
        h.fb_pending = true;
        h.fb_pend_c = c;
    }
    const KFn kc = coop_kernel(A.bounces, g, count);
    // the hot kernel's tiles, hottest first, their number on the device
    rtd::KArgs B = hot_args(A, ctw, 4 * (int)h.n_tiles, d_hot);
    B.n_tiles_dev = d_cnt;
    B.tile_cost = cost_out;
    rtd::KArgs P = A;  // the cold 8x8 tiles by region, costliest first (the region offsets hold their number)
    P.region_off = d_cold;
    P.tile_order = d_cold + 9;
    P.tile_cost = cost_out;
    size_t dyn = 0;
    const KFn kp = persist_kernel(P, h.cand[c].cold, count, ctx->device, dyn, ctx->pk_ok, ctx->tq_ok, ctx->list_ok, build);
    if (build) *build |= RT_BUILD_FEEDBACK;
    const int rp = resident(kp, ctx->device, 8, dyn);
    const int rcp = resident(kc, ctx->device);
    const int est = h.fb_hot_est >= 0 && h.fb_est_c == c ? h.fb_hot_est : h.cl[c].n_hot;  // (another candidate's: its own)
    // the hot kernel's grid from a count a few frames old: with headroom (2x + 64 tiles), since a hot set that grew
    // past its grid's waves -- a moving camera's, after frames of few hot tiles -- is rendered by too few waves (dragon
    // walkthrough frames of 3-6 ms among ~1.1 ms ones); a persistent grid's waves that find no tile exit at once
    const int est_h = 2 * est + 64;
    int nc, np;
    rtl::hybrid_grids(rp, rcp, hot ? est_h : 0, A.n_tiles, nc, np);
    // (no hot candidate: the whole frame, costliest first)
    return launch_hot_cold(ctx, Grid{kc, nc, 0, B}, Grid{kp, np, dyn, with_slots(P, dyn)});
}

// the persistent grids' work counters (d_work), and the ray counters, which restart with every launch (rt_get_stats
// reports the frame, not the trial launches)
int clear_counters(rt_ctx* ctx) {
    if (!ctx->batch_sum)  // a per-frame loop of a batch keeps adding to the batch's counters
        HIPC(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned long long) * rtd::NCOUNT, ctx->stream));
    HIPC(hipMemsetAsync(ctx->d_work, 0, 1024, ctx->stream));
    return RT_OK;
}

// One frame of RT_VARIANT_HYBRID: what hybrid_pick says (P: the whole frame's arguments in the launch's dealing order)
int dispatch_hybrid(rt_ctx* ctx, Launch& L, int cp, rtd::KArgs& P) {
    rt_ctx::Hybrid& h = ctx->hy;
    rt_launch_info& li = L.li;
    Pick pk{};
    if (int rc = hybrid_pick(ctx, L, pk)) return rc;
    // (a hybrid frame on device-built lists has its list builder clear the counters)
    const bool fb = PRT_FEEDBACK && pk.kind == 2 && h.fb_ok && h.d_cost;
    if (PRT_FEEDBACK && !fb)
        if (int rc = clear_counters(ctx)) return rc;
    // the frame's HIP-event time starts here, after the host work of the pick (the trials compare them)
    HIPC(hipEventRecord(ctx->ev0, ctx->stream));
    if (pk.kind == 2) {
        li.hot_pct = h.cand[pk.c].pct;
        li.hot_lanes = h.cand[pk.c].lanes;
        li.cold_variant = h.cand[pk.c].cold;
    }
    // every frame of the shape records its tiles' durations (rt_feedback.hpp); a hybrid candidate's frame --
    // tried or chosen -- builds its lists from the previous frame's first, on the device (the memset follows
    // that build: k_coop's hot tiles combine their group tiles' times by atomic max). The trials too: with a
    // moving camera the measuring frame's lists age frame by frame, and a candidate tried later would be
    // priced with older lists than one tried first (a car_boxed walkthrough settled on the wrong candidate).
    if (PRT_FEEDBACK && h.d_cost) {
        if (fb) {
            const int rc = launch_hybrid_fb(ctx, L.A, L.count, pk.c, &li.build);
            h.fb_ok = rc == RT_OK;
            return rc;
        }
        unsigned* w = h.cost_at(h.cost_cur ^ 1);
        HIPC(hipMemsetAsync(w, 0, sizeof(unsigned) * (h.n_tiles + 1), ctx->stream));
        P.tile_cost = w;
        L.A.tile_cost = w;
        h.cost_cur ^= 1;
        h.fb_ok = true;  // (this frame, in stream order, fills it)
    }
    if (pk.kind == 2) return launch_hybrid(ctx, L.A, L.count, pk.c, &li.build);
    if (pk.kind == 0) {  // measuring frame: k_persist with per-tile times, copied to the host behind it
        li.variant = RT_VARIANT_PERSIST;
        li.refresh = h.choice >= 0 ? 1 : 0;  // a decided shape's periodic list refresh (settled)
        li.trial = li.refresh ? 0 : 1;
        li.settled = li.refresh;
        P.tile_trace = h.d_tr;
        launch_paths(P, RT_VARIANT_PERSIST, L.count, ctx->device, ctx->stream, cp, ctx->pk_ok, ctx->tq_ok, ctx->list_ok, &li.build);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(h.h_tr, h.d_tr, sizeof(unsigned long long) * 4 * h.n_tiles, hipMemcpyDeviceToHost,
                            ctx->stream));
        HIPC(hipEventRecord(h.ev, ctx->stream));
        h.state = 1;
        return RT_OK;
    }
    // a whole-frame kernel: chosen, tried, or while the measurement / trials are on their way
    li.variant = pk.c;
    launch_paths(P, pk.c, L.count, ctx->device, ctx->stream, cp, ctx->pk_ok, ctx->tq_ok, ctx->list_ok, &li.build);
    return RT_OK;
}

// one frame (or one batch) of configuration (variant md, cap cp)
int dispatch(rt_ctx* ctx, Launch& L, int md, int cp) {
    const rt_frame* f = L.f;
    // (a hybrid frame clears after its pick: dispatch_hybrid)
    if (!(PRT_FEEDBACK && md == RT_VARIANT_HYBRID))
        if (int rc = clear_counters(ctx)) return rc;
    L.li.variant = md;
    if (L.kernel == RT_KERNEL_STRICT) {
        L.li.variant = 0;
        const dim3 grid((f->width + 15) / 16, (f->n_rows + 15) / 16);
        tiles_kernel(f->bounces, L.count)<<<grid, rtd::BLOCK, 0, ctx->stream>>>(L.A);
        return RT_OK;
    }
    if (md == RT_VARIANT_COOP2 || md == RT_VARIANT_COOP4) {
        rtd::KArgs B = L.A;
        const int gr = md == RT_VARIANT_COOP2 ? 2 : 4;
        int tw, th;
        hot_tile(gr, tw, th);  // rtd::GTile<gr>
        B.tiles_x = (f->width + tw - 1) / tw;
        const int ty = (f->n_rows + th - 1) / th;
        B.n_tiles = B.tiles_x * ty;
        if (int rc = order_for(ctx, L, B.tiles_x, ty, B.tile_order)) return rc;
        return launch_group(B, gr, L.count, ctx->device, ctx->stream, cp);
    }
    rtd::KArgs P = L.A;
    if (L.region_off) {
        P.region_off = L.region_off;
        P.tile_order = L.region_order;
    }
    if (md == RT_VARIANT_HYBRID) return dispatch_hybrid(ctx, L, cp, P);
    launch_paths(P, md, L.count, ctx->device, ctx->stream, cp, ctx->pk_ok, ctx->tq_ok, ctx->list_ok, &L.li.build);
    return RT_OK;
}

// diagnostics: PRT_TILE_TRACE=<file> writes 4 x uint64 per tile of a k_persist frame (rt_kernels.hpp)
// (s_memrealtime, 100 MHz); synchronous, never used by tests or the bench
int write_tile_trace(rt_ctx* ctx, unsigned long long* d_trace, size_t n_tiles, const char* path) {
    std::vector<unsigned long long> h(4 * n_tiles);
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipMemcpy(h.data(), d_trace, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    HIPC(hipFree(d_trace));
    if (FILE* fp = std::fopen(path, "wb")) {
        std::fwrite(h.data(), sizeof(unsigned long long), h.size(), fp);
        std::fclose(fp);
    }
    return RT_OK;
}

// rt_render / rt_render_frames: n_frames frames of the same shape (cameras cams[0..n_frames-1]); outputs
// [n_frames][n_rows][width]... Persistent fast configurations trace the whole batch in ONE launch (frames'
// tiles interleaved in the dealing order); other kernels launch once per frame.
int render_batch(rt_ctx* ctx, const rt_camera* cams, int n_frames, const rt_frame* f, const rt_outputs* out) {
    if (!ctx) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_render: no scene uploaded";
        return RT_E_STATE;
    }
    if (!cams || !f) return arg_err(ctx, "rt_render: null camera/frame");
    int spp_grid = 1;
    if (const char* why = rtl::check_frame(*f, n_frames, spp_grid)) return arg_err(ctx, why);
    HIPC(hipSetDevice(ctx->device));
    Launch L;
    L.f = f;
    L.cams = cams;
    L.n_frames = n_frames;
    L.kernel = f->kernel == RT_KERNEL_AUTO ? RT_KERNEL_FAST : f->kernel;
    L.count = (ctx->flags & RT_FLAG_COUNTERS) != 0;
    rtd::KArgs& A = L.A;
    const size_t pixels = (size_t)f->width * f->n_rows;  // per frame
    const size_t all_px = pixels * (size_t)n_frames;
    float* rgb = out ? out->rgb : nullptr;
    unsigned* bgra = out ? out->bgra : nullptr;
    if (!rgb && !bgra)
        if (int rc = own_rgb(ctx, all_px, rgb)) return rc;
    fill_args(ctx, L, out, rgb, bgra, spp_grid);
    if (n_frames > 1 && L.kernel != RT_KERNEL_FAST) {  // one launch per frame, outputs at frame offsets
        for (int i = 0; i < n_frames; i++) {
            rt_outputs o{rgb ? rgb + 3 * pixels * i : nullptr, A.hit ? A.hit + pixels * i : nullptr,
                         A.t ? A.t + pixels * i : nullptr,
                         A.bounce_hit ? A.bounce_hit + pixels * f->bounces * i : nullptr,
                         bgra ? bgra + pixels * i : nullptr};
            ctx->batch_sum = i > 0;
            const int rc = render_batch(ctx, cams + i, 1, f, &o);
            ctx->batch_sum = false;
            if (rc) return rc;
        }
        ctx->last_rgb = rgb;
        ctx->last_bgra = bgra;
        ctx->last_hit = A.hit;
        ctx->last_pixels = all_px;
        ctx->last_frames = n_frames;
        return RT_OK;
    }
    A.n_frames = n_frames;
    A.frame_px = pixels;
    if (L.kernel == RT_KERNEL_FAST)
        if (int rc = walk_buffers(ctx)) return rc;
    A.pathbuf = ctx->d_pathbuf;
    A.lanebuf = ctx->d_lanebuf;
    A.gstack = ctx->d_gstack;
    A.wcap = ctx->wide.n > 0 ? std::max(1, std::max(ctx->wide.depth, std::max(ctx->unit.depth, ctx->prim.depth))) : 0;
    if (n_frames > 1) {  // the batch's cameras, uploaded when they change
        if (int rc = upload_cams(ctx, cams, n_frames)) return rc;
        A.cams = ctx->d_cams;
    }
    A.regroup = f->regroup > 0 ? f->regroup : 16;
    const int slot = (int)(ctx->launches % rt_ctx::NEV);
    ctx->ev0 = ctx->ev0s[slot];
    ctx->ev1 = ctx->ev1s[slot];
    const char* trace_path = std::getenv("PRT_TILE_TRACE");  // (write_tile_trace)
    unsigned long long* d_trace = nullptr;
    const size_t trace_n = (size_t)A.n_tiles;
    if (trace_path && L.kernel == RT_KERNEL_FAST && n_frames == 1 && f->spp == 1) {
        HIPC(hipMalloc((void**)&d_trace, sizeof(unsigned long long) * 4 * trace_n));
        HIPC(hipMemsetAsync(d_trace, 0, sizeof(unsigned long long) * 4 * trace_n, ctx->stream));
        A.tile_trace = d_trace;
    }
    if (int rc = tile_orders(ctx, L)) return rc;
    L.caps = launch_caps(ctx, L);
    int mode = rtl::resolve_variant(L.caps, f->variant);
    L.li.settled = 1;
    // the measured rule of frame batches and spp > 1, where the pool can run and nothing forbids trials
    if (f->variant == RT_VARIANT_DEFAULT && L.kernel == RT_KERNEL_FAST && !A.tile_trace && !L.count &&
        (n_frames > 1 || f->spp > 1) && L.caps.shp_ok)
        if (int rc = batch_rule_pick(ctx, L, mode)) return rc;
    HIPC(hipEventRecord(ctx->ev0, ctx->stream));
    if (int rc = dispatch(ctx, L, mode, f->waves_cap)) return rc;
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ctx->ev1, ctx->stream));
    if (d_trace)
        if (int rc = write_tile_trace(ctx, d_trace, trace_n, trace_path)) return rc;
    ctx->last_launch = L.li;
    ctx->launches++;
    ctx->last_rgb = rgb;
    ctx->last_bgra = bgra;
    ctx->last_hit = A.hit;
    ctx->last_pixels = all_px;
    ctx->last_frames = n_frames;
    ctx->last_W = f->width;
    ctx->last_H = f->height;
    ctx->last_off = f->row_offset;
    ctx->last_stride = f->row_stride;
    ctx->last_rows = f->n_rows;
    ctx->last_block = A.row_block;
    ctx->last_shift = f->frame_shift;
    ctx->rendered = true;
    return RT_OK;
}
}  // namespace

extern "C" int rt_render(rt_ctx* ctx, const rt_camera* cam, const rt_frame* f, const rt_outputs* out) {
    return render_batch(ctx, cam, 1, f, out);
}

extern "C" int rt_render_frames(rt_ctx* ctx, const rt_camera* cams, int n_frames, const rt_frame* f,
                                const rt_outputs* out) {
    return render_batch(ctx, cams, n_frames, f, out);
}

extern "C" int rt_get_launch_info(rt_ctx* ctx, rt_launch_info* info) {
    if (!ctx || !info) return RT_E_ARG;
    if (!ctx->rendered) {
        ctx->err = "rt_get_launch_info: nothing rendered";
        return RT_E_STATE;
    }
    *info = ctx->last_launch;
    return RT_OK;
}

// ---------------------------------------------------------------- the queries' shared steps
// An entry point reads: the checks (rtq::check_enter, the family's own, rtq::check_args), query_begin, fill A, pick the
// kernel, query_launch. Its info call: query_read, the family's fields, query_finish.
namespace {
// The family's slot made ready for a new query, after every check (a refused call leaves the family's info as it was)
// and before the n = 0 return (an empty query reports zero counters and no kernel time); A: the kernel's arguments,
// cleared, with the slot's counters in them.
template <class Args>
int query_begin(rt_ctx* ctx, rtq::Fam f, int ncount, Args& A) {
    rt_ctx::QuerySlot& q = ctx->slots[f];
    HIPC(hipSetDevice(ctx->device));
    const size_t cbytes = sizeof(unsigned long long) * (ncount + 1);
    if (!q.counters) HIPC(hipMalloc((void**)&q.counters, cbytes));
    if (!q.ev0) HIPC(hipEventCreate(&q.ev0));
    if (!q.ev1) HIPC(hipEventCreate(&q.ev1));
    HIPC(hipMemsetAsync(q.counters, 0, cbytes, ctx->stream));
    q.run = true;
    q.launched = false;
    std::memset(&A, 0, sizeof A);
    A.counters = q.counters;
    A.work = reinterpret_cast<unsigned int*>(q.counters + ncount);
    return RT_OK;
}

// resident workgroups of a query kernel with `dyn` bytes of dynamic LDS (the occupancy query once per kernel, not per
// query); must_fit: 0 when a workgroup of it does not fit a CU, where the others count one per CU (resident())
template <class K>
int query_resident(rt_ctx* ctx, K k, size_t dyn = 0, bool must_fit = false) {
    auto res = ctx->residents.find((const void*)k);
    if (res != ctx->residents.end()) return res->second;
    bool fits = true;
    if (must_fit) {
        int per_cu = 0;
        fits = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, rtd::BLOCK, dyn) == hipSuccess && per_cu >= 1;
        (void)hipGetLastError();
    }
    const int n = fits ? resident(k, ctx->device, 8, dyn) : 0;
    ctx->residents.emplace((const void*)k, n);
    return n;
}

// the kernel over A.n queries, between the slot's events
template <class Args>
int query_launch(rt_ctx* ctx, rtq::Fam f, void (*k)(Args), const Args& A, size_t dyn = 0) {
    rt_ctx::QuerySlot& q = ctx->slots[f];
    const int blocks = rtq::grid_blocks(A.n, rtd::QUERY_CHUNK, query_resident(ctx, k, dyn));
    HIPC(hipEventRecord(q.ev0, ctx->stream));
    k<<<blocks, rtd::BLOCK, dyn, ctx->stream>>>(A);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(q.ev1, ctx->stream));
    q.launched = true;
    return RT_OK;
}

// The counters of the family's last query into c (after a wait for the stream), and a cleared info; none_run: the
// family's message when it has run none.
template <class Info, size_t N>
int query_read(rt_ctx* ctx, rtq::Fam f, const char* none_run, unsigned long long (&c)[N], Info* info) {
    if (!ctx || !info) return RT_E_ARG;
    if (!ctx->slots[f].run) {
        ctx->err = none_run;
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipMemcpy(c, ctx->slots[f].counters, sizeof c, hipMemcpyDeviceToHost));
    std::memset(info, 0, sizeof *info);
    return RT_OK;
}

// The kernel's time when one was launched, and RT_E_KERNEL when its walks overflowed a stack; too_deep: what was
// (the three ray families walk every view, the others the wide view only).
constexpr const char* DEEP_BVH = "BVH deeper than the walks' stacks";
constexpr const char* DEEP_WIDE = "wide view deeper than the walk's stack";
int query_finish(rt_ctx* ctx, rtq::Fam f, const char* who, unsigned long long overflows, const char* too_deep,
                 float* kernel_ms) {
    const rt_ctx::QuerySlot& q = ctx->slots[f];
    if (q.launched) HIPC(hipEventElapsedTime(kernel_ms, q.ev0, q.ev1));
    if (overflows) {
        ctx->err = std::string(who) + ": the query's traversal stack overflowed " + std::to_string(overflows) +
                   " times (" + too_deep + "): its results are not valid";
        return RT_E_KERNEL;
    }
    return RT_OK;
}

// fn<CAP, STRICT> of a list family: the build with the smallest capacity that holds cap entries (rtq::list_capacity)
#define FOR_LIST_CAP(cap, strict, fn)                                                          \
    (rtq::list_capacity(cap) == 0   ? ((strict) ? fn<0, true> : fn<0, false>)                  \
     : rtq::list_capacity(cap) == 4 ? ((strict) ? fn<4, true> : fn<4, false>)                  \
     : rtq::list_capacity(cap) == 8 ? ((strict) ? fn<8, true> : fn<8, false>)                  \
                                    : ((strict) ? fn<16, true> : fn<16, false>))

// d_ref_inv of the scene (rt_neighbours.hpp ref_inv), made on first use
int ensure_ref_inv(rt_ctx* ctx) {
    if (ctx->d_ref_inv) return RT_OK;
    const int nt = ctx->n_tris;
    HIPC(hipMalloc((void**)&ctx->d_ref_inv, sizeof(int) * (size_t)std::max(nt, 1)));
    HIPC(hipMemsetAsync(ctx->d_ref_inv, 0, sizeof(int) * (size_t)std::max(nt, 1), ctx->stream));
    if (nt > 0) {
        rtd::k_invert_orig<<<(nt + 255) / 256, 256, 0, ctx->stream>>>(ctx->ref.orig, nt, ctx->d_ref_inv);
        HIPC(hipGetLastError());
    }
    return RT_OK;
}
}  // namespace

// ---------------------------------------------------------------- ray queries (rt_query.hpp)
namespace {
using QFn = void (*)(rtd::QArgs);
QFn query_kernel(int kind, bool strict, bool tq, bool pool) {
    using rtd::k_query;
    if (pool) return tq ? k_query<1, false, true, true> : k_query<1, false, false, true>;
    if (kind == RT_QUERY_CLOSEST) {
        if (strict) return k_query<0, true, false>;
        return tq ? k_query<0, false, true> : k_query<0, false, false>;
    }
    if (strict) return k_query<1, true, false>;
    return tq ? k_query<1, false, true> : k_query<1, false, false>;
}
}  // namespace

extern "C" int rt_trace_rays(rt_ctx* ctx, const rt_rays* r, const rt_ray_results* out) {
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::RAYS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (r->kind != RT_QUERY_CLOSEST && r->kind != RT_QUERY_OCCLUDED) return arg_err(ctx, "rt_trace_rays: bad kind");
    if (int rc = rtq::check_args(rtq::RAYS, r->kernel, r->n, ctx->err)) return rc;
    if (r->regroup < 0 || r->regroup > 64) return arg_err(ctx, "rt_trace_rays: regroup must be 0..64");
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->origin || !r->dir)) return arg_err(ctx, "rt_trace_rays: null origin / dir");
    if (r->n > 0 && r->kind == RT_QUERY_OCCLUDED && (!r->max_dist2 || !out->occluded))
        return arg_err(ctx, "rt_trace_rays: RT_QUERY_OCCLUDED needs max_dist2 and an occluded output");
    if (r->n > 0 && r->kind == RT_QUERY_CLOSEST && !out->hit && !out->t)
        return arg_err(ctx, "rt_trace_rays: RT_QUERY_CLOSEST needs a hit or a t output");
    rtd::QArgs A;
    if (int rc = query_begin(ctx, rtq::RAYS, rtd::Q_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the primary view is chosen per ray)
    A.origin = r->origin;
    A.dir = r->dir;
    A.max_dist2 = r->max_dist2;
    A.hit = out->hit;
    A.t = out->t;
    A.occluded = out->occluded;
    A.n = r->n;
    A.o_max = 4.0f * ctx->scene_mx;
    const bool strict = r->kernel == RT_KERNEL_STRICT;
    // the pool form (rt_query.hpp occluded_pool): the fast occlusion query on a wide view; regroup = its refill
    // threshold in idle lanes (0: 16), 64 = the lockstep form instead. The closest-hit query has the lockstep form only.
    const bool pool = r->kind == RT_QUERY_OCCLUDED && !strict && ctx->wide.n > 0 && r->regroup != 64;
    A.regroup = r->regroup > 0 ? r->regroup : 16;
    return query_launch(ctx, rtq::RAYS, query_kernel(r->kind, strict, ctx->tq_ok, pool), A);
}

extern "C" int rt_get_query_info(rt_ctx* ctx, rt_query_info* info) {
    unsigned long long c[rtd::Q_NCOUNT];
    if (int rc = query_read(ctx, rtq::RAYS, "rt_get_query_info: no query traced", c, info)) return rc;
    info->rays = (long long)c[rtd::Q_RAYS];
    info->hits = (long long)c[rtd::Q_HITS];
    info->unit_rays = (long long)c[rtd::Q_UNIT];
    info->short_rays = (long long)c[rtd::Q_SHORT];
    info->full_rays = (long long)c[rtd::Q_FULL];
    info->strict_rays = (long long)c[rtd::Q_STRICT];
    info->tie_rewalks = (long long)c[rtd::Q_TIE];
    info->stack_overflows = (long long)c[rtd::Q_ERR];
    return query_finish(ctx, rtq::RAYS, "rt_get_query_info", c[rtd::Q_ERR], DEEP_BVH, &info->kernel_ms);
}

// ---------------------------------------------------------------- vertex updates (rt_refit.hpp)
namespace {

// the smallest double x whose square root reaches thr: sqrt is correctly rounded, hence monotonic, so hittable()'s
// sqrt(len2) >= thr is len2 >= x, which the plan kernel evaluates without a device square root
double sqrt_threshold(double thr) {
    double x = thr * thr;
    while (x > 0.0 && std::sqrt(x) >= thr) x = std::nextafter(x, 0.0);
    while (std::sqrt(x) < thr) x = std::nextafter(x, (double)INFINITY);
    return x;
}

// A binary view's records by tree level, from the device's own records (a record's parent is its 4th float4's z and
// precedes it: build_view numbers the records in preorder). Once per topology; waits for the stream.
int make_bin_topo(rt_ctx* ctx, const DevView& v, RefitTopo& t) {
    if (t.made) return RT_OK;
    const int n = v.n_inner;
    std::vector<float4> h(4 * (size_t)n);
    HIPC(hipStreamSynchronize(ctx->stream));
    if (n) HIPC(hipMemcpy(h.data(), v.nodes, sizeof(float4) * h.size(), hipMemcpyDeviceToHost));
    std::vector<int> depth(n, 0);
    int levels = 0;
    for (int r = 0; r < n; r++) {
        int par;
        std::memcpy(&par, &h[4 * (size_t)r + 3].z, 4);
        if (par >= r) {
            ctx->err = "rt_update_vertices: a binary view's records are not in preorder";
            return RT_E_STATE;
        }
        depth[r] = par < 0 ? 0 : depth[par] + 1;
        levels = std::max(levels, depth[r] + 1);
    }
    t.off.assign((size_t)levels + 1, 0);
    for (int r = 0; r < n; r++) t.off[(size_t)depth[r] + 1]++;
    for (int l = 0; l < levels; l++) t.off[(size_t)l + 1] += t.off[l];
    std::vector<int> list(std::max(n, 1)), at(t.off.begin(), t.off.end());
    for (int r = 0; r < n; r++) list[at[depth[r]]++] = r;
    HIPC(hipMalloc((void**)&t.d_list, sizeof(int) * list.size()));
    HIPC(hipMemcpy(t.d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    HIPC(hipMalloc((void**)&t.d_exact, sizeof(float4) * 2 * (size_t)std::max(n, 1)));
    t.made = true;
    return RT_OK;
}

// A wide view's levels: the collapse lays the nodes out breadth first, every level one range whose interior slots'
// children, in node and slot order, are the next range (rt_wide.cpp) -- checked here. bitmap: also the set of the
// triangles the view holds (a subset view's membership). Once per topology; waits for the stream.
int make_wide_topo(rt_ctx* ctx, const DevWide& w, RefitTopo& t, bool bitmap) {
    if (t.made) return RT_OK;
    const int n = w.n;
    std::vector<uint32_t> h(20 * (size_t)n);
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipMemcpy(h.data(), w.nodes, sizeof(uint32_t) * h.size(), hipMemcpyDeviceToHost));
    t.off = {0, 1};
    for (;;) {
        const int s = t.off[t.off.size() - 2], e = t.off.back();
        long long next = e;
        for (int k = s; k < e; k++) {
            const uint32_t* W = &h[20 * (size_t)k];
            const int kids = __builtin_popcount(W[3] >> 24);
            if (kids && (long long)W[4] != next) {
                ctx->err = "rt_update_vertices: a wide view's nodes are not in breadth-first order";
                return RT_E_STATE;
            }
            next += kids;
        }
        if (next == e) break;
        if (next > n) {
            ctx->err = "rt_update_vertices: a wide view's child index is out of range";
            return RT_E_STATE;
        }
        t.off.push_back((int)next);
    }
    if (t.off.back() != n) {
        ctx->err = "rt_update_vertices: a wide view has unreachable nodes";
        return RT_E_STATE;
    }
    HIPC(hipMalloc((void**)&t.d_exact, sizeof(float4) * 2 * (size_t)n));
    if (bitmap) {
        const size_t words = ((size_t)ctx->n_tris + 31) / 32;
        HIPC(hipMalloc((void**)&t.d_bits, sizeof(unsigned) * words));
        HIPC(hipMemsetAsync(t.d_bits, 0, sizeof(unsigned) * words, ctx->stream));
        rtr::k_member<<<(w.tris_n + 255) / 256, 256, 0, ctx->stream>>>(w.orig, w.tris_n, t.d_bits);
        HIPC(hipGetLastError());
    }
    t.made = true;
    return RT_OK;
}

// steps 2-3 for one binary view: its triangle records, then its child boxes level by level, deepest first
int refit_binary(rt_ctx* ctx, const DevView& v, const RefitTopo& t, const float* coords, float inflate) {
    hipStream_t st = ctx->stream;
    rtr::k_tri_records<<<(ctx->n_tris + 255) / 256, 256, 0, st>>>(coords, v.orig, ctx->n_tris, v.tris);
    for (int l = (int)t.off.size() - 2; l >= 0; l--) {
        const int cnt = t.off[(size_t)l + 1] - t.off[l];
        if (cnt <= 0) continue;
        rtr::k_bin_level<<<(cnt + 255) / 256, 256, 0, st>>>(t.d_list + t.off[l], cnt, v.nodes, v.leaves, v.orig, coords,
                                                            t.d_exact, inflate);
    }
    HIPC(hipGetLastError());
    return RT_OK;
}

// steps 2 and 4 for one wide view (area: the full view's decoded-area accumulator, else null)
int refit_wide(rt_ctx* ctx, const DevWide& w, const RefitTopo& t, const float* coords, float inflate, double* area) {
    hipStream_t st = ctx->stream;
    rtr::k_tri_records<<<(w.tris_n + 255) / 256, 256, 0, st>>>(coords, w.orig, w.tris_n, w.tris);
    for (int l = (int)t.off.size() - 2; l >= 0; l--) {
        const int first = t.off[l], cnt = t.off[(size_t)l + 1] - first;
        rtr::k_wide_level<<<(cnt + 63) / 64, 64, 0, st>>>(first, cnt, w.nodes, w.orig, coords, t.d_exact, inflate, area);
    }
    HIPC(hipGetLastError());
    return RT_OK;
}

// The face lists' buffers, made with the per-topology data (first update after an upload; waits for the stream): the
// upload's array holds the distinct faces only, a refit writes all four per record. The lists in use move over as
// they are, so that an update refused after this point leaves the scene as it was.
int make_face_buffers(rt_ctx* ctx) {
    const int n = ctx->ref.n_inner;
    if (ctx->faces_own || n == 0) return RT_OK;
    const size_t m = 4 * (size_t)n, have = (size_t)ctx->n_face[0] + ctx->n_face[1] + ctx->n_face[2];
    float* grown = nullptr;
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipMalloc((void**)&grown, sizeof(float) * 3 * m));
    if (ctx->d_faces && have > 0 && have <= 3 * m)
        HIPC(hipMemcpy(grown, ctx->d_faces, sizeof(float) * have, hipMemcpyDeviceToDevice));
    if (ctx->d_faces) HIPC(hipFree(ctx->d_faces));
    ctx->d_faces = grown;
    HIPC(hipMalloc((void**)&ctx->d_face_tmp, sizeof(float) * 3 * m));
    HIPC(hipcub::DeviceRadixSort::SortKeys(nullptr, ctx->sort_bytes, ctx->d_face_tmp, ctx->d_faces, (int)m, 0, 32,
                                           ctx->stream));
    HIPC(hipMalloc(&ctx->d_sort_tmp, std::max<size_t>(ctx->sort_bytes, 16)));
    ctx->faces_own = true;
    return RT_OK;
}

// step 3's second half: the reference view's face coordinates per axis, sorted on the device (duplicates stay:
// on_face needs order only)
int refit_faces(rt_ctx* ctx) {
    const int n = ctx->ref.n_inner;
    if (n == 0) {
        for (int& f : ctx->n_face) f = 0;
        return RT_OK;
    }
    hipStream_t st = ctx->stream;
    const int m = 4 * n;
    rtr::k_faces<<<(n + 255) / 256, 256, 0, st>>>(ctx->ref.nodes, n, ctx->d_face_tmp);
    HIPC(hipGetLastError());
    for (int a = 0; a < 3; a++) {
        size_t bytes = ctx->sort_bytes;
        HIPC(hipcub::DeviceRadixSort::SortKeys(ctx->d_sort_tmp, bytes, ctx->d_face_tmp + (size_t)a * m,
                                               ctx->d_faces + (size_t)a * m, m, 0, 32, st));
        ctx->n_face[a] = m;
    }
    return RT_OK;
}

// step 5: a subset view whose membership changed, rebuilt through the upload's own path (subset_view) over the new
// triangles; none where the new subset is empty or leaves out too little (the full view then serves)
int rebuild_subset(rt_ctx* ctx, const rt_scene* s2, double dmax, size_t fewer_than, float inflate, DevWide& d,
                   RefitTopo& t) {
    HostWide hw;
    int rc = subset_view(ctx, s2, dmax, fewer_than, ctx->built_accel, inflate, hw);
    if (rc) return rc;
    HIPC(hipStreamSynchronize(ctx->stream));
    free_wide(d);
    free_topo(t);
    return upload_wide(ctx, hw, d);
}

}  // namespace

namespace {
// rt_update_vertices; report: the update becomes the one rt_get_update_info answers for (a view rebuild runs the same
// update without touching that state); inflate_out (nullable): the new inflation
int update_vertices(rt_ctx* ctx, const rt_vertex_update* u, bool report, float* inflate_out) {
    if (!ctx) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_update_vertices: no scene uploaded";
        return RT_E_STATE;
    }
    if (!u || !u->coords) return arg_err(ctx, "rt_update_vertices: null update / coords");
    if (u->n_triangles != ctx->n_tris) return arg_err(ctx, "rt_update_vertices: n_triangles differs from the uploaded scene's");
    HIPC(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n = ctx->n_tris;
    const float* coords = u->coords;
    if (!ctx->d_plan) HIPC(hipMalloc((void**)&ctx->d_plan, sizeof(unsigned) * rtr::P_WORDS));
    if (!ctx->d_area) HIPC(hipMalloc((void**)&ctx->d_area, sizeof(double) * 5));
    if (!ctx->h_plan) HIPC(hipHostMalloc((void**)&ctx->h_plan, sizeof(unsigned) * rtr::P_WORDS, hipHostMallocDefault));
    if (!ctx->u_ev0) HIPC(hipEventCreate(&ctx->u_ev0));
    if (!ctx->u_ev1) HIPC(hipEventCreate(&ctx->u_ev1));
    if (!ctx->u_evs) HIPC(hipEventCreate(&ctx->u_evs));
    // the per-topology data (first update after an upload or a rebuild)
    int rc;
    if ((rc = make_bin_topo(ctx, ctx->ref, ctx->tp_ref))) return rc;
    if (ctx->acc.nodes && (rc = make_bin_topo(ctx, ctx->acc, ctx->tp_acc))) return rc;
    if (ctx->wide.nodes && (rc = make_wide_topo(ctx, ctx->wide, ctx->tp_wide, false))) return rc;
    if (ctx->unit.nodes && (rc = make_wide_topo(ctx, ctx->unit, ctx->tp_unit, true))) return rc;
    if (ctx->prim.nodes && (rc = make_wide_topo(ctx, ctx->prim, ctx->tp_prim, true))) return rc;
    if ((rc = make_face_buffers(ctx))) return rc;
    // (the start event becomes u_ev0 only when the update is made: a refused one leaves the last update's pair alone)
    HIPC(hipEventRecord(ctx->u_evs, st));
    // 1. the plan pass (read-only), and the one host wait
    const float floor16 = 16.0f;
    unsigned init[rtr::P_WORDS] = {0, 0, 0, 0};
    std::memcpy(&init[rtr::P_MX], &floor16, 4);
    std::memcpy(ctx->h_plan, init, sizeof init);
    HIPC(hipMemcpyAsync(ctx->d_plan, ctx->h_plan, sizeof init, hipMemcpyHostToDevice, st));
    const double x_unit = sqrt_threshold(UNIT_KEEP * (double)rtd::EPS / 1.0);
    const double x_prim = sqrt_threshold(UNIT_KEEP * (double)rtd::EPS / PRIMARY_D);
    rtr::k_plan<<<(n + 255) / 256, 256, 0, st>>>(coords, n, ctx->tp_unit.d_bits, ctx->tp_prim.d_bits, x_unit, x_prim,
                                                 ctx->d_plan);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(ctx->h_plan, ctx->d_plan, sizeof init, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (ctx->h_plan[rtr::P_BAD]) return arg_err(ctx, "rt_update_vertices: a coordinate is not finite (nothing was changed)");
    float scene_mx;
    std::memcpy(&scene_mx, &ctx->h_plan[rtr::P_MX], 4);
    if (!(scene_mx <= RT_COORD_MAX))
        return arg_err(ctx, "rt_update_vertices: a coordinate is beyond RT_COORD_MAX (nothing was changed)");
    const float inflate = std::ldexp(scene_mx, -16);
    rt_update_info ui{};
    ui.joined_unit = (int)ctx->h_plan[rtr::P_JOIN_UNIT];
    ui.joined_primary = (int)ctx->h_plan[rtr::P_JOIN_PRIM];
    ui.scene_magnitude = scene_mx;
    ui.area_ratio = 1.0f;
    // 5. views that triangles joined: the slow path, on the host
    const bool re_unit = ctx->unit.nodes && ui.joined_unit > 0, re_prim = ctx->prim.nodes && ui.joined_primary > 0;
    if (re_unit || re_prim) {
        std::vector<float> hv(9 * (size_t)n);
        HIPC(hipMemcpy(hv.data(), coords, sizeof(float) * hv.size(), hipMemcpyDeviceToHost));
        std::vector<rt_triangle> T((size_t)n);
        const rt_vec3 zero{0.0f, 0.0f, 0.0f};
        for (int i = 0; i < n; i++) {  // (the builds read coords and centroid)
            const float* p = &hv[9 * (size_t)i];
            const rt_vec3 a{p[0], p[1], p[2]}, b{p[3], p[4], p[5]}, c{p[6], p[7], p[8]};
            rth_triangle_init(&T[i], &a, &b, &c, &zero, &zero, &zero);
        }
        rt_scene s2{};
        s2.triangles = T.data();
        s2.n_triangles = n;
        s2.ploc_radius = ctx->ploc_radius;
        s2.collapse_node_cost = ctx->collapse_cost;
        if (re_unit && (rc = rebuild_subset(ctx, &s2, 1.0, (size_t)n, inflate, ctx->unit, ctx->tp_unit))) return rc;
        if (re_prim && (rc = rebuild_subset(ctx, &s2, PRIMARY_D, (size_t)n - (size_t)n / 50, inflate, ctx->prim, ctx->tp_prim)))
            return rc;
        ui.views_rebuilt = (int)re_unit + (int)re_prim;
        ctx->pk_ok = std::max(ctx->wide.n, std::max(ctx->unit.n, ctx->prim.n)) <= rtd::WIDE_MAX_NODES &&
                     !(ctx->flags & RT_FLAG_UNPACKED_STACK);
        ctx->info.unit_triangles = ctx->unit.tris_n;
        ctx->info.unit_nodes = ctx->unit.n;
        ctx->info.unit_depth = ctx->unit.depth;
        ctx->info.primary_triangles = ctx->prim.tris_n;
        ctx->info.primary_nodes = ctx->prim.n;
    }
    // 2. the shading normals (the views' triangle records with each view below)
    rtr::k_shade_normals<<<(n + 255) / 256, 256, 0, st>>>(coords, n, ctx->d_shade);
    HIPC(hipGetLastError());
    // 3. the binary trees: the reference tree with its own boxes, the acceleration tree's grown by the inflation
    if ((rc = refit_binary(ctx, ctx->ref, ctx->tp_ref, coords, 0.0f))) return rc;
    if (ctx->acc.nodes && (rc = refit_binary(ctx, ctx->acc, ctx->tp_acc, coords, inflate))) return rc;
    if ((rc = refit_faces(ctx))) return rc;
    // 4. the wide views not rebuilt above
    if (ctx->wide.nodes) {
        if (!ctx->area_base) {  // the denominator: the un-updated nodes of this build
            HIPC(hipMemsetAsync(ctx->d_area, 0, sizeof(double), st));
            rtr::k_wide_area<<<(ctx->wide.n + 255) / 256, 256, 0, st>>>(ctx->wide.nodes, ctx->wide.n, ctx->d_area);
            HIPC(hipGetLastError());
            ctx->area_base = true;
        }
        HIPC(hipMemsetAsync(ctx->d_area + 1, 0, sizeof(double), st));
        if ((rc = refit_wide(ctx, ctx->wide, ctx->tp_wide, coords, inflate, ctx->d_area + 1))) return rc;
        ui.views_refit++;
    }
    if (ctx->unit.nodes && !re_unit) {
        if ((rc = refit_wide(ctx, ctx->unit, ctx->tp_unit, coords, inflate, nullptr))) return rc;
        ui.views_refit++;
    }
    if (ctx->prim.nodes && !re_prim) {
        if ((rc = refit_wide(ctx, ctx->prim, ctx->tp_prim, coords, inflate, nullptr))) return rc;
        ui.views_refit++;
    }
    ctx->scene_mx = scene_mx;
    if (inflate_out) *inflate_out = inflate;
    if (!report) return RT_OK;
    std::swap(ctx->u_ev0, ctx->u_evs);
    HIPC(hipEventRecord(ctx->u_ev1, st));
    ctx->uinfo = ui;
    ctx->updated = true;
    return RT_OK;
}
}  // namespace

extern "C" int rt_update_vertices(rt_ctx* ctx, const rt_vertex_update* u) { return update_vertices(ctx, u, true, nullptr); }

extern "C" int rt_get_update_info(rt_ctx* ctx, rt_update_info* info) {
    if (!ctx || !info) return RT_E_ARG;
    if (!ctx->updated) {
        ctx->err = "rt_get_update_info: no vertex update made";
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    *info = ctx->uinfo;
    if (ctx->wide.nodes && ctx->area_base) {
        double a[2] = {0.0, 0.0};
        HIPC(hipMemcpy(a, ctx->d_area, sizeof a, hipMemcpyDeviceToHost));
        info->area_ratio = a[0] > 0.0 ? (float)(a[1] / a[0]) : 1.0f;
    }
    HIPC(hipEventElapsedTime(&info->update_ms, ctx->u_ev0, ctx->u_ev1));
    return RT_OK;
}

extern "C" int rt_update_lights(rt_ctx* ctx, const rt_light* lights, int n_lights) {
    if (!ctx) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_update_lights: no scene uploaded";
        return RT_E_STATE;
    }
    if (n_lights != ctx->n_lights) return arg_err(ctx, "rt_update_lights: n_lights differs from the uploaded scene's");
    if (n_lights > 0 && !lights) return arg_err(ctx, "rt_update_lights: null lights");
    if (n_lights == 0) return RT_OK;
    HIPC(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float4) * 2 * (size_t)n_lights;
    if (!ctx->lights_ev) HIPC(hipEventCreateWithFlags(&ctx->lights_ev, hipEventDisableTiming));
    else HIPC(hipEventSynchronize(ctx->lights_ev));  // (the staging's previous copy has run)
    if (!ctx->h_lights) HIPC(hipHostMalloc((void**)&ctx->h_lights, bytes, hipHostMallocDefault));
    for (int j = 0; j < n_lights; j++) {  // the upload's 32-B layout
        ctx->h_lights[2 * j] = make_float4(lights[j].pos.x, lights[j].pos.y, lights[j].pos.z, 0.0f);
        ctx->h_lights[2 * j + 1] = make_float4(lights[j].kl.x, lights[j].kl.y, lights[j].kl.z, 0.0f);
    }
    HIPC(hipMemcpyAsync(ctx->d_lights, ctx->h_lights, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipEventRecord(ctx->lights_ev, ctx->stream));
    return RT_OK;
}

extern "C" int rt_debug_read_wide(rt_ctx* ctx, int view, unsigned int* nodes, int cap_nodes, int* tri_orig, int cap_tris) {
    if (!ctx || view < 0 || view > 2 || cap_nodes < 0 || cap_tris < 0) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_debug_read_wide: no scene uploaded";
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    const DevWide& w = view == 0 ? ctx->wide : (view == 1 ? ctx->unit : ctx->prim);
    if (!w.nodes) return 0;
    const int nn = std::min(w.n, cap_nodes), nt = std::min(w.tris_n, cap_tris);
    if (nodes && nn > 0) HIPC(hipMemcpy(nodes, w.nodes, sizeof(unsigned) * 20 * (size_t)nn, hipMemcpyDeviceToHost));
    if (tri_orig && nt > 0) HIPC(hipMemcpy(tri_orig, w.orig, sizeof(int) * (size_t)nt, hipMemcpyDeviceToHost));
    return w.n;
}

// ---------------------------------------------------------------- view rebuilds (rt_collapse.hpp)
namespace {

using clk = std::chrono::steady_clock;
float ms_since(clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); }

// A wide view built for a rebuild, not yet part of the context: the view, its refit data (made with it: the levels are
// known here) and, from the device path, the binary tree it was collapsed from.
struct NewView {
    DevWide w;
    RefitTopo t;
    rt_ctx::BuildTree bt;
    void release() {
        free_wide(w);
        free_topo(t);
        free_build_tree(bt);
    }
};

// the device path's working buffers beside PLOC's
struct CollapseDev {
    int *flag = nullptr, *at = nullptr, *sub = nullptr, *item = nullptr, *item2 = nullptr, *slots = nullptr;
    float* v = nullptr;
    float4* nodes = nullptr;
    unsigned long long *sums = nullptr, *scan = nullptr, *tot = nullptr;  // tot: pinned
    void* tmp = nullptr;
    void release() {
        if (tot) (void)hipHostFree(tot);
        for (void* p : {(void*)flag, (void*)at, (void*)sub, (void*)item, (void*)item2, (void*)slots, (void*)v, (void*)nodes,
                        (void*)sums, (void*)scan, tmp})
            if (p) (void)hipFree(p);
        *this = CollapseDev();
    }
};

struct RebuildTimes {
    float ploc = 0.0f, collapse = 0.0f, fill = 0.0f;
    int launches = 0;
};

enum { WHY_NONE = 0, WHY_DEEP = 1, WHY_NODES = 2 };

// One view on the device from the coordinates of all n_all triangles. x < 0: the full view; else the subset whose
// |n|^2 >= x, when it has members and fewer than fewer_than (else out stays empty). area (nullable): += the view's
// decoded child-box area. why: RT_E_STATE's reason (too deep for the wide walk). Waits for the stream per PLOC round
// and per wide level; nothing of the context's scene is touched.
int device_view(rt_ctx* ctx, const float* coords, int n_all, double x, size_t fewer_than, int R, float inflate,
                double* area, NewView& out, RebuildTimes& tm, int& why, PlocDev& P, CollapseDev& D) {
    hipStream_t st = ctx->stream;
    auto t0 = clk::now();
    int m = n_all;
    const float* v = coords;
    HIPC(hipHostMalloc((void**)&D.tot, sizeof(unsigned long long) * 2, hipHostMallocDefault));
    if (x >= 0.0) {  // a. subset compaction
        HIPC(hipMalloc((void**)&D.flag, sizeof(int) * n_all));
        HIPC(hipMalloc((void**)&D.at, sizeof(int) * n_all));
        size_t bytes = 0;
        HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, D.flag, D.at, n_all, st));
        HIPC(hipMalloc(&D.tmp, std::max<size_t>(bytes, 16)));
        rtc::k_hittable<<<(n_all + 255) / 256, 256, 0, st>>>(coords, n_all, x, D.flag);
        HIPC(hipGetLastError());
        HIPC(hipcub::DeviceScan::ExclusiveSum(D.tmp, bytes, D.flag, D.at, n_all, st));
        int* last = (int*)D.tot;
        HIPC(hipMemcpyAsync(last, D.flag + n_all - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(last + 1, D.at + n_all - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        m = last[0] + last[1];
        tm.launches += 4;
        if (m <= 0 || (size_t)m >= fewer_than) return RT_OK;
        HIPC(hipMalloc((void**)&D.sub, sizeof(int) * m));
        HIPC(hipMalloc((void**)&D.v, sizeof(float) * 9 * (size_t)m));
        rtc::k_gather<<<(n_all + 255) / 256, 256, 0, st>>>(coords, n_all, D.flag, D.at, D.sub, D.v);
        HIPC(hipGetLastError());
        tm.launches++;
        v = D.v;
        (void)hipFree(D.tmp);  // (the scan over the level's nodes below sizes its own)
        D.tmp = nullptr;
    }
    // b. PLOC from the device vertices
    int rc;
    if ((rc = ploc_alloc(ctx, P, m))) return rc;
    if ((rc = ploc_build(ctx, P, v, R))) {
        if (rc == RT_E_STATE) ctx->err = "rt_rebuild_views: the device build made no progress";
        return rc;
    }
    tm.launches += 5 + 10 * P.rounds;
    tm.ploc += ms_since(t0);
    t0 = clk::now();
    // c, d. the greedy collapse, one launch pair and one scan per wide level
    const int cap = m;  // wide nodes are distinct binary nodes of more than 4 triangles, or the root
    HIPC(hipMalloc((void**)&D.nodes, sizeof(float4) * 5 * (size_t)cap));
    HIPC(hipMalloc((void**)&D.item, sizeof(int) * cap));
    HIPC(hipMalloc((void**)&D.item2, sizeof(int) * cap));
    HIPC(hipMalloc((void**)&D.slots, sizeof(int) * 8 * (size_t)cap));
    HIPC(hipMalloc((void**)&D.sums, sizeof(unsigned long long) * cap));
    HIPC(hipMalloc((void**)&D.scan, sizeof(unsigned long long) * cap));
    HIPC(hipMalloc((void**)&out.w.orig, sizeof(int) * m));
    size_t scan_bytes = 0;
    HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, D.sums, D.scan, cap, st));
    HIPC(hipMalloc(&D.tmp, std::max<size_t>(scan_bytes, 16)));
    HIPC(hipMemcpyAsync(D.item, P.C, sizeof(int), hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(&out.bt.root, P.C, sizeof(int), hipMemcpyDeviceToHost, st));
    const rtc::DevTree tree{P.left, P.right, P.cnt, P.nlo, P.nhi, m};
    int first = 0, count = 1;
    long long tri_first = 0;
    out.t.off = {0};
    while (count > 0) {
        if ((long long)first + count > cap) {
            ctx->err = "rt_rebuild_views: the collapse made more wide nodes than binary nodes";
            return RT_E_STATE;
        }
        if ((int)out.t.off.size() > rtd::WSTACK) {
            ctx->err = "rt_rebuild_views: the device tree is too deep for the wide walk";
            why = WHY_DEEP;
            return RT_E_STATE;
        }
        const int g = (count + 63) / 64;
        rtc::k_collapse<<<g, 64, 0, st>>>(tree, D.item, count, D.slots, D.sums);
        HIPC(hipGetLastError());
        size_t b = scan_bytes;
        HIPC(hipcub::DeviceScan::ExclusiveSum(D.tmp, b, D.sums, D.scan, count, st));
        HIPC(hipMemcpyAsync(D.tot, D.sums + count - 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPC(hipMemcpyAsync(D.tot + 1, D.scan + count - 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        rtc::k_emit<<<g, 64, 0, st>>>(tree, D.slots, D.scan, first, count, first + count, (int)tri_first, P.sorted, D.sub,
                                      D.nodes, D.item2, out.w.orig);
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(st));
        tm.launches += 5;
        const unsigned long long total = D.tot[0] + D.tot[1];
        first += count;
        out.t.off.push_back(first);
        count = (int)(total >> 32);
        tri_first += (long long)(total & 0xFFFFFFFFull);
        std::swap(D.item, D.item2);
        if (tri_first > m) break;
    }
    if (tri_first != m) {
        ctx->err = "rt_rebuild_views: the collapse did not place every triangle once";
        return RT_E_STATE;
    }
    const int n_wide = first;
    tm.collapse += ms_since(t0);
    t0 = clk::now();
    // e. the view's own buffers and the refit's fill: records, then boxes level by level, deepest first
    HIPC(hipMalloc((void**)&out.w.nodes, sizeof(float4) * 5 * (size_t)n_wide));
    HIPC(hipMalloc((void**)&out.w.tris, sizeof(float4) * 3 * (size_t)m));
    HIPC(hipMalloc((void**)&out.t.d_exact, sizeof(float4) * 2 * (size_t)n_wide));
    HIPC(hipMemcpyAsync(out.w.nodes, D.nodes, sizeof(float4) * 5 * (size_t)n_wide, hipMemcpyDeviceToDevice, st));
    out.w.n = n_wide;
    out.w.depth = (int)out.t.off.size() - 1;
    out.w.tris_n = m;
    out.t.made = true;
    int rf;
    if ((rf = refit_wide(ctx, out.w, out.t, coords, inflate, area))) return rf;
    tm.launches += 2 + out.w.depth;
    if (x >= 0.0) {  // a subset view's membership bitmap (make_wide_topo's)
        const size_t words = ((size_t)n_all + 31) / 32;
        HIPC(hipMalloc((void**)&out.t.d_bits, sizeof(unsigned) * words));
        HIPC(hipMemsetAsync(out.t.d_bits, 0, sizeof(unsigned) * words, st));
        rtr::k_member<<<(m + 255) / 256, 256, 0, st>>>(out.w.orig, m, out.t.d_bits);
        HIPC(hipGetLastError());
        tm.launches += 2;
    }
    // the collapsed tree, kept for the test read-back: PLOC's child arrays as they are, the leaves' scene triangles
    HIPC(hipMalloc((void**)&out.bt.leaf, sizeof(int) * m));
    rtc::k_leaf_ids<<<(m + 255) / 256, 256, 0, st>>>(P.sorted, D.sub, m, out.bt.leaf);
    HIPC(hipGetLastError());
    out.bt.left = P.left;
    out.bt.right = P.right;
    P.left = P.right = nullptr;
    out.bt.n = m;
    HIPC(hipStreamSynchronize(st));  // (the working buffers are freed by the caller)
    tm.fill += ms_since(t0);
    return RT_OK;
}

// the new coordinates as host triangles (the builds read coords and centroid)
int download_triangles(rt_ctx* ctx, const float* coords, int n, std::vector<rt_triangle>& T) {
    std::vector<float> hv(9 * (size_t)n);
    HIPC(hipStreamSynchronize(ctx->stream));
    HIPC(hipMemcpy(hv.data(), coords, sizeof(float) * hv.size(), hipMemcpyDeviceToHost));
    T.resize((size_t)n);
    const rt_vec3 zero{0.0f, 0.0f, 0.0f};
    for (int i = 0; i < n; i++) {
        const float* p = &hv[9 * (size_t)i];
        const rt_vec3 a{p[0], p[1], p[2]}, b{p[3], p[4], p[5]}, c{p[6], p[7], p[8]};
        rth_triangle_init(&T[i], &a, &b, &c, &zero, &zero, &zero);
    }
    return RT_OK;
}

// the three views through the upload's own path (wide_view / subset_view) over downloaded coordinates
int host_views(rt_ctx* ctx, const float* coords, int n, float inflate, NewView nv[3], RebuildTimes& tm) {
    std::vector<rt_triangle> T;
    int rc = download_triangles(ctx, coords, n, T);
    if (rc) return rc;
    const float keep[3] = {ctx->t_ploc, ctx->t_treelet, ctx->t_collapse};  // (the upload's stage times stay its own)
    ctx->t_ploc = ctx->t_treelet = ctx->t_collapse = 0.0f;
    rt_scene s2{};
    s2.triangles = T.data();
    s2.n_triangles = n;
    s2.ploc_radius = ctx->ploc_radius;
    s2.collapse_node_cost = ctx->collapse_cost;
    const int R = ctx->ploc_radius > 0 ? std::min(ctx->ploc_radius, rtb::PLOC_R_MAX) : rtb::PLOC_R;
    HostWide hw[3];
    int built = ctx->built_accel;
    rc = wide_view(ctx, T.data(), n, built, R, inflate, ctx->collapse_cost, hw[0]);
    if (rc == RT_E_STATE && built == RT_ACCEL_GPU) {  // too deep for the wide walk: the host build, as the upload does
        built = RT_ACCEL_HOST;
        hw[0] = HostWide();
        rc = wide_view(ctx, T.data(), n, built, R, inflate, ctx->collapse_cost, hw[0]);
    }
    if (rc == RT_E_STATE) ctx->err = "rt_rebuild_views: no wide view could be built over the new coordinates";
    if (!rc) rc = subset_view(ctx, &s2, 1.0, (size_t)n, built, inflate, hw[1]);
    if (!rc) rc = subset_view(ctx, &s2, PRIMARY_D, (size_t)n - (size_t)n / 50, built, inflate, hw[2]);
    tm.ploc = ctx->t_ploc + ctx->t_treelet;
    tm.collapse = ctx->t_collapse;
    ctx->t_ploc = keep[0];
    ctx->t_treelet = keep[1];
    ctx->t_collapse = keep[2];
    if (rc) return rc;
    const auto t0 = clk::now();
    for (int k = 0; k < 3; k++)
        if ((rc = upload_wide(ctx, hw[k], nv[k].w))) return rc;
    tm.fill = ms_since(t0);
    return RT_OK;
}

}  // namespace

extern "C" int rt_rebuild_views(rt_ctx* ctx, const rt_view_rebuild* r) {
    if (!ctx) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_rebuild_views: no scene uploaded";
        return RT_E_STATE;
    }
    if (!r || !r->coords) return arg_err(ctx, "rt_rebuild_views: null rebuild / coords");
    if (r->mode < RT_REBUILD_AUTO || r->mode > RT_REBUILD_HOST) return arg_err(ctx, "rt_rebuild_views: bad mode");
    if (r->n_triangles != ctx->n_tris) return arg_err(ctx, "rt_rebuild_views: n_triangles differs from the uploaded scene's");
    if (!ctx->wide.nodes) {
        ctx->err = "rt_rebuild_views: the scene has no wide view (RT_ACCEL_REFERENCE)";
        return RT_E_STATE;
    }
    if (r->mode == RT_REBUILD_DEVICE && ctx->built_accel != RT_ACCEL_GPU)
        return arg_err(ctx, "rt_rebuild_views: RT_REBUILD_DEVICE needs a scene built with RT_ACCEL_GPU");
    HIPC(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const auto t_call = clk::now();
    if (!ctx->r_ev0) HIPC(hipEventCreate(&ctx->r_ev0));
    if (!ctx->r_ev1) HIPC(hipEventCreate(&ctx->r_ev1));
    if (!ctx->r_evs) HIPC(hipEventCreate(&ctx->r_evs));
    HIPC(hipEventRecord(ctx->r_evs, st));  // (becomes r_ev0 only when the rebuild is made)
    // 1. the whole vertex update
    const rt_vertex_update u{r->coords, r->n_triangles};
    float inflate = 0.0f;
    int rc = update_vertices(ctx, &u, false, &inflate);
    if (rc) return rc;
    const int n = ctx->n_tris;
    // 2. the new views into fresh buffers
    NewView nv[3];
    RebuildTimes tm;
    rt_rebuild_info ri{};
    bool device = r->mode == RT_REBUILD_DEVICE || (r->mode == RT_REBUILD_AUTO && ctx->built_accel == RT_ACCEL_GPU);
    auto drop = [&]() {
        for (NewView& v : nv) v.release();
    };
    HIPC(hipMemsetAsync(ctx->d_area + 4, 0, sizeof(double), st));
    if (device) {
        const int R = ctx->ploc_radius > 0 ? std::min(ctx->ploc_radius, rtb::PLOC_R_MAX) : rtb::PLOC_R;
        const double xs[3] = {-1.0, sqrt_threshold(UNIT_KEEP * (double)rtd::EPS / 1.0),
                              sqrt_threshold(UNIT_KEEP * (double)rtd::EPS / PRIMARY_D)};
        const size_t fewer[3] = {0, (size_t)n, (size_t)n - (size_t)n / 50};
        int why = WHY_NONE;
        for (int k = 0; k < 3 && !rc; k++) {
            PlocDev P;
            CollapseDev D;
            rc = device_view(ctx, r->coords, n, xs[k], fewer[k], R, inflate, k == 0 ? ctx->d_area + 4 : nullptr, nv[k],
                             tm, why, P, D);
            if (rc) (void)hipStreamSynchronize(st);
            P.release();
            D.release();
            if (!rc && nv[k].w.n > rtd::WIDE_MAX_NODES && r->mode == RT_REBUILD_AUTO) {
                rc = RT_E_STATE;
                why = WHY_NODES;
            }
        }
        if (rc == RT_E_STATE && why != WHY_NONE && r->mode == RT_REBUILD_AUTO) {  // the fallback
            drop();
            tm = RebuildTimes();
            ri.fell_back = why;
            device = false;
            rc = RT_OK;
            HIPC(hipMemsetAsync(ctx->d_area + 4, 0, sizeof(double), st));
        }
    }
    if (!rc && !device) {
        rc = host_views(ctx, r->coords, n, inflate, nv, tm);
        if (!rc) {
            rtr::k_wide_area<<<(nv[0].w.n + 255) / 256, 256, 0, st>>>(nv[0].w.nodes, nv[0].w.n, ctx->d_area + 4);
            if (hipGetLastError() != hipSuccess) rc = RT_E_HIP;
        }
    }
    if (rc || !nv[0].w.nodes) {  // the refitted scene stays
        drop();
        return rc ? rc : RT_E_STATE;
    }
    // 3, 4. swap the views in (stream order: everything issued so far has run) and free the old ones with their topologies
    HIPC(hipStreamSynchronize(st));
    DevWide* views[3] = {&ctx->wide, &ctx->unit, &ctx->prim};
    RefitTopo* topos[3] = {&ctx->tp_wide, &ctx->tp_unit, &ctx->tp_prim};
    for (int k = 0; k < 3; k++) {
        free_wide(*views[k]);
        free_topo(*topos[k]);
        free_build_tree(ctx->bt[k]);
        *views[k] = nv[k].w;
        *topos[k] = nv[k].t;
        ctx->bt[k] = nv[k].bt;
        ri.nodes[k] = nv[k].w.n;
        ri.depth[k] = nv[k].w.depth;
        ri.views_built += nv[k].w.nodes != nullptr;
    }
    // 5. the next area_ratio is measured against the rebuilt view ([3]: the area before, [0] = [1] = [2]: the area after)
    HIPC(hipMemcpyAsync(ctx->d_area + 3, ctx->d_area + 1, sizeof(double), hipMemcpyDeviceToDevice, st));
    for (int k = 0; k < 3; k++)
        HIPC(hipMemcpyAsync(ctx->d_area + k, ctx->d_area + 4, sizeof(double), hipMemcpyDeviceToDevice, st));
    ctx->area_base = true;
    // 6, 7. the packed layouts' bound and the scene report
    ctx->pk_ok = std::max(ctx->wide.n, std::max(ctx->unit.n, ctx->prim.n)) <= rtd::WIDE_MAX_NODES &&
                 !(ctx->flags & RT_FLAG_UNPACKED_STACK);
    ctx->info.wide_nodes = ctx->wide.n;
    ctx->info.wide_depth = ctx->wide.depth;
    ctx->info.unit_triangles = ctx->unit.tris_n;
    ctx->info.unit_nodes = ctx->unit.n;
    ctx->info.unit_depth = ctx->unit.depth;
    ctx->info.primary_triangles = ctx->prim.tris_n;
    ctx->info.primary_nodes = ctx->prim.n;
    std::swap(ctx->r_ev0, ctx->r_evs);
    HIPC(hipEventRecord(ctx->r_ev1, st));
    ri.mode_used = device ? RT_REBUILD_DEVICE : RT_REBUILD_HOST;
    ri.launches = tm.launches;
    ri.ploc_ms = tm.ploc;
    ri.collapse_ms = tm.collapse;
    ri.fill_ms = tm.fill;
    ri.host_ms = ms_since(t_call);
    ctx->rinfo = ri;
    ctx->rebuilt = true;
    return RT_OK;
}

extern "C" int rt_get_rebuild_info(rt_ctx* ctx, rt_rebuild_info* info) {
    if (!ctx || !info) return RT_E_ARG;
    if (!ctx->rebuilt) {
        ctx->err = "rt_get_rebuild_info: no view rebuild made";
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    *info = ctx->rinfo;
    double a[2] = {0.0, 0.0};
    HIPC(hipMemcpy(a, ctx->d_area + 2, sizeof a, hipMemcpyDeviceToHost));
    info->area_after = a[0];
    info->area_before = a[1];
    HIPC(hipEventElapsedTime(&info->rebuild_ms, ctx->r_ev0, ctx->r_ev1));
    return RT_OK;
}

extern "C" int rt_debug_read_build_tree(rt_ctx* ctx, int view, int* left, int* right, int* leaf_tri, int cap, int* root) {
    if (!ctx || view < 0 || view > 2 || cap < 0) return RT_E_ARG;
    if (!ctx->has_scene) {
        ctx->err = "rt_debug_read_build_tree: no scene uploaded";
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    const rt_ctx::BuildTree& b = ctx->bt[view];
    if (!b.leaf) return 0;
    const int nl = std::min(b.n, cap), ni = std::min(b.n - 1, cap);
    if (leaf_tri && nl > 0) HIPC(hipMemcpy(leaf_tri, b.leaf, sizeof(int) * (size_t)nl, hipMemcpyDeviceToHost));
    if (left && ni > 0) HIPC(hipMemcpy(left, b.left, sizeof(int) * (size_t)ni, hipMemcpyDeviceToHost));
    if (right && ni > 0) HIPC(hipMemcpy(right, b.right, sizeof(int) * (size_t)ni, hipMemcpyDeviceToHost));
    if (root) *root = b.root;
    return b.n;
}

// ---------------------------------------------------------------- radiance queries (rt_shade.hpp)
namespace {
using SFn = void (*)(rtd::SArgs);
template <int MAXB>
SFn shade_kernel_of(bool strict, bool tq, bool pool) {
    using rtd::k_shade;
    if (strict) return k_shade<MAXB, true, false, false>;
    if (pool) return tq ? k_shade<MAXB, false, true, true> : k_shade<MAXB, false, false, true>;
    return tq ? k_shade<MAXB, false, true, false> : k_shade<MAXB, false, false, false>;
}
SFn shade_kernel(int bounces, bool strict, bool tq, bool pool) {
    return FOR_MAXB(bounces, shade_kernel_of, strict, tq, pool);
}
template <int MAXB>
size_t shade_lds_of(bool tq) { return rtd::shade_pool_lds<MAXB>(tq); }
size_t shade_lds(int bounces, bool tq) { return FOR_MAXB(bounces, shade_lds_of, tq); }
// The library's choice for regroup = 0: the pool form at 16 idle lanes (measured, DESIGN.md §3l: 28 % less time than
// the lockstep form on dragon's row-major camera rays, 3 % more on car_boxed's).
constexpr int SHADE_REGROUP_DEFAULT = 16;
}  // namespace

extern "C" int rt_shade_rays(rt_ctx* ctx, const rt_shade* r, const rt_shade_results* out) {
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::SHADE, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::SHADE, r->kernel, r->n, ctx->err)) return rc;
    if (r->bounces < 1 || r->bounces > 8) return arg_err(ctx, "rt_shade_rays: bounces must be 1..8");
    if (r->regroup < 0 || r->regroup > 64) return arg_err(ctx, "rt_shade_rays: regroup must be 0..64");
    if (r->unclamped != 0 && r->unclamped != 1) return arg_err(ctx, "rt_shade_rays: unclamped must be 0 or 1");
    if (r->unclamped && out->bgra) return arg_err(ctx, "rt_shade_rays: unclamped has no bgra quantisation");
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->origin || !r->dir)) return arg_err(ctx, "rt_shade_rays: null origin / dir");
    if (r->n > 0 && !out->rgb && !out->bgra && !out->hit && !out->t && !out->bounce_hit)
        return arg_err(ctx, "rt_shade_rays: no output");
    rtd::SArgs A;
    if (int rc = query_begin(ctx, rtq::SHADE, rtd::S_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the primary view is chosen per ray)
    A.origin = r->origin;
    A.dir = r->dir;
    A.rgb = out->rgb;
    A.bgra = out->bgra;
    A.hit = out->hit;
    A.t = out->t;
    A.bounce_hit = out->bounce_hit;
    A.n = r->n;
    A.bounces = r->bounces;
    A.o_max = 4.0f * ctx->scene_mx;
    A.unclamped = r->unclamped;
    const bool strict = r->kernel == RT_KERNEL_STRICT;
    // the pool form (rt_shade.hpp shade_pool): the fast kernel on a wide view whose lights fit trace_path_dfr's 8-bit masks
    // and whose nodes fit the pool's packed stack entries; regroup = its refill threshold, 64 = the lockstep form
    const int regroup = r->regroup > 0 ? r->regroup : SHADE_REGROUP_DEFAULT;
    bool pool = !strict && regroup != 64 && ctx->wide.n > 0 && ctx->n_lights <= 8 && ctx->pk_ok;
    A.regroup = regroup;
    // (a k_shade build counts 0 resident workgroups when one does not fit a CU: query_resident's must_fit)
    SFn k = nullptr;
    size_t dyn = 0;
    if (pool) {
        k = shade_kernel(r->bounces, false, ctx->tq_ok, true);
        dyn = shade_lds(r->bounces, ctx->tq_ok);
        if (query_resident(ctx, k, dyn, true) == 0) pool = false;  // its LDS does not fit: the lockstep form
    }
    if (!pool) {
        k = shade_kernel(r->bounces, strict, ctx->tq_ok, false);
        dyn = 0;
        if (query_resident(ctx, k, 0, true) == 0)
            return arg_err(ctx, "rt_shade_rays: the kernel does not fit this device");
    }
    return query_launch(ctx, rtq::SHADE, k, A, dyn);
}

extern "C" int rt_get_shade_info(rt_ctx* ctx, rt_shade_info* info) {
    unsigned long long c[rtd::S_NCOUNT];
    if (int rc = query_read(ctx, rtq::SHADE, "rt_get_shade_info: no rays shaded", c, info)) return rc;
    info->rays = (long long)c[rtd::S_RAYS];
    info->hits = (long long)c[rtd::S_HITS];
    info->reflection = (long long)c[rtd::S_REFL];
    info->shadow = (long long)c[rtd::S_SHAD];
    info->shadow_skipped = (long long)c[rtd::S_SKIP];
    info->strict_paths = (long long)c[rtd::S_STRICT];
    info->tie_rewalks = (long long)c[rtd::S_TIE];
    info->stack_overflows = (long long)c[rtd::S_ERR];
    return query_finish(ctx, rtq::SHADE, "rt_get_shade_info", c[rtd::S_ERR], DEEP_BVH, &info->kernel_ms);
}

// ---------------------------------------------------------------- multi-hit queries (rt_hits.hpp)
extern "C" int rt_trace_hits(rt_ctx* ctx, const rt_hits* r, const rt_hit_results* out) {
    static_assert(RT_HITS_MAX == rtd::HITS_MAX && RT_HITS_MAX == rtq::LIST_MAX,
                  "rt_hip.h, rt_hits.hpp and rt_query_logic.hpp must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::HITS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::HITS, r->kernel, r->n, r->max_hits, r->count_all, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->origin || !r->dir)) return arg_err(ctx, "rt_trace_hits: null origin / dir");
    if (r->n > 0 && r->max_hits > 0 && !out->tri && !out->t)
        return arg_err(ctx, "rt_trace_hits: max_hits > 0 needs a tri or a t output");
    if (int rc = rtq::check_count_out(rtq::HITS, r->n, r->max_hits, out->count != nullptr, ctx->err)) return rc;
    rtd::HArgs A;
    if (int rc = query_begin(ctx, rtq::HITS, rtd::H_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the view is chosen per ray)
    A.origin = r->origin;
    A.dir = r->dir;
    A.t_max = r->t_max;
    A.tri = out->tri;
    A.t = out->t;
    A.count = out->count;
    A.n = r->n;
    A.o_max = 4.0f * ctx->scene_mx;
    A.max_hits = r->max_hits;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::HITS, FOR_LIST_CAP(r->max_hits, r->kernel == RT_KERNEL_STRICT, rtd::k_hits), A);
}

extern "C" int rt_get_hits_info(rt_ctx* ctx, rt_hits_info* info) {
    unsigned long long c[rtd::H_NCOUNT];
    if (int rc = query_read(ctx, rtq::HITS, "rt_get_hits_info: no hits query traced", c, info)) return rc;
    info->rays = (long long)c[rtd::H_RAYS];
    info->rays_hit = (long long)c[rtd::H_RAYS_HIT];
    info->hits_stored = (long long)c[rtd::H_STORED];
    info->hits_counted = (long long)c[rtd::H_COUNTED];
    info->unit_rays = (long long)c[rtd::H_UNIT];
    info->short_rays = (long long)c[rtd::H_SHORT];
    info->full_rays = (long long)c[rtd::H_FULL];
    info->exhaustive_rays = (long long)c[rtd::H_EXH];
    info->stack_overflows = (long long)c[rtd::H_ERR];
    return query_finish(ctx, rtq::HITS, "rt_get_hits_info", c[rtd::H_ERR], DEEP_BVH, &info->kernel_ms);
}

// ---------------------------------------------------------------- nearest-surface queries (rt_nearest.hpp)
extern "C" int rt_nearest_points(rt_ctx* ctx, const rt_points* r, const rt_nearest_results* out) {
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::NEAREST, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::NEAREST, r->kernel, r->n, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && !r->point) return arg_err(ctx, "rt_nearest_points: null point");
    if (r->n > 0 && !out->tri && !out->d2 && !out->point)
        return arg_err(ctx, "rt_nearest_points: needs a tri, a d2 or a point output");
    rtd::NArgs A;
    if (int rc = query_begin(ctx, rtq::NEAREST, rtd::N_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.point = r->point;
    A.max_dist2 = r->max_dist2;
    A.tri = out->tri;
    A.d2 = out->d2;
    A.out = out->point;
    A.n = r->n;
    void (*k)(rtd::NArgs) = r->kernel == RT_KERNEL_STRICT ? rtd::k_nearest<true> : rtd::k_nearest<false>;
    return query_launch(ctx, rtq::NEAREST, k, A);
}

extern "C" int rt_get_nearest_info(rt_ctx* ctx, rt_nearest_info* info) {
    unsigned long long c[rtd::N_NCOUNT];
    if (int rc = query_read(ctx, rtq::NEAREST, "rt_get_nearest_info: no nearest query run", c, info)) return rc;
    info->points = (long long)c[rtd::N_POINTS];
    info->found = (long long)c[rtd::N_FOUND];
    info->walked_points = (long long)c[rtd::N_WALKED];
    info->exhaustive_points = (long long)c[rtd::N_EXH];
    info->empty_points = (long long)c[rtd::N_EMPTY];
    info->nodes_visited = (long long)c[rtd::N_NODES];
    info->tris_tested = (long long)c[rtd::N_TRIS];
    info->stack_overflows = (long long)c[rtd::N_ERR];
    return query_finish(ctx, rtq::NEAREST, "rt_get_nearest_info", c[rtd::N_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- neighbour queries (rt_neighbours.hpp)
extern "C" int rt_nearest_tris(rt_ctx* ctx, const rt_neighbours* r, const rt_neighbour_results* out) {
    static_assert(RT_NEIGHBOURS_MAX == rtd::NEIGHBOURS_MAX && RT_NEIGHBOURS_MAX == rtq::LIST_MAX,
                  "rt_hip.h, rt_neighbours.hpp and rt_query_logic.hpp must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::NEIGHBOURS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::NEIGHBOURS, r->kernel, r->n, r->max_tris, r->count_all, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && !r->point) return arg_err(ctx, "rt_nearest_tris: null point");
    if (r->n > 0 && r->max_tris > 0 && !out->tri && !out->d2 && !out->point)
        return arg_err(ctx, "rt_nearest_tris: max_tris > 0 needs a tri, a d2 or a point output");
    if (int rc = rtq::check_count_out(rtq::NEIGHBOURS, r->n, r->max_tris, out->count != nullptr, ctx->err)) return rc;
    rtd::BArgs A;
    if (int rc = query_begin(ctx, rtq::NEIGHBOURS, rtd::B_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    const bool want_p = r->max_tris > 0 && out->point;
    if (want_p)
        if (int rc = ensure_ref_inv(ctx)) return rc;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.point = r->point;
    A.max_dist2 = r->max_dist2;
    A.tri = r->max_tris > 0 ? out->tri : nullptr;
    A.d2 = r->max_tris > 0 ? out->d2 : nullptr;
    A.out = want_p ? out->point : nullptr;
    A.count = out->count;
    A.ref_inv = ctx->d_ref_inv;
    A.n = r->n;
    A.max_tris = r->max_tris;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::NEIGHBOURS, FOR_LIST_CAP(r->max_tris, r->kernel == RT_KERNEL_STRICT, rtd::k_neighbours),
                        A);
}

extern "C" int rt_get_neighbours_info(rt_ctx* ctx, rt_neighbours_info* info) {
    unsigned long long c[rtd::B_NCOUNT];
    if (int rc = query_read(ctx, rtq::NEIGHBOURS, "rt_get_neighbours_info: no neighbours query run", c, info))
        return rc;
    info->points = (long long)c[rtd::B_POINTS];
    info->found = (long long)c[rtd::B_FOUND];
    info->tris_stored = (long long)c[rtd::B_STORED];
    info->tris_counted = (long long)c[rtd::B_COUNTED];
    info->walked_points = (long long)c[rtd::B_WALKED];
    info->exhaustive_points = (long long)c[rtd::B_EXH];
    info->empty_points = (long long)c[rtd::B_EMPTY];
    info->nodes_visited = (long long)c[rtd::B_NODES];
    info->tris_tested = (long long)c[rtd::B_TRIS];
    info->stack_overflows = (long long)c[rtd::B_ERR];
    return query_finish(ctx, rtq::NEIGHBOURS, "rt_get_neighbours_info", c[rtd::B_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- overlap queries (rt_overlap.hpp)
extern "C" int rt_overlap_boxes(rt_ctx* ctx, const rt_boxes* r, const rt_overlap_results* out) {
    static_assert(RT_OVERLAPS_MAX == rtd::OVERLAPS_MAX && RT_OVERLAPS_MAX == rtq::LIST_MAX,
                  "rt_hip.h, rt_overlap.hpp and rt_query_logic.hpp must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::OVERLAPS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::OVERLAPS, r->kernel, r->n, r->max_tris, r->count_all, ctx->err)) return rc;
    if ((r->offsets != nullptr) != (out->list != nullptr))
        return arg_err(ctx, "rt_overlap_boxes: offsets and list are given together or not at all");
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->lo || !r->hi)) return arg_err(ctx, "rt_overlap_boxes: null lo / hi");
    if (r->n > 0 && r->max_tris > 0 && !out->tri) return arg_err(ctx, "rt_overlap_boxes: max_tris > 0 needs a tri output");
    if (int rc = rtq::check_count_out(rtq::OVERLAPS, r->n, r->max_tris, out->count != nullptr, ctx->err)) return rc;
    rtd::OArgs A;
    if (int rc = query_begin(ctx, rtq::OVERLAPS, rtd::O_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.lo = r->lo;
    A.hi = r->hi;
    A.offsets = r->offsets;
    A.tri = r->max_tris > 0 ? out->tri : nullptr;
    A.count = out->count;
    A.list = out->list;
    A.n = r->n;
    A.max_tris = r->max_tris;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::OVERLAPS, FOR_LIST_CAP(r->max_tris, r->kernel == RT_KERNEL_STRICT, rtd::k_overlap),
                        A);
}

extern "C" int rt_get_overlaps_info(rt_ctx* ctx, rt_overlaps_info* info) {
    unsigned long long c[rtd::O_NCOUNT];
    if (int rc = query_read(ctx, rtq::OVERLAPS, "rt_get_overlaps_info: no overlap query run", c, info)) return rc;
    info->boxes = (long long)c[rtd::O_BOXES];
    info->found = (long long)c[rtd::O_FOUND];
    info->tris_stored = (long long)c[rtd::O_STORED];
    info->tris_counted = (long long)c[rtd::O_COUNTED];
    info->tris_listed = (long long)c[rtd::O_LISTED];
    info->walked_boxes = (long long)c[rtd::O_WALKED];
    info->exhaustive_boxes = (long long)c[rtd::O_EXH];
    info->empty_boxes = (long long)c[rtd::O_EMPTY];
    info->nodes_visited = (long long)c[rtd::O_NODES];
    info->tris_tested = (long long)c[rtd::O_TRIS];
    info->stack_overflows = (long long)c[rtd::O_ERR];
    return query_finish(ctx, rtq::OVERLAPS, "rt_get_overlaps_info", c[rtd::O_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- sweep queries (rt_sweep.hpp)
extern "C" int rt_sweep_spheres(rt_ctx* ctx, const rt_spheres* r, const rt_sweep_results* out) {
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::SWEEP, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::SWEEP, r->kernel, r->n, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->centre || !r->motion || !r->radius))
        return arg_err(ctx, "rt_sweep_spheres: null centre / motion / radius");
    if (r->n > 0 && !out->tri && !out->t && !out->point)
        return arg_err(ctx, "rt_sweep_spheres: needs a tri, a t or a point output");
    rtd::SWArgs A;
    if (int rc = query_begin(ctx, rtq::SWEEP, rtd::SW_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.centre = r->centre;
    A.motion = r->motion;
    A.radius = r->radius;
    A.t_max = r->t_max;
    A.tri = out->tri;
    A.t = out->t;
    A.out = out->point;
    A.n = r->n;
    A.c_max = std::ldexp(ctx->scene_mx, 20);  // rtd::sweep_domain
    void (*k)(rtd::SWArgs) = r->kernel == RT_KERNEL_STRICT ? rtd::k_sweep<true> : rtd::k_sweep<false>;
    return query_launch(ctx, rtq::SWEEP, k, A);
}

extern "C" int rt_get_sweep_info(rt_ctx* ctx, rt_sweep_info* info) {
    unsigned long long c[rtd::SW_NCOUNT];
    if (int rc = query_read(ctx, rtq::SWEEP, "rt_get_sweep_info: no sweep query run", c, info)) return rc;
    info->spheres = (long long)c[rtd::SW_SPHERES];
    info->found = (long long)c[rtd::SW_FOUND];
    info->empty_spheres = (long long)c[rtd::SW_EMPTY];
    info->walked_spheres = (long long)c[rtd::SW_WALKED];
    info->exhaustive_spheres = (long long)c[rtd::SW_EXH];
    info->nodes_visited = (long long)c[rtd::SW_NODES];
    info->tris_tested = (long long)c[rtd::SW_TRIS];
    info->stack_overflows = (long long)c[rtd::SW_ERR];
    return query_finish(ctx, rtq::SWEEP, "rt_get_sweep_info", c[rtd::SW_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- contact queries (rt_contacts.hpp)
extern "C" int rt_sweep_contacts(rt_ctx* ctx, const rt_sphere_contacts* r, const rt_contact_results* out) {
    static_assert(RT_CONTACTS_MAX == rtd::CONTACTS_MAX && RT_CONTACTS_MAX == rtq::LIST_MAX,
                  "rt_hip.h, rt_contacts.hpp and rt_query_logic.hpp must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::CONTACTS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::CONTACTS, r->kernel, r->n, r->max_tris, r->count_all, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->centre || !r->motion || !r->radius))
        return arg_err(ctx, "rt_sweep_contacts: null centre / motion / radius");
    if (r->n > 0 && r->max_tris > 0 && !out->tri && !out->t && !out->point)
        return arg_err(ctx, "rt_sweep_contacts: max_tris > 0 needs a tri, a t or a point output");
    if (int rc = rtq::check_count_out(rtq::CONTACTS, r->n, r->max_tris, out->count != nullptr, ctx->err)) return rc;
    rtd::CArgs A;
    if (int rc = query_begin(ctx, rtq::CONTACTS, rtd::CT_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    const bool want_p = r->max_tris > 0 && out->point;
    if (want_p)
        if (int rc = ensure_ref_inv(ctx)) return rc;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.centre = r->centre;
    A.motion = r->motion;
    A.radius = r->radius;
    A.t_max = r->t_max;
    A.tri = r->max_tris > 0 ? out->tri : nullptr;
    A.t = r->max_tris > 0 ? out->t : nullptr;
    A.out = want_p ? out->point : nullptr;
    A.count = out->count;
    A.ref_inv = ctx->d_ref_inv;
    A.n = r->n;
    A.c_max = std::ldexp(ctx->scene_mx, 20);  // rtd::sweep_domain
    A.max_tris = r->max_tris;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::CONTACTS, FOR_LIST_CAP(r->max_tris, r->kernel == RT_KERNEL_STRICT, rtd::k_contacts),
                        A);
}

extern "C" int rt_get_contacts_info(rt_ctx* ctx, rt_contacts_info* info) {
    unsigned long long c[rtd::CT_NCOUNT];
    if (int rc = query_read(ctx, rtq::CONTACTS, "rt_get_contacts_info: no contacts query run", c, info)) return rc;
    info->spheres = (long long)c[rtd::CT_SPHERES];
    info->found = (long long)c[rtd::CT_FOUND];
    info->tris_stored = (long long)c[rtd::CT_STORED];
    info->tris_counted = (long long)c[rtd::CT_COUNTED];
    info->walked_spheres = (long long)c[rtd::CT_WALKED];
    info->exhaustive_spheres = (long long)c[rtd::CT_EXH];
    info->empty_spheres = (long long)c[rtd::CT_EMPTY];
    info->nodes_visited = (long long)c[rtd::CT_NODES];
    info->tris_tested = (long long)c[rtd::CT_TRIS];
    info->stack_overflows = (long long)c[rtd::CT_ERR];
    return query_finish(ctx, rtq::CONTACTS, "rt_get_contacts_info", c[rtd::CT_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- cut queries (rt_cut.hpp)
extern "C" int rt_cut_triangles(rt_ctx* ctx, const rt_tris* r, const rt_cut_results* out) {
    static_assert(RT_CUTS_MAX == rtd::CUTS_MAX && rtd::CUTS_MAX == rtd::OVERLAPS_MAX,
                  "rt_hip.h, rt_cut.hpp and the capacities of rt_overlap.hpp's OState must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::CUTS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::CUTS, r->kernel, r->n, r->max_tris, r->count_all, ctx->err)) return rc;
    if ((r->offsets != nullptr) != (out->list != nullptr))
        return arg_err(ctx, "rt_cut_triangles: offsets and list are given together or not at all");
    if (out->list_seg && !out->list) return arg_err(ctx, "rt_cut_triangles: list_seg needs a list");
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && !r->tris) return arg_err(ctx, "rt_cut_triangles: null tris");
    if (r->n > 0 && r->max_tris > 0 && !out->tri) return arg_err(ctx, "rt_cut_triangles: max_tris > 0 needs a tri output");
    if (int rc = rtq::check_count_out(rtq::CUTS, r->n, r->max_tris, out->count != nullptr, ctx->err)) return rc;
    rtd::XArgs A;
    if (int rc = query_begin(ctx, rtq::CUTS, rtd::X_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.tris = r->tris;
    A.offsets = r->offsets;
    A.tri = r->max_tris > 0 ? out->tri : nullptr;
    A.count = out->count;
    A.list = out->list;
    A.list_seg = out->list_seg;
    A.n = r->n;
    A.max_tris = r->max_tris;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::CUTS, FOR_LIST_CAP(r->max_tris, r->kernel == RT_KERNEL_STRICT, rtd::k_cut), A);
}

extern "C" int rt_get_cuts_info(rt_ctx* ctx, rt_cuts_info* info) {
    unsigned long long c[rtd::X_NCOUNT];
    if (int rc = query_read(ctx, rtq::CUTS, "rt_get_cuts_info: no cut query run", c, info)) return rc;
    info->triangles = (long long)c[rtd::X_TRIS];
    info->found = (long long)c[rtd::X_FOUND];
    info->stored = (long long)c[rtd::X_STORED];
    info->counted = (long long)c[rtd::X_COUNTED];
    info->listed = (long long)c[rtd::X_LISTED];
    info->walked = (long long)c[rtd::X_WALKED];
    info->exhaustive = (long long)c[rtd::X_EXH];
    info->empty = (long long)c[rtd::X_EMPTY];
    info->nodes_visited = (long long)c[rtd::X_NODES];
    info->pairs_tested = (long long)c[rtd::X_PAIRS];
    info->stack_overflows = (long long)c[rtd::X_ERR];
    return query_finish(ctx, rtq::CUTS, "rt_get_cuts_info", c[rtd::X_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- clearance queries (rt_clearance.hpp)
extern "C" int rt_clearance_triangles(rt_ctx* ctx, const rt_clear_tris* r, const rt_clearance_results* out) {
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::CLEARANCE, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::CLEARANCE, r->kernel, r->n, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && !r->tris) return arg_err(ctx, "rt_clearance_triangles: null tris");
    if (r->n > 0 && !out->tri && !out->d2 && !out->on_query && !out->on_mesh && !out->kind)
        return arg_err(ctx, "rt_clearance_triangles: needs a tri, a d2, an on_query, an on_mesh or a kind output");
    rtd::CLArgs A;
    if (int rc = query_begin(ctx, rtq::CLEARANCE, rtd::CL_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.tris = r->tris;
    A.max_dist2 = r->max_dist2;
    A.tri = out->tri;
    A.d2 = out->d2;
    A.on_query = out->on_query;
    A.on_mesh = out->on_mesh;
    A.kind = out->kind;
    A.n = r->n;
    void (*k)(rtd::CLArgs) = r->kernel == RT_KERNEL_STRICT ? rtd::k_clearance<true> : rtd::k_clearance<false>;
    return query_launch(ctx, rtq::CLEARANCE, k, A);
}

extern "C" int rt_get_clearance_info(rt_ctx* ctx, rt_clearance_info* info) {
    unsigned long long c[rtd::CL_NCOUNT];
    if (int rc = query_read(ctx, rtq::CLEARANCE, "rt_get_clearance_info: no clearance query run", c, info)) return rc;
    info->triangles = (long long)c[rtd::CL_TRIS];
    info->found = (long long)c[rtd::CL_FOUND];
    info->walked = (long long)c[rtd::CL_WALKED];
    info->exhaustive = (long long)c[rtd::CL_EXH];
    info->empty = (long long)c[rtd::CL_EMPTY];
    info->nodes_visited = (long long)c[rtd::CL_NODES];
    info->pairs_gated = (long long)c[rtd::CL_GATED];
    info->pairs_tested = (long long)c[rtd::CL_PAIRS];
    info->stack_overflows = (long long)c[rtd::CL_ERR];
    return query_finish(ctx, rtq::CLEARANCE, "rt_get_clearance_info", c[rtd::CL_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- proximity queries (rt_proximity.hpp)
extern "C" int rt_proximity_triangles(rt_ctx* ctx, const rt_prox_tris* r, const rt_proximity_results* out) {
    static_assert(RT_PROXIMITY_MAX == rtd::PROXIMITY_MAX && RT_PROXIMITY_MAX == rtq::LIST_MAX,
                  "rt_hip.h, rt_proximity.hpp and rt_query_logic.hpp must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::PROXIMITY, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::PROXIMITY, r->kernel, r->n, r->max_tris, r->count_all, ctx->err)) return rc;
    if ((r->offsets != nullptr) != (out->list != nullptr))
        return arg_err(ctx, "rt_proximity_triangles: offsets and list are given together or not at all");
    if ((out->list_d2 || out->list_points || out->list_kind) && !out->list)
        return arg_err(ctx, "rt_proximity_triangles: list_d2, list_points and list_kind need a list");
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && !r->tris) return arg_err(ctx, "rt_proximity_triangles: null tris");
    if (r->n > 0 && r->max_tris > 0 && !out->tri && !out->d2 && !out->on_query && !out->on_mesh && !out->kind)
        return arg_err(ctx,
                       "rt_proximity_triangles: max_tris > 0 needs a tri, a d2, an on_query, an on_mesh or a kind output");
    if (int rc = rtq::check_count_out(rtq::PROXIMITY, r->n, r->max_tris, out->count != nullptr, ctx->err)) return rc;
    rtd::PXArgs A;
    if (int rc = query_begin(ctx, rtq::PROXIMITY, rtd::PX_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    const bool lists = r->max_tris > 0;
    if (lists && (out->on_query || out->on_mesh || out->kind))
        if (int rc = ensure_ref_inv(ctx)) return rc;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.tris = r->tris;
    A.max_dist2 = r->max_dist2;
    A.offsets = r->offsets;
    A.tri = lists ? out->tri : nullptr;
    A.d2 = lists ? out->d2 : nullptr;
    A.on_query = lists ? out->on_query : nullptr;
    A.on_mesh = lists ? out->on_mesh : nullptr;
    A.kind = lists ? out->kind : nullptr;
    A.count = out->count;
    A.list = out->list;
    A.list_d2 = out->list_d2;
    A.list_points = out->list_points;
    A.list_kind = out->list_kind;
    A.ref_inv = ctx->d_ref_inv;
    A.n = r->n;
    A.max_tris = r->max_tris;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::PROXIMITY,
                        FOR_LIST_CAP(r->max_tris, r->kernel == RT_KERNEL_STRICT, rtd::k_proximity), A);
}

extern "C" int rt_get_proximity_info(rt_ctx* ctx, rt_proximity_info* info) {
    unsigned long long c[rtd::PX_NCOUNT];
    if (int rc = query_read(ctx, rtq::PROXIMITY, "rt_get_proximity_info: no proximity query run", c, info)) return rc;
    info->triangles = (long long)c[rtd::PX_TRIS];
    info->found = (long long)c[rtd::PX_FOUND];
    info->stored = (long long)c[rtd::PX_STORED];
    info->counted = (long long)c[rtd::PX_COUNTED];
    info->listed = (long long)c[rtd::PX_LISTED];
    info->walked = (long long)c[rtd::PX_WALKED];
    info->exhaustive = (long long)c[rtd::PX_EXH];
    info->empty = (long long)c[rtd::PX_EMPTY];
    info->nodes_visited = (long long)c[rtd::PX_NODES];
    info->pairs_gated = (long long)c[rtd::PX_GATED];
    info->pairs_tested = (long long)c[rtd::PX_PAIRS];
    info->stack_overflows = (long long)c[rtd::PX_ERR];
    return query_finish(ctx, rtq::PROXIMITY, "rt_get_proximity_info", c[rtd::PX_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- triangle sweep queries (rt_trisweep.hpp)
extern "C" int rt_sweep_triangles(rt_ctx* ctx, const rt_sweep_tris* r, const rt_trisweep_results* out) {
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::TRISWEEP, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::TRISWEEP, r->kernel, r->n, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->tris || !r->motion)) return arg_err(ctx, "rt_sweep_triangles: null tris / motion");
    if (r->n > 0 && !out->tri && !out->t && !out->point && !out->kind)
        return arg_err(ctx, "rt_sweep_triangles: needs a tri, a t, a point or a kind output");
    rtd::TSArgs A;
    if (int rc = query_begin(ctx, rtq::TRISWEEP, rtd::TS_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.tris = r->tris;
    A.motion = r->motion;
    A.t_max = r->t_max;
    A.tri = out->tri;
    A.t = out->t;
    A.out = out->point;
    A.kind = out->kind;
    A.n = r->n;
    A.c_max = std::ldexp(ctx->scene_mx, 20);  // rtd::tsw_domain
    void (*k)(rtd::TSArgs) = r->kernel == RT_KERNEL_STRICT ? rtd::k_trisweep<true> : rtd::k_trisweep<false>;
    return query_launch(ctx, rtq::TRISWEEP, k, A);
}

extern "C" int rt_get_trisweep_info(rt_ctx* ctx, rt_trisweep_info* info) {
    unsigned long long c[rtd::TS_NCOUNT];
    if (int rc = query_read(ctx, rtq::TRISWEEP, "rt_get_trisweep_info: no triangle sweep query run", c, info)) return rc;
    info->triangles = (long long)c[rtd::TS_TRIS];
    info->found = (long long)c[rtd::TS_FOUND];
    info->empty = (long long)c[rtd::TS_EMPTY];
    info->walked = (long long)c[rtd::TS_WALKED];
    info->exhaustive = (long long)c[rtd::TS_EXH];
    info->nodes_visited = (long long)c[rtd::TS_NODES];
    info->pairs_gated = (long long)c[rtd::TS_GATED];
    info->pairs_tested = (long long)c[rtd::TS_PAIRS];
    info->stack_overflows = (long long)c[rtd::TS_ERR];
    return query_finish(ctx, rtq::TRISWEEP, "rt_get_trisweep_info", c[rtd::TS_ERR], DEEP_WIDE, &info->kernel_ms);
}

// ---------------------------------------------------------------- triangle contact queries (rt_tricontacts.hpp)
extern "C" int rt_sweep_tri_contacts(rt_ctx* ctx, const rt_tri_contacts* r, const rt_tricontact_results* out) {
    static_assert(RT_TRICONTACTS_MAX == rtd::TRICONTACTS_MAX && RT_TRICONTACTS_MAX == rtq::LIST_MAX,
                  "rt_hip.h, rt_tricontacts.hpp and rt_query_logic.hpp must agree");
    if (!ctx) return RT_E_ARG;
    if (int rc = rtq::check_enter(rtq::TRICONTACTS, ctx->has_scene, r && out, ctx->err)) return rc;
    if (int rc = rtq::check_args(rtq::TRICONTACTS, r->kernel, r->n, r->max_tris, r->count_all, ctx->err)) return rc;
    // (n = 0 reads and writes nothing: empty arrays may have no address)
    if (r->n > 0 && (!r->tris || !r->motion)) return arg_err(ctx, "rt_sweep_tri_contacts: null tris / motion");
    if (r->n > 0 && r->max_tris > 0 && !out->tri && !out->t && !out->point && !out->kind)
        return arg_err(ctx, "rt_sweep_tri_contacts: max_tris > 0 needs a tri, a t, a point or a kind output");
    if (int rc = rtq::check_count_out(rtq::TRICONTACTS, r->n, r->max_tris, out->count != nullptr, ctx->err)) return rc;
    rtd::TCArgs A;
    if (int rc = query_begin(ctx, rtq::TRICONTACTS, rtd::TC_NCOUNT, A)) return rc;
    if (r->n == 0) return RT_OK;
    const bool lists = r->max_tris > 0;
    if (lists && (out->point || out->kind))
        if (int rc = ensure_ref_inv(ctx)) return rc;
    A.s = scene_args(ctx);  // (the full wide view only; without one the kernel runs its exhaustive loop)
    A.tris = r->tris;
    A.motion = r->motion;
    A.t_max = r->t_max;
    A.tri = lists ? out->tri : nullptr;
    A.t = lists ? out->t : nullptr;
    A.out = lists ? out->point : nullptr;
    A.kind = lists ? out->kind : nullptr;
    A.count = out->count;
    A.ref_inv = ctx->d_ref_inv;
    A.n = r->n;
    A.c_max = std::ldexp(ctx->scene_mx, 20);  // rtd::tsw_domain
    A.max_tris = r->max_tris;
    A.count_all = r->count_all;
    return query_launch(ctx, rtq::TRICONTACTS,
                        FOR_LIST_CAP(r->max_tris, r->kernel == RT_KERNEL_STRICT, rtd::k_tricontacts), A);
}

extern "C" int rt_get_tricontacts_info(rt_ctx* ctx, rt_tricontacts_info* info) {
    unsigned long long c[rtd::TC_NCOUNT];
    if (int rc = query_read(ctx, rtq::TRICONTACTS, "rt_get_tricontacts_info: no triangle contact query run", c, info))
        return rc;
    info->triangles = (long long)c[rtd::TC_TRIS];
    info->found = (long long)c[rtd::TC_FOUND];
    info->stored = (long long)c[rtd::TC_STORED];
    info->counted = (long long)c[rtd::TC_COUNTED];
    info->walked = (long long)c[rtd::TC_WALKED];
    info->exhaustive = (long long)c[rtd::TC_EXH];
    info->empty = (long long)c[rtd::TC_EMPTY];
    info->nodes_visited = (long long)c[rtd::TC_NODES];
    info->pairs_gated = (long long)c[rtd::TC_GATED];
    info->pairs_tested = (long long)c[rtd::TC_PAIRS];
    info->stack_overflows = (long long)c[rtd::TC_ERR];
    return query_finish(ctx, rtq::TRICONTACTS, "rt_get_tricontacts_info", c[rtd::TC_ERR], DEEP_WIDE, &info->kernel_ms);
}

namespace {
int comm_settle_ctx(rt_ctx* ctx, const char* who);  // (below, with the communicators)
// Waits for the context stream; with a render behind it, reads that render's error counter (rtd::C_ERR: a traversal
// stack overflowed, rt_kernels.hpp) in the same wait, so that a frame computed with a truncated walk never passes as
// good: RT_E_KERNEL. A stream holding a multi-process gather's send / recv group is first waited for through the
// communicator's bounded wait (comm_settle): a peer that never joins fails the call with RT_E_TIMEOUT instead of
// blocking in hipStreamSynchronize.
int sync_checked(rt_ctx* ctx, const char* who) {
    if (int rc = comm_settle_ctx(ctx, who)) return rc;
    if (ctx->rendered)
        HIPC(hipMemcpyAsync(ctx->h_err, ctx->d_counters + rtd::C_ERR, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                            ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    if (ctx->rendered && *ctx->h_err) {
        ctx->err = std::string(who) + ": the render's traversal stack overflowed " + std::to_string(*ctx->h_err) +
                   " times (BVH deeper than the walks' stacks): the frame is not valid";
        return RT_E_KERNEL;
    }
    return RT_OK;
}
}  // namespace

// The HIP-event time of render launch `launch` (one of the last NEV, finished). hipEventElapsedTime converts the pair's
// device ticks with a clock calibration the runtime refreshes as it goes, so two reads of the same finished pair can
// differ in the last digits (seen: 0.7003270 and 0.7003260 ms). rt_sync and rt_kernel_times report a launch's time as
// one value: the first read is kept until the slot's pair is recorded again.
static hipError_t launch_ms(rt_ctx* ctx, long long launch, float* ms) {
    const int slot = (int)(launch % rt_ctx::NEV);
    if (ctx->ms_launch[slot] != launch + 1) {
        float t = 0.0f;
        if (hipError_t e = hipEventElapsedTime(&t, ctx->ev0s[slot], ctx->ev1s[slot]); e != hipSuccess) return e;
        ctx->ms_of[slot] = t;
        ctx->ms_launch[slot] = launch + 1;
    }
    *ms = ctx->ms_of[slot];
    return hipSuccess;
}

extern "C" int rt_sync(rt_ctx* ctx, float* kernel_ms) {
    if (!ctx) return RT_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    if (int rc = sync_checked(ctx, "rt_sync")) return rc;
    if (kernel_ms) {
        *kernel_ms = 0.0f;
        if (ctx->rendered) HIPC(launch_ms(ctx, ctx->launches - 1, kernel_ms));
    }
    return RT_OK;
}

extern "C" int rt_kernel_times(rt_ctx* ctx, float* ms, int n) {
    if (!ctx || !ms || n < 0) return RT_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    if (int rc = comm_settle_ctx(ctx, "rt_kernel_times")) return rc;
    HIPC(hipStreamSynchronize(ctx->stream));
    long long avail = ctx->launches < rt_ctx::NEV ? ctx->launches : rt_ctx::NEV;
    if (n > avail) n = (int)avail;
    for (int i = 0; i < n; i++) {  // oldest first among the last n launches
        HIPC(launch_ms(ctx, ctx->launches - n + i, &ms[i]));
    }
    return n;
}

extern "C" int rt_download(rt_ctx* ctx, float* h_rgb, int* h_hit) {
    if (!ctx) return RT_E_ARG;
    if (!ctx->rendered) {
        ctx->err = "rt_download: nothing rendered";
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    if (int rc = sync_checked(ctx, "rt_download")) return rc;
    if (h_rgb && !ctx->last_rgb) {
        ctx->err = "rt_download: last frame was rendered to a bgra output only";
        return RT_E_STATE;
    }
    if (h_rgb)
        HIPC(hipMemcpy(h_rgb, ctx->last_rgb, sizeof(float) * 3 * ctx->last_pixels, hipMemcpyDeviceToHost));
    if (h_hit) {
        if (!ctx->last_hit) {
            ctx->err = "rt_download: last frame had no hit output";
            return RT_E_STATE;
        }
        HIPC(hipMemcpy(h_hit, ctx->last_hit, sizeof(int) * ctx->last_pixels, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

namespace {
template <class T>
int grow(rt_ctx* ctx, T** p, size_t& cap, size_t n) {
    if (*p && cap >= n) return RT_OK;
    if (*p) HIPC(hipFree(*p));
    *p = nullptr;
    cap = 0;
    HIPC(hipMalloc((void**)p, sizeof(T) * std::max<size_t>(n, 1)));
    cap = n;
    return RT_OK;
}
}  // namespace

namespace {
// a rank's part of a gathered frame batch, the layout checks (rt_comm_logic.hpp: host-only, unit-tested with g++)
using rtc::check_parts;
using rtc::Part;
using rtc::part_px;

Part part_of(const rt_ctx* c) {
    Part p{};
    p.W = c->last_W;
    p.H = c->last_H;
    p.frames = c->last_frames;
    p.rows = c->last_rows;
    p.off = c->last_off;
    p.stride = c->last_stride;
    p.block = c->last_block;
    p.shift = c->last_shift;
    p.words = c->last_bgra ? 1 : 3;
    p.hit = c->last_hit ? 1 : 0;
    return p;
}
const void* payload_of(const rt_ctx* c) { return c->last_bgra ? (const void*)c->last_bgra : (const void*)c->last_rgb; }

// compact part -> full frames on stream s (root's device)
int unshuffle(rt_ctx* ctx, const void* src, void* dst, const Part& p, int words, hipStream_t s) {
    const size_t n = part_px(p);
    if (!n) return RT_OK;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096));
    rtd::k_unshuffle_frames<<<grid, 256, 0, s>>>((const unsigned*)src, (unsigned*)dst, p.W, p.H, p.frames, p.rows,
                                                   p.off, p.stride, p.block, p.shift, words);
    HIPC(hipGetLastError());
    return RT_OK;
}

// the root's full frames (its own buffers unless the caller gave one); afterwards its last render IS them
int full_target(rt_ctx* ctx, const Part& a, void* user, void** dst, int** dst_hit, bool want_hit) {
    const size_t px = (size_t)a.frames * a.W * a.H;
    int rc;
    if (user) *dst = user;
    else if (a.words == 1) {
        if ((rc = grow(ctx, &ctx->d_full_bgra, ctx->full_bgra_cap, px))) return rc;
        *dst = ctx->d_full_bgra;
    } else {
        if ((rc = grow(ctx, &ctx->d_full, ctx->full_cap, 3 * px))) return rc;
        *dst = ctx->d_full;
    }
    *dst_hit = nullptr;
    if (want_hit) {
        if ((rc = grow(ctx, &ctx->d_full_hit, ctx->full_hit_cap, px))) return rc;
        *dst_hit = ctx->d_full_hit;
    }
    return RT_OK;
}

int finish_gather(rt_ctx* ctx, const Part& a, void* dst, int* dst_hit) {
    // the gather's completion has its own event: ev0s / ev1s stay the render launches' (rt_kernel_times)
    if (!ctx->gather_ev) HIPC(hipEventCreateWithFlags(&ctx->gather_ev, hipEventDisableTiming));
    HIPC(hipEventRecord(ctx->gather_ev, ctx->stream));
    ctx->last_rgb = a.words == 3 ? (float*)dst : nullptr;
    ctx->last_bgra = a.words == 1 ? (unsigned*)dst : nullptr;
    ctx->last_hit = dst_hit;
    ctx->last_pixels = (size_t)a.frames * a.W * a.H;
    ctx->last_off = 0;
    ctx->last_stride = 1;
    ctx->last_rows = a.H;
    ctx->last_block = 1;
    ctx->last_shift = 0;
    return RT_OK;
}
}  // namespace

extern "C" int rt_gather(rt_ctx* const* ctxs, int n, int root) { return rt_gather_to(ctxs, n, root, nullptr); }

extern "C" int rt_gather_to(rt_ctx* const* ctxs, int n, int root, void* d_dst) {
    if (!ctxs || n <= 0 || root < 0 || root >= n || !ctxs[root]) return RT_E_ARG;
    rt_ctx* ctx = ctxs[root];
    std::vector<Part> ps;
    bool all_hit = true;
    for (int i = 0; i < n; i++) {
        rt_ctx* c = ctxs[i];
        if (!c || !c->rendered) return arg_err(ctx, "rt_gather: a context has not rendered");
        ps.push_back(part_of(c));
        all_hit = all_hit && c->last_hit;
    }
    const std::string why = check_parts(ps);
    if (!why.empty()) return arg_err(ctx, ("rt_gather: " + why).c_str());
    const Part& a = ps[0];
    const int words = a.words;
    // staging on the root for the parts of other devices, in rank order: payload, then hit
    size_t stage = 0;
    for (int i = 0; i < n; i++)
        if (ctxs[i]->device != ctx->device) stage += part_px(ps[i]) * 4 * (words + (all_hit ? 1 : 0));
    HIPC(hipSetDevice(ctx->device));
    int rc;
    if (stage && (rc = grow(ctx, &ctx->d_stage, ctx->stage_cap, stage))) return rc;
    void* dst;
    int* dst_hit;
    if ((rc = full_target(ctx, a, d_dst, &dst, &dst_hit, all_hit))) return rc;
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        rt_ctx* c = ctxs[i];
        const size_t cpx = part_px(ps[i]);
        const void* src = payload_of(c);
        const int* src_hit = c->last_hit;
        if (c->device != ctx->device) {
            // xGMI peer copies issued on the SOURCE's stream (after its render; the copies of different sources
            // run on their own devices' engines at once), then the root waits for them
            void* d1 = ctx->d_stage + at;
            at += cpx * 4 * words;
            HIPC(hipSetDevice(c->device));
            // the root's staging area may still be read by the previous gather's un-interleaving (root stream):
            // the source's copy into it waits for that gather's completion (write after read)
            if (ctx->gather_ev) HIPC(hipStreamWaitEvent(c->stream, ctx->gather_ev, 0));
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, c->device, ctx->device);
            if (can) {  // direct xGMI copies (else the runtime stages through the host)
                const hipError_t e = hipDeviceEnablePeerAccess(ctx->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(ctx, e, "hipDeviceEnablePeerAccess");
                (void)hipGetLastError();
            }
            HIPC(hipMemcpyPeerAsync(d1, ctx->device, src, c->device, cpx * 4 * words, c->stream));
            src = d1;
            if (all_hit) {
                int* d2 = (int*)(ctx->d_stage + at);
                at += cpx * 4;
                HIPC(hipMemcpyPeerAsync(d2, ctx->device, src_hit, c->device, cpx * 4, c->stream));
                src_hit = d2;
            }
            if (!c->copy_ev) HIPC(hipEventCreateWithFlags(&c->copy_ev, hipEventDisableTiming));
            HIPC(hipEventRecord(c->copy_ev, c->stream));
            HIPC(hipSetDevice(ctx->device));
            HIPC(hipStreamWaitEvent(ctx->stream, c->copy_ev, 0));
        } else if (c != ctx) {
            HIPC(hipStreamWaitEvent(ctx->stream, c->ev1, 0));  // after the source's last render
        }
        if ((rc = unshuffle(ctx, src, dst, ps[i], words, ctx->stream))) return rc;
        if (all_hit && (rc = unshuffle(ctx, src_hit, dst_hit, ps[i], 1, ctx->stream))) return rc;
    }
    return finish_gather(ctx, a, dst, dst_hit);
}

// ---------------------------------------------------------------- RCCL communicator (rt_comm_*)
struct rt_comm {
    std::vector<rt_ctx*> ctxs;  // rt_comm_init: the local ranks rank0 .. rank0 + n - 1; rt_comm_init_rank: this rank's
    std::vector<int> devices;   // their devices
    std::vector<ncclComm_t> comms;
    int nranks = 0, rank0 = 0;
    bool multi = false;  // rt_comm_init_rank: one rank of a multi-process job (row sets exchanged over RCCL)
    // multi-process: the layout -- every rank's descriptor as last exchanged (ncclAllGather), and this rank's part
    // at that exchange. A gather exchanges again only on what every rank sees the same way (rtc::layout_step: the
    // first gather, a new frame size / count / pixel kind, or rt_comm_relayout on every rank).
    std::vector<Part> layout;
    Part mine{};
    bool have_layout = false;
    Part* d_desc = nullptr;  // every rank's descriptor (ncclAllGather) + this rank's staging slot, on its device
    Part* h_desc = nullptr;  // pinned
    unsigned long long* d_count = nullptr;  // the root's coverage check of a layout's first gather
    hipStream_t side = nullptr;  // the exchange's stream: the host waits for the exchange only, not for renders
    hipEvent_t done = nullptr;   // after the last send / recv group: the next operation on the communicator waits
    bool issued = false;
    // the issued send / recv groups not yet seen complete, oldest first: `pre` recorded on the source's stream before
    // the group (after its render: the group's local part), `done` after it (rtc::settle: the deadline covers the
    // collective, not the render before it); events reused from ev_pool
    struct Pending {
        hipEvent_t pre, done;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
    std::shared_ptr<CommLink> link = std::make_shared<CommLink>();
    bool aborted = false;     // a collective missed its deadline: the communicator was aborted (ncclCommAbort)
    double timeout_s = 120.0;  // host waits on a collective (rt_comm_set_timeout)
    rt_comm_info info{};
    std::string err;
};

namespace {
// RCCL is opened on first use (dlopen of librccl.so.1), not linked: a process that never builds a communicator
// never loads it, and one that already has it (torch.distributed's RCCL) gets that same library (matched by
// soname) instead of a second copy next to it.
struct Rccl {
    bool tried = false, ok = false;
    std::string why;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl& rccl() {
    static Rccl R;
    if (R.tried) return R;
    R.tried = true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        R.why = std::string("cannot load librccl.so.1: ") + dlerror();
        return R;
    }
    bool all = true;
    auto sym = [&](auto& fp, const char* name) {
        fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name));
        if (!fp) all = false;
    };
    sym(R.GetUniqueId, "ncclGetUniqueId");
    sym(R.CommInitAll, "ncclCommInitAll");
    sym(R.CommInitRank, "ncclCommInitRank");
    sym(R.CommDestroy, "ncclCommDestroy");
    sym(R.CommAbort, "ncclCommAbort");
    sym(R.AllGather, "ncclAllGather");
    sym(R.Send, "ncclSend");
    sym(R.Recv, "ncclRecv");
    sym(R.GroupStart, "ncclGroupStart");
    sym(R.GroupEnd, "ncclGroupEnd");
    sym(R.GetErrorString, "ncclGetErrorString");
    R.ok = all;
    if (!all) R.why = "librccl.so.1 lacks a symbol";
    return R;
}

int comm_fail(rt_comm* cm, ncclResult_t r, const char* what) {
    cm->err = std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error");
    if (!cm->ctxs.empty() && cm->ctxs[0]) cm->ctxs[0]->err = cm->err;  // (null: that context was destroyed)
    return RT_E_HIP;
}
int comm_arg(rt_comm* cm, const std::string& what) {
    cm->err = what;
    for (rt_ctx* c : cm->ctxs)
        if (c) c->err = what;
    return RT_E_ARG;
}
#define NCCLC(call)                                       \
    do {                                                  \
        ncclResult_t r_ = (call);                         \
        if (r_ != ncclSuccess) return comm_fail(cm, r_, #call); \
    } while (0)

// A collective that misses its deadline: every RCCL communicator of `cm` is aborted (its kernels stop waiting for
// the missing peer, so the streams drain), and the communicator refuses further gathers.
int comm_abort(rt_comm* cm, const std::string& what) {
    for (size_t l = 0; l < cm->comms.size(); l++)
        if (cm->comms[l]) {
            (void)hipSetDevice(cm->devices[l]);
            (void)rccl().CommAbort(cm->comms[l]);
            cm->comms[l] = nullptr;
        }
    cm->aborted = true;
    cm->err = what;
    for (rt_ctx* c : cm->ctxs)
        if (c) c->err = what;
    // (the aborted groups' kernels stop waiting, the streams drain: nothing outstanding is waited for again)
    for (const rt_comm::Pending& p : cm->pending) {
        cm->ev_pool.push_back(p.pre);
        cm->ev_pool.push_back(p.done);
    }
    cm->pending.clear();
    return RT_E_TIMEOUT;
}
// A host wait on work behind a collective (a stream or an event), bounded by the communicator's timeout
// (rtc::bounded_wait): RT_E_TIMEOUT and an aborted communicator instead of a hang when a peer never arrives.
template <class Q>
int comm_wait(rt_comm* cm, Q query_hip, const char* what) {
    int err = 0;
    const rtc::Wait w = rtc::bounded_wait(
        [&]() -> int {
            const hipError_t e = query_hip();
            if (e == hipSuccess) return 0;
            if (e == hipErrorNotReady) {
                (void)hipGetLastError();  // not an error: still running
                return 1;
            }
            return -(int)e;
        },
        cm->timeout_s, err);
    if (w == rtc::Wait::Done) return RT_OK;
    if (w == rtc::Wait::Error) {
        cm->err = std::string(what) + ": " + hipGetErrorString((hipError_t)(-err));
        for (rt_ctx* c : cm->ctxs)
            if (c) c->err = cm->err;
        return RT_E_HIP;
    }
    return comm_abort(cm, std::string(what) + ": no completion within " + std::to_string(cm->timeout_s) +
                              " s (a peer rank never joined the collective); the communicator is aborted");
}

int event_state(hipEvent_t e) {  // rtc query convention: 0 complete, 1 not yet, < 0 -(hipError_t)
    const hipError_t q = hipEventQuery(e);
    if (q == hipSuccess) return 0;
    if (q == hipErrorNotReady) {
        (void)hipGetLastError();  // not an error: still running
        return 1;
    }
    return -(int)q;
}

// Waits for every outstanding send / recv group of a multi-process communicator, in issue order (rtc::settle): each
// group's render without a deadline, its collective within the communicator's timeout from the moment that render has
// completed. RT_E_TIMEOUT (the communicator aborted) when a peer never joins.
int comm_settle(rt_comm* cm, const char* what) {
    if (cm->aborted) {
        cm->err = std::string(what) + ": the communicator was aborted";
        return RT_E_TIMEOUT;
    }
    if (cm->pending.empty()) return RT_OK;
    (void)hipSetDevice(cm->devices[0]);
    int err = 0, n_done = 0;
    const rtc::Wait w = rtc::settle((int)cm->pending.size(), [&](int j) { return event_state(cm->pending[j].pre); },
                                    [&](int j) { return event_state(cm->pending[j].done); }, cm->timeout_s, err, n_done);
    for (int j = 0; j < n_done; j++) {
        cm->ev_pool.push_back(cm->pending[j].pre);
        cm->ev_pool.push_back(cm->pending[j].done);
    }
    cm->pending.erase(cm->pending.begin(), cm->pending.begin() + n_done);
    if (w == rtc::Wait::Done) return RT_OK;
    if (w == rtc::Wait::Error) {
        cm->err = std::string(what) + ": " + hipGetErrorString((hipError_t)(-err));
        for (rt_ctx* c : cm->ctxs)
            if (c) c->err = cm->err;
        return RT_E_HIP;
    }
    return comm_abort(cm, std::string(what) + ": a gather's collective did not complete within " +
                              std::to_string(cm->timeout_s) +
                              " s of its render (a peer rank never joined it); the communicator is aborted");
}
// the same for a context whose stream holds a group (sync_checked, rt_kernel_times, rt_destroy)
int comm_settle_ctx(rt_ctx* ctx, const char* who) {
    if (!ctx->comm_link || !ctx->comm_link->cm) return RT_OK;
    rt_comm* cm = ctx->comm_link->cm;
    if (cm->aborted) return RT_OK;  // (aborted: its groups no longer block the stream)
    const int rc = comm_settle(cm, who);
    (void)hipSetDevice(ctx->device);
    if (rc) ctx->err = cm->err;
    return rc;
}
// completed groups off the front of the list, without waiting (each gather: the list stays short)
void comm_prune(rt_comm* cm) {
    size_t k = 0;
    while (k < cm->pending.size() && event_state(cm->pending[k].done) == 0) {
        cm->ev_pool.push_back(cm->pending[k].pre);
        cm->ev_pool.push_back(cm->pending[k].done);
        k++;
    }
    cm->pending.erase(cm->pending.begin(), cm->pending.begin() + k);
}
hipError_t comm_event(rt_comm* cm, hipEvent_t* e) {
    if (!cm->ev_pool.empty()) {
        *e = cm->ev_pool.back();
        cm->ev_pool.pop_back();
        return hipSuccess;
    }
    return hipEventCreateWithFlags(e, hipEventDisableTiming);
}
}  // namespace

extern "C" int rt_comm_get_id(unsigned char* id) {
    if (!id) return RT_E_ARG;
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "ncclUniqueId size");
    if (!rccl().ok) return RT_E_STATE;
    ncclUniqueId u;
    if (rccl().GetUniqueId(&u) != ncclSuccess) return RT_E_HIP;
    std::memcpy(id, &u, sizeof u);
    return RT_OK;
}

extern "C" int rt_comm_init(rt_ctx* const* ctxs, int n, rt_comm** out) {
    if (!ctxs || n <= 0 || !out) return RT_E_ARG;
    *out = nullptr;
    std::vector<int> devs;
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return RT_E_ARG;
        for (int d : devs)
            if (d == ctxs[i]->device) {
                ctxs[i]->err = "rt_comm_init: RCCL takes one rank per device (two contexts share a device: use rt_gather)";
                return RT_E_ARG;
            }
        devs.push_back(ctxs[i]->device);
    }
    if (!rccl().ok) {
        ctxs[0]->err = "rt_comm_init: " + rccl().why;
        return RT_E_STATE;
    }
    rt_comm* cm = new rt_comm;
    cm->ctxs.assign(ctxs, ctxs + n);
    cm->devices = devs;
    cm->comms.resize(n);
    cm->nranks = n;
    cm->info.nranks = n;
    const ncclResult_t r = rccl().CommInitAll(cm->comms.data(), n, devs.data());
    if (r != ncclSuccess) {
        comm_fail(cm, r, "ncclCommInitAll");
        delete cm;
        return RT_E_HIP;
    }
    *out = cm;
    return RT_OK;
}

extern "C" int rt_comm_init_rank(rt_ctx* ctx, int nranks, int rank, const unsigned char* id, rt_comm** out) {
    if (!ctx || !id || !out || nranks <= 0 || rank < 0 || rank >= nranks) return RT_E_ARG;
    *out = nullptr;
    if (!rccl().ok) {
        ctx->err = "rt_comm_init_rank: " + rccl().why;
        return RT_E_STATE;
    }
    HIPC(hipSetDevice(ctx->device));
    rt_comm* cm = new rt_comm;
    cm->ctxs = {ctx};
    cm->devices = {ctx->device};
    cm->comms.resize(1);
    cm->nranks = nranks;
    cm->rank0 = rank;
    cm->multi = true;
    cm->info.nranks = nranks;
    cm->info.rank = rank;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    ncclResult_t r = rccl().CommInitRank(&cm->comms[0], nranks, u, rank);
    if (r != ncclSuccess) {
        comm_fail(cm, r, "ncclCommInitRank");
        delete cm;
        return RT_E_HIP;
    }
    hipError_t e = hipMalloc((void**)&cm->d_desc, sizeof(Part) * (nranks + 1));
    if (e == hipSuccess) e = hipHostMalloc((void**)&cm->h_desc, sizeof(Part) * (nranks + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&cm->d_count, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&cm->side, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&cm->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        fail(ctx, e, "rt_comm_init_rank: descriptor buffers");
        rt_comm_destroy(cm);
        return RT_E_HIP;
    }
    *out = cm;
    return RT_OK;
}

namespace {
// The multi-process gather: `src` (a context of this rank on the communicator's device) sends its last render to
// the root. One communicator serves every context of the rank (bench.py alternates two on two streams): each
// gather's send / recv group runs on its source's stream (so after that render) and after the previous group on
// the communicator (an event), so every rank runs the communicator's operations in one order.
int comm_gather_multi(rt_comm* cm, rt_ctx* src, int root, void* d_dst) {
    rt_ctx* ctx = src;
    HIPC(hipSetDevice(ctx->device));
    if (cm->aborted) return comm_arg(cm, "rt_comm_gather: the communicator was aborted (" + cm->err + ")");
    // this rank's part; a rank whose context has not rendered still takes part (W = 0), so that every rank fails
    // together in check_parts instead of the others waiting in the collective for it
    const Part mine = ctx->rendered ? part_of(ctx) : Part{};
    const rtc::Step step = rtc::layout_step(mine, cm->mine, cm->have_layout);
    if (step == rtc::Step::RowsChanged)  // (refused before any collective call: the peers' next wait times out)
        return comm_arg(cm, "rt_comm_gather: this rank's rows changed without a layout change every rank sees "
                            "(frame size, frame count, pixel kind): call rt_comm_relayout on every rank first");
    const bool fresh = step == rtc::Step::Exchange;
    if (fresh) {  // a new layout: exchange the 64-B descriptors (ncclAllGather) and check that they partition the frames
        // (the groups before it first: their renders unbounded, their collectives bounded -- the exchange's own
        // deadline then covers the AllGather only)
        if (int rc = comm_settle(cm, "rt_comm_gather: the gathers before a row-set exchange")) return rc;
        cm->h_desc[cm->nranks] = mine;
        if (cm->issued) HIPC(hipStreamWaitEvent(cm->side, cm->done, 0));
        HIPC(hipMemcpyAsync(cm->d_desc + cm->nranks, cm->h_desc + cm->nranks, sizeof(Part), hipMemcpyHostToDevice, cm->side));
        NCCLC(rccl().AllGather(cm->d_desc + cm->nranks, cm->d_desc, sizeof(Part) / 4, ncclInt32, cm->comms[0], cm->side));
        HIPC(hipMemcpyAsync(cm->h_desc, cm->d_desc, sizeof(Part) * cm->nranks, hipMemcpyDeviceToHost, cm->side));
        if (int rc = comm_wait(cm, [&] { return hipStreamQuery(cm->side); }, "rt_comm_gather: row-set exchange"))
            return rc;
        cm->info.exchanges++;
        cm->layout.assign(cm->h_desc, cm->h_desc + cm->nranks);
        cm->have_layout = false;
        const std::string why = check_parts(cm->layout);
        if (!why.empty()) return comm_arg(cm, "rt_comm_gather: " + why);
        cm->mine = mine;
        cm->have_layout = true;
    }
    const std::vector<Part>& ps = cm->layout;
    const Part& a = ps[0];
    const int words = a.words;
    const bool is_root = cm->rank0 == root;
    std::vector<size_t> at(cm->nranks, 0);
    void* dst = nullptr;
    int* dst_hit = nullptr;
    if (is_root) {
        size_t stage = 0;
        for (int q = 0; q < cm->nranks; q++) {
            at[q] = stage;
            if (q != root) stage += part_px(ps[q]) * 4 * words;
        }
        int rc;
        if (stage && (rc = grow(ctx, &ctx->d_stage, ctx->stage_cap, stage))) return rc;
        if ((rc = full_target(ctx, a, d_dst, &dst, &dst_hit, false))) return rc;
    }
    if (cm->issued) HIPC(hipStreamWaitEvent(ctx->stream, cm->done, 0));
    const size_t full_px = (size_t)a.frames * a.W * a.H;
    if (is_root && fresh)  // coverage check of a layout's first gather: no render writes this value (k_count_unwritten)
        HIPC(hipMemsetAsync(dst, words == 1 ? 0 : 0xFF, full_px * 4 * words, ctx->stream));
    comm_prune(cm);
    rt_comm::Pending pend{};
    HIPC(comm_event(cm, &pend.pre));
    if (hipError_t e = comm_event(cm, &pend.done); e != hipSuccess) {
        cm->ev_pool.push_back(pend.pre);
        return fail(ctx, e, "rt_comm_gather: events");
    }
    cm->ev_pool.push_back(pend.pre);  // (back to the pool unless the group is issued below)
    cm->ev_pool.push_back(pend.done);
    HIPC(hipEventRecord(pend.pre, ctx->stream));  // the group's local part (the render) ends here
    NCCLC(rccl().GroupStart());
    if (!is_root) {
        NCCLC(rccl().Send(payload_of(ctx), part_px(ps[cm->rank0]) * words, ncclUint32, root, cm->comms[0], ctx->stream));
    } else {
        for (int q = 0; q < cm->nranks; q++)
            if (q != root)
                NCCLC(rccl().Recv(ctx->d_stage + at[q], part_px(ps[q]) * words, ncclUint32, q, cm->comms[0], ctx->stream));
    }
    NCCLC(rccl().GroupEnd());
    HIPC(hipEventRecord(cm->done, ctx->stream));
    cm->ev_pool.pop_back();
    cm->ev_pool.pop_back();
    HIPC(hipEventRecord(pend.done, ctx->stream));
    cm->pending.push_back(pend);
    ctx->comm_link = cm->link;
    cm->issued = true;
    cm->info.gathers++;
    if (!is_root) return RT_OK;
    int rc;
    for (int q = 0; q < cm->nranks; q++) {
        const void* s = q == root ? payload_of(ctx) : (const void*)(ctx->d_stage + at[q]);
        if ((rc = unshuffle(ctx, s, dst, ps[q], words, ctx->stream))) return rc;
    }
    if ((rc = finish_gather(ctx, a, dst, dst_hit))) return rc;
    if (fresh) {  // the layout's first gather, checked pixel by pixel on the root (once per layout: a host wait)
        unsigned long long left = 0;
        HIPC(hipMemsetAsync(cm->d_count, 0, sizeof left, ctx->stream));
        const int grid = (int)std::max<size_t>(1, std::min<size_t>((full_px + 255) / 256, 4096));
        rtd::k_count_unwritten<<<grid, 256, 0, ctx->stream>>>((const unsigned*)dst, full_px, words, cm->d_count);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(&left, cm->d_count, sizeof left, hipMemcpyDeviceToHost, ctx->stream));
        // the group (its render unbounded, its collective bounded), then the local unshuffle and count behind it
        if (int rc2 = comm_settle(cm, "rt_comm_gather: coverage check")) return rc2;
        if (int rc2 = comm_wait(cm, [&] { return hipStreamQuery(ctx->stream); }, "rt_comm_gather: coverage check"))
            return rc2;
        cm->info.checked++;
        if (left)  // (the layout stays: every rank keeps the same view of it, so the next gathers stay matched)
            return comm_arg(cm, "rt_comm_gather: the gathered frames miss " + std::to_string(left) + " pixels");
    }
    return RT_OK;
}
}  // namespace

extern "C" int rt_comm_gather_from(rt_comm* cm, rt_ctx* src, int root, void* d_dst) {
    if (!cm || root < 0 || root >= cm->nranks) return RT_E_ARG;
    if (cm->multi) {
        if (!src) src = cm->ctxs[0];
        if (!src) return comm_arg(cm, "rt_comm_gather_from: the communicator's context was destroyed");
        if (src->device != cm->devices[0])
            return comm_arg(cm, "rt_comm_gather_from: the context is not on the communicator's device");
        return comm_gather_multi(cm, src, root, d_dst);
    }
    if (src && src != cm->ctxs[0]) return comm_arg(cm, "rt_comm_gather_from: a one-process communicator gathers its own contexts");
    const int nl = (int)cm->ctxs.size();
    // one process: every rank's descriptor at hand
    std::vector<Part> ps(cm->nranks);
    for (rt_ctx* c : cm->ctxs)
        if (!c || !c->rendered) return comm_arg(cm, "rt_comm_gather: a context has not rendered (or was destroyed)");
    for (int i = 0; i < nl; i++) ps[i] = part_of(cm->ctxs[i]);
    const std::string why = check_parts(ps);
    if (!why.empty()) return comm_arg(cm, "rt_comm_gather: " + why);
    const Part& a = ps[0];
    const int words = a.words;
    rt_ctx* rctx = cm->ctxs[root];
    std::vector<size_t> at(cm->nranks, 0);
    void* dst = nullptr;
    int* dst_hit = nullptr;
    {
        rt_ctx* ctx = rctx;
        size_t stage = 0;
        for (int q = 0; q < cm->nranks; q++) {
            at[q] = stage;
            if (q != root) stage += part_px(ps[q]) * 4 * words;
        }
        HIPC(hipSetDevice(ctx->device));
        int rc;
        if (stage && (rc = grow(ctx, &ctx->d_stage, ctx->stage_cap, stage))) return rc;
        if ((rc = full_target(ctx, a, d_dst, &dst, &dst_hit, false))) return rc;
    }
    // one group: every non-root rank sends its compact frames (on its stream: after its render), the root receives
    // every peer's into its staging slot
    NCCLC(rccl().GroupStart());
    for (int l = 0; l < nl; l++) {
        rt_ctx* c = cm->ctxs[l];
        if (l != root) {
            NCCLC(rccl().Send(payload_of(c), part_px(ps[l]) * words, ncclUint32, root, cm->comms[l], c->stream));
        } else {
            for (int q = 0; q < cm->nranks; q++)
                if (q != root)
                    NCCLC(rccl().Recv(rctx->d_stage + at[q], part_px(ps[q]) * words, ncclUint32, q, cm->comms[l], c->stream));
        }
    }
    NCCLC(rccl().GroupEnd());
    cm->info.gathers++;
    rt_ctx* ctx = rctx;
    HIPC(hipSetDevice(ctx->device));
    int rc;
    for (int q = 0; q < cm->nranks; q++) {
        const void* s = q == root ? payload_of(ctx) : (const void*)(ctx->d_stage + at[q]);
        if ((rc = unshuffle(ctx, s, dst, ps[q], words, ctx->stream))) return rc;
    }
    return finish_gather(ctx, a, dst, dst_hit);
}

extern "C" int rt_comm_gather(rt_comm* cm, int root, void* d_dst) { return rt_comm_gather_from(cm, nullptr, root, d_dst); }

extern "C" int rt_comm_relayout(rt_comm* cm) {
    if (!cm) return RT_E_ARG;
    cm->have_layout = false;  // the next gather exchanges (every rank calls this before the same gather)
    return RT_OK;
}

extern "C" int rt_comm_set_timeout(rt_comm* cm, double seconds) {
    if (!cm || !(seconds > 0.0)) return RT_E_ARG;
    cm->timeout_s = seconds;
    return RT_OK;
}

extern "C" int rt_comm_wait(rt_comm* cm) {
    if (!cm) return RT_E_ARG;
    if (cm->aborted) return RT_E_TIMEOUT;
    if (!cm->issued || !cm->done) return RT_OK;
    (void)hipSetDevice(cm->devices[0]);
    if (cm->multi) return comm_settle(cm, "rt_comm_wait: the gathers issued");
    return comm_wait(cm, [&] { return hipEventQuery(cm->done); }, "rt_comm_wait: the last gather");
}

extern "C" int rt_comm_get_info(rt_comm* cm, rt_comm_info* info) {
    if (!cm || !info) return RT_E_ARG;
    *info = cm->info;
    return RT_OK;
}

extern "C" const char* rt_comm_last_error(rt_comm* cm) { return cm ? cm->err.c_str() : "null communicator"; }

extern "C" void rt_comm_destroy(rt_comm* cm) {
    if (!cm) return;
    // (the contexts may be gone already: only the communicator's own devices, events and streams are touched)
    // the last send / recv group (any context's stream) has run -- or its peers never came and the bounded wait
    // aborted the communicator (comm_abort): nothing left to wait for
    if (cm->issued && cm->done && !cm->aborted) (void)rt_comm_wait(cm);
    for (size_t l = 0; l < cm->comms.size(); l++) {
        (void)hipSetDevice(cm->devices[l]);
        if (!cm->multi && !cm->aborted) (void)hipDeviceSynchronize();  // (one process: the groups ran on the contexts' streams)
        if (cm->comms[l]) (void)rccl().CommDestroy(cm->comms[l]);
    }
    if (cm->side && !cm->aborted) (void)hipStreamSynchronize(cm->side);
    if (cm->d_desc) (void)hipFree(cm->d_desc);
    if (cm->d_count) (void)hipFree(cm->d_count);
    if (cm->h_desc) (void)hipHostFree(cm->h_desc);
    if (cm->side) (void)hipStreamDestroy(cm->side);
    if (cm->done) (void)hipEventDestroy(cm->done);
    for (const rt_comm::Pending& p : cm->pending) cm->ev_pool.insert(cm->ev_pool.end(), {p.pre, p.done});
    for (hipEvent_t e : cm->ev_pool) (void)hipEventDestroy(e);
    cm->link->cm = nullptr;  // (the contexts that still hold the link see the communicator gone)
    delete cm;
}

extern "C" int rt_download_bmp(rt_ctx* ctx, unsigned char* h_bmp, size_t cap) {
    if (!ctx || !h_bmp) return RT_E_ARG;
    if (!ctx->rendered) {
        ctx->err = "rt_download_bmp: nothing rendered";
        return RT_E_STATE;
    }
    if (ctx->last_frames != 1) return arg_err(ctx, "rt_download_bmp: the last render was a frame batch");
    if (!ctx->last_rgb && !ctx->last_bgra) return arg_err(ctx, "rt_download_bmp: no pixels in the last render");
    const int W = ctx->last_W, H = ctx->last_H;
    if (ctx->last_off != 0 || ctx->last_stride != ctx->last_block || ctx->last_rows != H) {
        ctx->err = "rt_download_bmp: the last frame is not a full frame (gather it first)";
        return RT_E_STATE;
    }
    const size_t px = (size_t)W * H;
    if (cap < 54 + 4 * px) return arg_err(ctx, "rt_download_bmp: buffer too small");
    HIPC(hipSetDevice(ctx->device));
    int rc;
    if ((rc = grow(ctx, &ctx->d_bmp, ctx->bmp_cap, px))) return rc;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((px + 255) / 256, 4096));
    if (ctx->last_rgb) rtd::k_bgra<<<grid, 256, 0, ctx->stream>>>(ctx->last_rgb, ctx->d_bmp, W, H);
    else rtd::k_flip_rows<<<grid, 256, 0, ctx->stream>>>(ctx->last_bgra, ctx->d_bmp, W, H);  // already quantised
    HIPC(hipGetLastError());
    if (rth_bmp_header(W, H, h_bmp) != RT_OK) return arg_err(ctx, "rt_download_bmp: bad frame size");
    HIPC(hipMemcpyAsync(h_bmp + 54, ctx->d_bmp, 4 * px, hipMemcpyDeviceToHost, ctx->stream));
    return sync_checked(ctx, "rt_download_bmp");
}

extern "C" int rt_get_stats(rt_ctx* ctx, rt_stats* st) {
    if (!ctx || !st) return RT_E_ARG;
    HIPC(hipSetDevice(ctx->device));
    HIPC(hipStreamSynchronize(ctx->stream));
    unsigned long long c[rtd::NCOUNT];
    HIPC(hipMemcpy(c, ctx->d_counters, sizeof c, hipMemcpyDeviceToHost));
    std::memset(st, 0, sizeof *st);
    st->primary = c[rtd::C_PRIM];
    st->reflection = c[rtd::C_REFL];
    st->shadow = c[rtd::C_SHAD];
    st->shadow_skipped = c[rtd::C_SKIP];
    st->hits = c[rtd::C_HITS];
    st->ch_inner = c[rtd::C_CHI];
    st->ch_leaf = c[rtd::C_CHL];
    st->ch_tri = c[rtd::C_CHT];
    st->sh_inner = c[rtd::C_SHI];
    st->sh_leaf = c[rtd::C_SHL];
    st->sh_tri = c[rtd::C_SHT];
    st->pixels = c[rtd::C_PIX];
    st->fallbacks = c[rtd::C_FALLBACK];
    st->stack_overflows = c[rtd::C_ERR];
    st->node_bytes = 8 * c[rtd::C_NB];
    st->wave_steps = c[rtd::C_WS];
    st->shadow_wave_steps = c[rtd::C_WSH];
    st->steps_lanes_16 = c[rtd::C_Q1];
    st->steps_lanes_32 = c[rtd::C_Q2];
    st->steps_lanes_48 = c[rtd::C_Q3];
    st->steps_lanes_64 = c[rtd::C_Q4];
    std::memcpy(st->steps_hist, c + rtd::C_HIST, sizeof st->steps_hist);
    static_assert(sizeof st->steps_hist == 32 * sizeof(unsigned long long), "histogram slots");
    if (c[rtd::C_ERR]) {
        ctx->err = "rt_get_stats: the render's traversal stack overflowed (BVH deeper than the walks' stacks)";
        return RT_E_KERNEL;
    }
    return RT_OK;
}

extern "C" const char* rt_last_error(rt_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // a send / recv group on this stream: waited for through the communicator (bounded; aborted if a peer never
    // joins), and the communicator forgets this context
    (void)comm_settle_ctx(ctx, "rt_destroy");
    if (ctx->comm_link && ctx->comm_link->cm)
        for (rt_ctx*& c : ctx->comm_link->cm->ctxs)
            if (c == ctx) c = nullptr;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_scene(ctx);
    if (ctx->gather_ev) (void)hipEventDestroy(ctx->gather_ev);
    if (ctx->copy_ev) (void)hipEventDestroy(ctx->copy_ev);
    if (ctx->d_rgb_own) (void)hipFree(ctx->d_rgb_own);
    if (ctx->d_cams) (void)hipFree(ctx->d_cams);
    if (ctx->d_pathbuf) (void)hipFree(ctx->d_pathbuf);
    if (ctx->d_lanebuf) (void)hipFree(ctx->d_lanebuf);
    if (ctx->d_gstack) (void)hipFree(ctx->d_gstack);
    if (ctx->h_cams) (void)hipHostFree(ctx->h_cams);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->h_err) (void)hipHostFree(ctx->h_err);
    for (auto& o : ctx->orders) (void)hipFree(o.second);
    for (void* p : {(void*)ctx->d_full, (void*)ctx->d_full_hit, (void*)ctx->d_stage, (void*)ctx->d_bmp,
                    (void*)ctx->d_full_bgra})
        if (p) (void)hipFree(p);
    if (ctx->d_work) (void)hipFree(ctx->d_work);
    for (rt_ctx::QuerySlot& q : ctx->slots) {
        if (q.counters) (void)hipFree(q.counters);
        if (q.ev0) (void)hipEventDestroy(q.ev0);
        if (q.ev1) (void)hipEventDestroy(q.ev1);
    }
    for (void* p : {(void*)ctx->d_plan, (void*)ctx->d_area})
        if (p) (void)hipFree(p);
    if (ctx->h_plan) (void)hipHostFree(ctx->h_plan);
    if (ctx->h_lights) (void)hipHostFree(ctx->h_lights);
    for (hipEvent_t e : {ctx->u_ev0, ctx->u_ev1, ctx->u_evs, ctx->lights_ev, ctx->r_ev0, ctx->r_ev1, ctx->r_evs})
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < rt_ctx::NEV; i++) {
        if (ctx->ev0s[i]) (void)hipEventDestroy(ctx->ev0s[i]);
        if (ctx->ev1s[i]) (void)hipEventDestroy(ctx->ev1s[i]);
    }
    if (ctx->hy.s2) (void)hipStreamSynchronize(ctx->hy.s2);
    if (ctx->hy.d_tr) (void)hipFree(ctx->hy.d_tr);
    if (ctx->hy.d_cost) (void)hipFree(ctx->hy.d_cost);
    if (ctx->hy.d_fb) (void)hipFree(ctx->hy.d_fb);
    if (ctx->hy.d_info) (void)hipFree(ctx->hy.d_info);
    if (ctx->hy.h_fb_cnt) (void)hipHostFree(ctx->hy.h_fb_cnt);
    if (ctx->hy.fb_ev) (void)hipEventDestroy(ctx->hy.fb_ev);
    if (ctx->hy.h_tr) (void)hipHostFree(ctx->hy.h_tr);
    if (ctx->hy.d_lists) (void)hipFree(ctx->hy.d_lists);
    if (ctx->hy.h_lists) (void)hipHostFree(ctx->hy.h_lists);
    for (hipEvent_t e : ctx->cam_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ctx->hy.ev, ctx->hy.fork, ctx->hy.join})
        if (e) (void)hipEventDestroy(e);
    if (ctx->hy.s2) (void)hipStreamDestroy(ctx->hy.s2);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}
