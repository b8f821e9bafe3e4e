// rt_query_logic.hpp — what the query entry points (rt_trace_rays ... rt_sweep_tri_contacts, rt_hip.hip) decide
// alike, kept free of HIP so that tests/c/query_logic_test.cpp can check it with g++ alone:
//   * Fam / FAMILY / family(): the families, and the words in which their messages differ;
//   * check_enter, check_args, check_count_out: the argument checks all of them make, with their messages;
//   * list_capacity: the list families' kernel capacity for a max_hits / max_tris;
//   * grid_blocks: the persistent grid of a query launch.
// A check that one family alone makes stays in its entry point; allocating and launching stay in rt_hip.hip.
#pragma once
#include <algorithm>
#include <string>

#include "rt_hip.h"

namespace rtq {

// NFAM counts the ten families that tests/c/query_logic_test.cpp tabulates (its EXPECT[rtq::NFAM] has ten rows and its
// loops run to NFAM), so it keeps the value 10. A family added since is numbered from NFAM upward; NFAM_ALL ends the
// list that tests/c/proximity_logic_test.cpp holds at eleven and sizes FAMILY. Families added after that are numbered
// from NFAM_ALL upward, have their rows in FAMILY_MORE and end at NFAM_SLOTS, which sizes rt_ctx::slots; family() finds
// the row of any of them. Each such family's row has a test of its own (tests/c/proximity_logic_test.cpp,
// tests/c/trisweep_logic_test.cpp).
// tests/c/trisweep_logic_test.cpp in turn holds NFAM_SLOTS at 12 and FAMILY_MORE at NFAM_SLOTS - NFAM_ALL rows, so
// families added after it are numbered from NFAM_SLOTS upward (TRICONTACTS = NFAM_SLOTS), have their rows in
// FAMILY_LATER and end at NFAM_END, which sizes rt_ctx::slots. This is the last table: tests/c/tricontacts_logic_test.cpp
// asserts its family's number, its row's words and its messages, and neither NFAM_END's value nor FAMILY_LATER's row
// count, so the next family appends its enumerator before NFAM_END and its row to FAMILY_LATER, and writes its own
// test the same way.
enum Fam { RAYS, SHADE, HITS, NEAREST, NEIGHBOURS, OVERLAPS, SWEEP, CONTACTS, CUTS, CLEARANCE, NFAM, PROXIMITY = NFAM,
           NFAM_ALL, TRISWEEP = NFAM_ALL, NFAM_SLOTS, TRICONTACTS = NFAM_SLOTS, NFAM_END };

struct Family {
    const char* fn;     // the entry point, as its messages begin
    const char* items;  // what it is given ("null <items> / results")
    const char* noun;   // what n counts ("negative <noun> count")
    const char* cap;    // the list families' capacity field; null: the family has no lists
};
constexpr Family FAMILY[NFAM_ALL] = {
    {"rt_trace_rays", "rays", "ray", nullptr},
    {"rt_shade_rays", "rays", "ray", nullptr},
    {"rt_trace_hits", "rays", "ray", "max_hits"},
    {"rt_nearest_points", "points", "point", nullptr},
    {"rt_nearest_tris", "points", "point", "max_tris"},
    {"rt_overlap_boxes", "boxes", "box", "max_tris"},
    {"rt_sweep_spheres", "spheres", "sphere", nullptr},
    {"rt_sweep_contacts", "spheres", "sphere", "max_tris"},
    {"rt_cut_triangles", "tris", "triangle", "max_tris"},
    {"rt_clearance_triangles", "tris", "triangle", nullptr},
    {"rt_proximity_triangles", "tris", "triangle", "max_tris"},
};
constexpr Family FAMILY_MORE[NFAM_SLOTS - NFAM_ALL] = {
    {"rt_sweep_triangles", "tris", "triangle", nullptr},
};
constexpr Family FAMILY_LATER[NFAM_END - NFAM_SLOTS] = {
    {"rt_sweep_tri_contacts", "tris", "triangle", "max_tris"},
};
constexpr const Family& family(Fam f) {
    return f < NFAM_ALL ? FAMILY[f] : f < NFAM_SLOTS ? FAMILY_MORE[f - NFAM_ALL] : FAMILY_LATER[f - NFAM_SLOTS];
}

constexpr int LIST_MAX = 16;  // RT_HITS_MAX, RT_NEIGHBOURS_MAX, ... (rt_hip.hip asserts each)

// Every check returns RT_OK, or the call's status with its message in err (untouched otherwise).
inline int refuse(int rc, Fam f, const std::string& what, std::string& err) {
    err = std::string(family(f).fn) + ": " + what;
    return rc;
}

// the first checks of an entry point: a scene, and both argument structs
inline int check_enter(Fam f, bool has_scene, bool have_args, std::string& err) {
    if (!has_scene) return refuse(RT_E_STATE, f, "no scene uploaded", err);
    if (!have_args) return refuse(RT_E_ARG, f, std::string("null ") + family(f).items + " / results", err);
    return RT_OK;
}

// kernel and n; for a list family also its capacity (Family::cap names the field) and count_all
inline int check_args(Fam f, int kernel, int n, int cap, int count_all, std::string& err) {
    if (kernel < RT_KERNEL_AUTO || kernel > RT_KERNEL_FAST) return refuse(RT_E_ARG, f, "bad kernel", err);
    if (n < 0) return refuse(RT_E_ARG, f, std::string("negative ") + family(f).noun + " count", err);
    const char* field = family(f).cap;
    if (!field) return RT_OK;
    if (cap < 0 || cap > LIST_MAX) return refuse(RT_E_ARG, f, std::string(field) + " must be 0..16", err);
    if (count_all != 0 && count_all != 1) return refuse(RT_E_ARG, f, "count_all must be 0 or 1", err);
    if (cap == 0 && !count_all) return refuse(RT_E_ARG, f, std::string(field) + " = 0 needs count_all", err);
    return RT_OK;
}
inline int check_args(Fam f, int kernel, int n, std::string& err) { return check_args(f, kernel, n, 0, 1, err); }

// a list family's last check: a query that only counts writes counts
inline int check_count_out(Fam f, int n, int cap, bool has_count, std::string& err) {
    if (n > 0 && cap == 0 && !has_count) return refuse(RT_E_ARG, f, "a counting query needs a count output", err);
    return RT_OK;
}

// the smallest list capacity a kernel is built for that holds cap entries (0: the counting build)
constexpr int list_capacity(int cap) { return cap == 0 ? 0 : cap <= 4 ? 4 : cap <= 8 ? 8 : 16; }

// workgroups of a query launch: persistent ones that take chunks of `chunk` queries from a counter, four chunks per
// workgroup while that leaves some of the `resident` ones idle
inline int grid_blocks(int n, int chunk, int resident) {
    const int chunks = (int)(((long long)n + chunk - 1) / chunk);
    return std::max(1, std::min(resident, (chunks + 3) / 4));
}

}  // namespace rtq
