// rt_collapse.hpp — the greedy collapse of a binary BVH into 8-wide nodes: one wide node's decision, shared by the host
// mirror (rt_wide.cpp rth_wbvh_build_greedy) and the device rebuild (rt_hip.hip rt_rebuild_views, k_collapse below):
// plain C++17 under g++, __host__ __device__ under hipcc, and the same choice from both.
//
// The rule is rt_wide.cpp's header comment: a wide node starts from the two children of a binary node and repeatedly
// opens the open child of largest box area that is interior and holds more than LEAF_MAX triangles, until it has 8
// children or none can be opened. Ties in area: the leftmost child. An opened child is replaced in place by its left and
// right child, so the children always stand in the binary tree's left-to-right order. A child with at most LEAF_MAX
// triangles becomes a leaf slot over its whole subtree. Areas are compared as doubles of exact products of the float
// extents (no rounding that a contraction could change). The slots follow the host collapse's octant rule (rt_wide.cpp
// form): greedy on -dot(child centre - node centre, slot direction), additions and halvings only.
//
// The tree is read through a small accessor (Tree): interior(i), left(i), right(i), count(i) and box(i, lo, hi). The
// device kernels (HIP only, below the shared part) run it over PLOC's arrays (rt_build.hpp), one thread per wide node
// and one launch pair per wide level; a level's child and triangle bases come from an exclusive scan in node order, so
// the layout is the breadth-first one k_wide_level needs and no atomic decides an index.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RTC_HD __host__ __device__ inline
#else
#define RTC_HD inline
#endif

#ifndef RTC_SLOT_OCTANT
#define RTC_SLOT_OCTANT 1  // 1: the host collapse's octant slots; 0: arrival (left-to-right) order. DESIGN §3n
#endif

namespace rtc {

constexpr int WIDTH = 8;
constexpr int LEAF_MAX = 4;

// half the surface area, in double: the three products of float extents are exact, so the sum rounds the same
// whichever way a compiler forms it
RTC_HD double half_area(const float* lo, const float* hi) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return (double)dx * (double)dy + (double)dy * (double)dz + (double)dz * (double)dx;
}

// One wide node over binary node b: its children into kid[0 .. k - 1], left to right; returns k (1: b itself, a tree of
// at most LEAF_MAX triangles -- the root only).
template <class Tree>
RTC_HD int collapse(const Tree& t, int b, int* kid) {
    if (!t.interior(b) || t.count(b) <= LEAF_MAX) {
        kid[0] = b;
        return 1;
    }
    double area[WIDTH];
    float lo[3], hi[3];
    int k = 2;
    kid[0] = t.left(b);
    kid[1] = t.right(b);
    for (int c = 0; c < 2; c++) {
        t.box(kid[c], lo, hi);
        area[c] = half_area(lo, hi);
    }
    while (k < WIDTH) {
        int best = -1;
        for (int c = 0; c < k; c++)
            if (t.interior(kid[c]) && t.count(kid[c]) > LEAF_MAX && (best < 0 || area[c] > area[best])) best = c;
        if (best < 0) break;
        for (int c = k; c > best + 1; c--) {
            kid[c] = kid[c - 1];
            area[c] = area[c - 1];
        }
        const int open = kid[best];
        kid[best] = t.left(open);
        kid[best + 1] = t.right(open);
        for (int c = best; c < best + 2; c++) {
            t.box(kid[c], lo, hi);
            area[c] = half_area(lo, hi);
        }
        k++;
    }
    return k;
}

// The children's slots: slot_kid[s] = the position in kid[] of the child in slot s, or -1.
template <class Tree>
RTC_HD void assign_slots(const Tree& t, const int* kid, int k, int* slot_kid) {
    for (int s = 0; s < WIDTH; s++) slot_kid[s] = -1;
#if RTC_SLOT_OCTANT
    float off[WIDTH][3], alo[3], ahi[3], lo[3], hi[3];
    for (int c = 0; c < k; c++) {
        t.box(kid[c], lo, hi);
        for (int a = 0; a < 3; a++) {
            off[c][a] = 0.5f * (lo[a] + hi[a]);
            alo[a] = (c == 0 || lo[a] < alo[a]) ? lo[a] : alo[a];
            ahi[a] = (c == 0 || hi[a] > ahi[a]) ? hi[a] : ahi[a];
        }
    }
    for (int a = 0; a < 3; a++) {
        const float pc = 0.5f * (alo[a] + ahi[a]);
        for (int c = 0; c < k; c++) off[c][a] = off[c][a] - pc;
    }
    bool done[WIDTH] = {false, false, false, false, false, false, false, false};
    for (int round = 0; round < k; round++) {
        float bc = 0.0f;
        int bk = -1, bs = -1;
        for (int c = 0; c < k; c++) {
            if (done[c]) continue;
            for (int s = 0; s < WIDTH; s++) {
                if (slot_kid[s] >= 0) continue;
                float cost = 0.0f;
                for (int a = 0; a < 3; a++) cost -= ((s >> a) & 1) ? off[c][a] : -off[c][a];
                if (bk < 0 || cost < bc) {
                    bc = cost;
                    bk = c;
                    bs = s;
                }
            }
        }
        done[bk] = true;
        slot_kid[bs] = bk;
    }
#else
    (void)t;
    (void)kid;
    for (int c = 0; c < k; c++) slot_kid[c] = c;
#endif
}

// The topology words of a wide node (rt_device.hpp DWide; the box words stay 0 until the fill, rt_quant.hpp requantise):
// imask into W[3]'s top byte, W[4] = child_base, W[5] = tri_base, the 8 meta bytes (count << 5 | offset) into W[6..7].
RTC_HD void topology_words(uint32_t* W, uint32_t imask, uint32_t child_base, uint32_t tri_base, const uint8_t* meta) {
    for (int j = 0; j < 20; j++) W[j] = 0;
    W[3] = imask << 24;
    W[4] = child_base;
    W[5] = tri_base;
    for (int s = 0; s < WIDTH; s++) W[6 + (s >> 2)] |= (uint32_t)meta[s] << (8 * (s & 3));
}

}  // namespace rtc

#if defined(__HIPCC__)
namespace rtc {

// PLOC's tree (rt_build.hpp): nodes 0 .. n - 1 are the leaves (one triangle each), n .. 2 n - 2 the merges with their
// children at left / right[id - n]; every node's box in nlo / nhi and its triangle count in cnt.
struct DevTree {
    const int *lft, *rgt, *cnt;
    const float4 *nlo, *nhi;
    int n;
    __device__ bool interior(int i) const { return i >= n; }
    __device__ int left(int i) const { return lft[i - n]; }
    __device__ int right(int i) const { return rgt[i - n]; }
    __device__ int count(int i) const { return cnt[i]; }
    __device__ void box(int i, float* lo, float* hi) const {
        const float4 l = nlo[i], h = nhi[i];
        lo[0] = l.x, lo[1] = l.y, lo[2] = l.z;
        hi[0] = h.x, hi[1] = h.y, hi[2] = h.z;
    }
};

// One wide level, first half: wide node i of the level collapses binary node item[i]; its slots' binary nodes go to
// slots[8 i + s] (-1: empty) and its interior-child and leaf-triangle counts, packed (interior << 32 | triangles), to
// sums[i] for the level's exclusive scan.
__global__ __launch_bounds__(64) void k_collapse(DevTree t, const int* __restrict__ item, int count,
                                                 int* __restrict__ slots, unsigned long long* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    int kid[WIDTH], slot_kid[WIDTH];
    const int k = collapse(t, item[i], kid);
    assign_slots(t, kid, k, slot_kid);
    unsigned long long inner = 0, tri = 0;
    for (int s = 0; s < WIDTH; s++) {
        const int b = slot_kid[s] >= 0 ? kid[slot_kid[s]] : -1;
        slots[8 * (size_t)i + s] = b;
        if (b < 0) continue;
        const int c = t.count(b);
        if (c <= LEAF_MAX) tri += (unsigned long long)c;
        else inner++;
    }
    sums[i] = (inner << 32) | tri;
}

// One wide level, second half, after the scan of sums (scan[i]: the interior children and leaf triangles of the level's
// nodes before i): node first + i gets its topology words, its interior children's binary nodes go to next[] in child
// order and its leaf triangles to the view's position -> triangle map (orig; ids: leaf -> scene triangle, sorted: leaf
// -> PLOC's input position, sub: that position -> scene triangle or null for the identity). A leaf slot lists its
// subtree's triangles left to right (at most LEAF_MAX: a walk of at most 7 nodes).
__global__ __launch_bounds__(64) void k_emit(DevTree t, const int* __restrict__ slots,
                                             const unsigned long long* __restrict__ scan, int first, int count,
                                             int next_first, int tri_first, const int* __restrict__ sorted,
                                             const int* __restrict__ sub, float4* __restrict__ nodes,
                                             int* __restrict__ next, int* __restrict__ orig) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned long long sc = scan[i];
    const int inner0 = (int)(sc >> 32), tri0 = (int)(sc & 0xFFFFFFFFull);
    uint32_t imask = 0;
    uint8_t meta[WIDTH];
    int ni = 0, nt = 0;
    for (int s = 0; s < WIDTH; s++) {
        meta[s] = 0;
        const int b = slots[8 * (size_t)i + s];
        if (b < 0) continue;
        const int c = t.count(b);
        if (c > LEAF_MAX) {
            imask |= 1u << s;
            next[inner0 + ni++] = b;
            continue;
        }
        meta[s] = (uint8_t)((c << 5) | nt);
        int stack[LEAF_MAX], sp = 0, cur = b;
        for (;;) {  // left first
            if (t.interior(cur)) {
                stack[sp++] = t.right(cur);
                cur = t.left(cur);
                continue;
            }
            const int p = sorted[cur];
            orig[tri_first + tri0 + nt++] = sub ? sub[p] : p;
            if (sp == 0) break;
            cur = stack[--sp];
        }
    }
    uint32_t W[20];
    topology_words(W, imask, (uint32_t)(next_first + inner0), (uint32_t)(tri_first + tri0), meta);
    for (int j = 0; j < 5; j++)
        nodes[5 * (size_t)(first + i) + j] =
            make_float4(__int_as_float((int)W[4 * j]), __int_as_float((int)W[4 * j + 1]),
                        __int_as_float((int)W[4 * j + 2]), __int_as_float((int)W[4 * j + 3]));
}

// ---- subset compaction: flag[i] = the triangle's |n|^2 reaches x (rt_refit.hpp k_plan's form of hittable()), then,
// after the exclusive scan of flag, the subset's triangle ids and its compact vertex array
__global__ __launch_bounds__(256) void k_hittable(const float* __restrict__ coords, int n, double x,
                                                  int* __restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = coords + 9 * (size_t)i;
    const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
    const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    flag[i] = ((double)nx * nx + (double)ny * ny + (double)nz * nz) >= x;
}

__global__ __launch_bounds__(256) void k_gather(const float* __restrict__ coords, int n, const int* __restrict__ flag,
                                                const int* __restrict__ at, int* __restrict__ sub,
                                                float* __restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int k = at[i];
    sub[k] = i;
    for (int j = 0; j < 9; j++) v[9 * (size_t)k + j] = coords[9 * (size_t)i + j];
}

// the scene triangle of every leaf of PLOC's tree (test read-back: rt_debug_read_build_tree)
__global__ __launch_bounds__(256) void k_leaf_ids(const int* __restrict__ sorted, const int* __restrict__ sub, int n,
                                                  int* __restrict__ ids) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) ids[k] = sub ? sub[sorted[k]] : sorted[k];
}

}  // namespace rtc
#endif
