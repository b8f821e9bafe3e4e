// rt_tricontacts.hpp — triangle contact queries: the k earliest contacts of each caller-supplied moving triangle with
// the mesh and the number of contacts (rt_sweep_tri_contacts, rt_hip.h): rt_sweep_triangles' plural form, as
// rt_contacts.hpp is rt_sweep_spheres' and rt_proximity.hpp is rt_clearance_triangles'.
//
// Query i is rt_sweep_triangles' own (corners q + t d, 0 <= t <= T = fminf(t_max[i], FLT_MAX)) and so is its candidate
// set, in its order:
//   S_i = { j : toi(i, record j) exists and toi <= T }, ordered by (toi ascending, original triangle index ascending),
// empty under the sweep's rules (a non-finite one among the twelve numbers, a NaN or negative t_max[i]; decided before
// any walk). toi, the contact point and the kind are rt_trisweep.hpp's tsw_gate and tsw_tri, called and not restated.
// The answer is the first max_tris entries of S_i and min(|S_i|, max_tris), or |S_i| itself with count_all. That is a
// total order, so the answer depends on no view, lane or visiting order.
//
// A pair's toi, point and kind depend on the query and the record alone. tend enters tsw_gate as the first value of the
// interval's END (a1) alone; t0 is built from 0 and the plane times; tsw_tri reads t0 and never a1, and uses tend only
// in its last comparison toi <= tend. So a record that is accepted under two different limits has the same toi, point
// and kind bits under both: the limit may shrink during a walk, and a pair may be evaluated again after it.
//
// The per-query list is rt_hits.hpp's HState, filled by rt_neighbours.hpp's neighbours_take: up to CAP 64-bit keys
// toi_bits << 32 | original index (toi >= +0: t0 starts at +0 and only grows by fmaxf, u >= 0, so one unsigned compare
// is the lexicographic one), kept sorted. Where the keys live and the occupancy are chosen per build (tct_reg and
// tct_waves below). Instantiated for CAP = 0 (counting only), 4, 8 and 16; a request runs the smallest
// that holds max_tris.
//
// The limit: lim (S.bound) = fminf(T, the max_tris-th stored toi once the list is full), and T alone for the whole walk
// with count_all. It is handed to tsw_gate and tsw_tri in T's place, for slots and records alike.
//
// Two kernels of k_trisweep's skeleton (persistent waves, QUERY_CHUNK queries per returning atomic, one query per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig; each
//                     record passes its own gate under T (the limit never follows the list here), each accepted toi is
//                     counted and offered to the list. The checker.
//   RT_KERNEL_FAST    tsw_wide's walk of the full wide view (per-level LDS stack entries (node, slots still to try), the
//                     node decoded again on a pop, slots, leaf and interior alike, in order of their gate t0, ties: the
//                     lowest slot) with the list's limit in the place of the best toi. A slot is kept while t0 <= lim
//                     and dropped only when t0 is STRICTLY greater. A record of a visited leaf slot passes its own gate
//                     under lim (else counted in pairs_gated), then tsw_tri under lim. A scene without a wide view
//                     (RT_ACCEL_REFERENCE) and a query outside tsw_domain run the exhaustive loop under either kernel.
// tct_wide is a sibling of tsw_wide, not a generalisation of it: rt_trisweep.hpp is untouched, so k_trisweep compiles
// to the code it had.
//
// Why the answer is the definition's, in two parts.
// 1. Nothing that belongs is pruned. lim never grows during a walk: it starts at T and is only ever replaced by the
//    max_tris-th key's toi, which an insertion can only lower; with count_all it stays T. So the final max_tris-th toi
//    is <= every earlier lim. A member of the answer has toi <= the final max_tris-th toi (or <= T, with count_all or a
//    list that never fills), hence toi <= lim at every moment. By (P1) of rt_trisweep.hpp its own gate
//    t0 <= toi <= lim. By (P2) every slot on its path has t0(slot) <= t0(record) and a gate interval that contains the
//    record's: with the interval's end clipped to lim >= toi >= t0(record), neither the slot's interval nor the
//    record's is empty, and t0(slot) <= lim. So no slot on its path is dropped (the drop needs an empty interval or
//    t0 > lim), whatever was found before, and tsw_tri under lim accepts the record with the toi it has under T
//    (above). An entry that ties the k-th toi with a lower index has toi == lim: it is still reached (<=), its key is
//    smaller, and it displaces the k-th. Pinned by tests/test_gpu_tricontacts.py: test_variants (every k on both sides
//    of every capacity, against the yardstick), test_fixture (boundary ties at k = 4, 8, 16 are present),
//    test_bound_at_kth (the bound on the k-th toi, one float below and above) and test_fast_is_strict.
// 2. Each record is offered at most once per query; a repeated offer would duplicate an entry or inflate a count. The
//    walk relies on all of: (a) the wide view holds each record in exactly one leaf slot (tests/test_gpu_hits.py checks
//    the views' tri_orig for duplicates); (b) a slot leaves the level's mask m before it is tested or entered, and a
//    stack entry's mask is that m, so it holds only untried slots: a pop neither tests a leaf slot nor enters a child
//    again; (c) the entry mask of a freshly entered node is all eight slots, and a child is entered only from its one
//    parent slot, hence once. The exhaustive loop offers record j at step j. Pinned by tests/test_gpu_tricontacts.py:
//    the count_all counts of test_variants and test_doubled (every triangle twice gives exactly twice).
//
// The point and kind outputs. The list holds keys only. After the walk, for each stored entry, the record of the
// REFERENCE tree is found through ref_inv (rt_neighbours.hpp: every view's records hold the same bits), tsw_gate runs
// on its corner box under T and tsw_tri under T: the pair's own point and kind, with the walk's bits because neither
// depends on the limit. An unused slot holds q0's own bits and kind -1.
//
// LDS: the walk's 2 x WSTACK ints of the per-level stack in the STACK-int column (34,816 B per workgroup), plus the
// column of CAP - REG keys per lane (2,048 B per key and workgroup) in the builds that have one.
#pragma once
#include "rt_neighbours.hpp"
#include "rt_trisweep.hpp"

namespace rtd {

constexpr int TRICONTACTS_MAX = 16;  // RT_TRICONTACTS_MAX
enum { TC_TRIS, TC_FOUND, TC_STORED, TC_COUNTED, TC_WALKED, TC_EXH, TC_EMPTY, TC_NODES, TC_GATED, TC_PAIRS, TC_ERR,
       TC_NCOUNT };

struct TCArgs {
    DScene s;
    const float* tris;    // [n][3][3]
    const float* motion;  // [n][3]
    const float* t_max;   // nullable
    int* tri;             // [n][max_tris], nullable
    float* t;             // [n][max_tris], nullable
    float* out;           // [n][max_tris][3], nullable
    int* kind;            // [n][max_tris], nullable
    int* count;           // [n], nullable
    const int* ref_inv;   // original triangle index -> position in s.ref.tris (read only for the points and kinds)
    unsigned long long* counters;  // TC_NCOUNT slots of the triangle contact query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    float c_max;  // tsw_domain's bound (TSArgs::c_max)
    int max_tris;
    int count_all;
};
static_assert(sizeof(TCArgs) == sizeof(DScene) + 11 * 8 + 16, "kernel-argument layout: both passes must agree");

// Where a build's keys live and its waves per SIMD, from the code object's figures (the table and the
// placements that were compiled and rejected). tct_reg of the CAP keys are in registers, the other CAP - tct_reg in
// the lane's LDS column. tsw_wide's walk leaves ten of the 168 VGPRs of three waves per SIMD: four keys fit beside it
// (166), eight do not (168 and 17 spilled, reloaded inside the walk), so the 8-key build keeps keys 5..8 in LDS (160);
// the 16-key build keeps rt_hits.hpp's placement, 8 + 8, and comes out at exactly 168 with no scratch. Every build
// stays at three waves per SIMD, by registers and by LDS (3 x 51,200 B <= 160 KB). The exhaustive kernels have no walk
// and hold 4 keys in registers, the rest in LDS, as k_proximity's do.
constexpr int tct_reg(int cap, bool strict) { return strict || cap <= 8 ? (cap <= 4 ? cap : 4) : 8; }
constexpr int tct_waves(int, bool) { return 3; }

// the record's own gate under the list's limit, then toi: false when the gate turned the record away (no evaluation of
// toi). An accepted toi is counted and offered to the list (neighbours_take; `all`: lim stays T)
template <class ST>
__device__ __forceinline__ bool tct_take(ST& S, const TSTri& Q, const float4* __restrict__ rec, int orig, int K,
                                         bool all) {
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
    const v3 a = mk(w0.x, w0.y, w0.z), b = add(a, mk(w0.w, w1.x, w1.y)), c = add(a, mk(w1.z, w1.w, w2.x));
    float t0;
    if (!tsw_gate(Q, vmin3(a, b, c), vmax3(a, b, c), S.bound, t0)) return false;
    float toi;
    v3 pt;
    int kind;
    if (tsw_tri(Q, rec, t0, S.bound, toi, pt, kind)) neighbours_take(S, toi, orig, K, all);
    return true;
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
template <class ST>
__device__ __forceinline__ void tct_exhaustive(const DScene& s, const TSTri& Q, ST& S, int K, bool all) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) (void)tct_take(S, Q, s.ref.tris + 3 * j, s.ref.tri_orig[j], K, all);
}

// leaf slot sl's 1..4 records (meta = count << 5 | offset), each gated, tested and offered to the list
template <class ST>
__device__ __forceinline__ void tct_leaf(const DWide& W, const TSTri& Q, ST& S, int K, bool all, unsigned sl,
                                         unsigned m0, unsigned m1, int tbase, unsigned long long& gated,
                                         unsigned long long& pairs) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
#pragma unroll 1
    for (int i = first; i < first + cnt; i++) {
        // (two sums, not a branch between the counters: tsw_leaf's note)
        const unsigned tested = tct_take(S, Q, W.tris + 3 * i, W.tri_orig[i], K, all) ? 1u : 0u;
        pairs += tested;
        gated += 1u - tested;
    }
}

// tsw_wide's walk with the list's limit S.bound in the place of the best toi (header)
template <class ST>
__device__ __forceinline__ void tct_wide(const DWide& W, const TSTri& Q, ST& S, int K, bool all, int* __restrict__ stk,
                                         unsigned long long& nodes, unsigned long long& gated,
                                         unsigned long long& pairs, unsigned& err) {
    const gnodes nbase = walk_base(W.nodes);
    int node = 0, sp = 0;
    unsigned mask = 0xFFu;
#pragma unroll 1
    for (;;) {
        const WNode N = wload_at(nbase, node);
        nodes++;
        const unsigned e = __float_as_uint(N.f0.w);
        const unsigned imask = e >> 24;
        const int cbase = __float_as_int(N.f1.x), tbase = __float_as_int(N.f1.y);
        const unsigned m0 = __float_as_uint(N.f1.z), m1 = __float_as_uint(N.f1.w);
        const v3 p = mk(N.f0.x, N.f0.y, N.f0.z);
        const v3 sc = mk(pow2_bits(e & 0xFFu), pow2_bits((e >> 8) & 0xFFu), pow2_bits((e >> 16) & 0xFFu));
        const unsigned wx[4] = {__float_as_uint(N.f2.x), __float_as_uint(N.f2.y), __float_as_uint(N.f2.z),
                                __float_as_uint(N.f2.w)},
                       wy[4] = {__float_as_uint(N.f3.x), __float_as_uint(N.f3.y), __float_as_uint(N.f3.z),
                                __float_as_uint(N.f3.w)},
                       wz[4] = {__float_as_uint(N.f4.x), __float_as_uint(N.f4.y), __float_as_uint(N.f4.z),
                                __float_as_uint(N.f4.w)};
        float b[8];
        unsigned m = 0u;  // the slots still to try: in the entry's mask, occupied, a gate interval within lim
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int j = s >> 1, sh = 16 * (s & 1);
            const unsigned qx = wx[j] >> sh, qy = wy[j] >> sh, qz = wz[j] >> sh;
            const v3 L = mk(__builtin_fmaf(sc.x, (float)(QBIAS + (qx & 0xFFu)), p.x),
                            __builtin_fmaf(sc.y, (float)(QBIAS + (qy & 0xFFu)), p.y),
                            __builtin_fmaf(sc.z, (float)(QBIAS + (qz & 0xFFu)), p.z));
            const v3 H = mk(__builtin_fmaf(sc.x, (float)(QBIAS + ((qx >> 8) & 0xFFu)), p.x),
                            __builtin_fmaf(sc.y, (float)(QBIAS + ((qy >> 8) & 0xFFu)), p.y),
                            __builtin_fmaf(sc.z, (float)(QBIAS + ((qz >> 8) & 0xFFu)), p.z));
            const bool open = tsw_gate(Q, L, H, S.bound, b[s]);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            if (((mask >> s) & 1u) && occ && open) m |= 1u << s;
        }
        bool descended = false;
#pragma unroll 1
        for (;;) {
            // the earliest remaining slot whose t0 does not exceed the (possibly smaller) limit; ties: the lowest slot
            int sl = -1;
            float bb = 0.0f;
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const bool in = ((m >> s) & 1u) != 0u && b[s] <= S.bound;
                if (in && (sl < 0 || b[s] < bb)) {
                    sl = s;
                    bb = b[s];
                }
            }
            if (sl < 0) break;
            m &= ~(1u << sl);  // (before the slot is tested or entered: a pushed mask holds untried slots only)
            if ((imask >> sl) & 1u) {
                if (m) {  // the rest of this level waits (re-tested against the limit of then)
                    if (sp >= WSTACK) {
                        err++;
                        return;
                    }
                    stk[(2 * sp) * BLOCK] = node;
                    stk[(2 * sp + 1) * BLOCK] = (int)m;
                    sp++;
                }
                node = cbase + __builtin_popcount(imask & ((1u << sl) - 1u));
                mask = 0xFFu;
                descended = true;
                break;
            }
            tct_leaf(W, Q, S, K, all, (unsigned)sl, m0, m1, tbase, gated, pairs);
        }
        if (descended) continue;
        if (sp == 0) return;
        --sp;
        node = stk[(2 * sp) * BLOCK];
        mask = (unsigned)stk[(2 * sp + 1) * BLOCK];
    }
}

// CAP: the list's capacity (0: counting only). STRICT: the exhaustive kernel.
template <int CAP, bool STRICT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(tct_waves(CAP, STRICT))))
void k_tricontacts(TCArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no stack)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    constexpr int REG = tct_reg(CAP, STRICT);
    unsigned long long* ovf = nullptr;
    if constexpr (CAP > REG) {
        __shared__ unsigned long long lds_ovf[(CAP - REG) * BLOCK];
        ovf = lds_ovf + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    const int K = A.max_tris;
    const bool all = A.count_all != 0;
    const bool want_pairs = A.out != nullptr || A.kind != nullptr;
    unsigned tris = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long stored = 0, counted = 0, nodes = 0, gated = 0, pairs = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long i = (long long)ch * QUERY_CHUNK + pass * 64 + (int)lane_now();
            if (i >= A.n) continue;
            tris++;
            const float* q = A.tris + 9 * i;
            const v3 q0 = mk(q[0], q[1], q[2]), q1 = mk(q[3], q[4], q[5]), q2 = mk(q[6], q[7], q[8]);
            const v3 d = mk(A.motion[3 * i], A.motion[3 * i + 1], A.motion[3 * i + 2]);
            const float tm = A.t_max ? A.t_max[i] : FMAX;
            // a non-finite corner or motion, a NaN or negative bound: the empty set, before any walk (k_trisweep's test)
            const bool valid = finite3(q0) && finite3(q1) && finite3(q2) && finite3(d) && tm >= 0.0f;
            const TSTri Q = tsw_query(q0, q1, q2, d);
            const float T = fminf(tm, FMAX);
            HState<CAP, REG> S;  // (S.bound is the walk's lim)
            hits_init(S, T, ovf);
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr && tsw_domain(q0, q1, q2, d, A.c_max);
                if (walk) tct_wide(A.s.wide, Q, S, K, all, stk, nodes, gated, pairs, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    tct_exhaustive(A.s, Q, S, K, STRICT || all);  // (the checker's limit is T throughout)
                    pairs += (unsigned long long)A.s.n_tris;
                }
            }
            exhc += exh;
            unsigned st = 0;
            if constexpr (CAP > 0) {
                const long long ob = i * K;
#pragma unroll
                for (int j = 0; j < CAP; j++) {
                    if (j < K) {
                        const unsigned long long k = hits_key(S, j);
                        const bool e = k == HKEY_EMPTY;
                        if (A.tri) A.tri[ob + j] = e ? -1 : (int)(unsigned)k;
                        if (A.t) A.t[ob + j] = e ? FMAX : __uint_as_float((unsigned)(k >> 32));
                        st += e ? 0u : 1u;
                    }
                }
                if (want_pairs) {  // each stored entry's own point and kind: the gate and tsw_tri again, under T (header)
#pragma unroll 1
                    for (int j = 0; j < K; j++) {
                        unsigned long long k = HKEY_EMPTY;
                        if constexpr (REG > 0) {
#pragma unroll
                            for (int u = 0; u < REG; u++) k = u == j ? S.key[u] : k;
                        }
                        if constexpr (CAP > REG) {
                            if (j >= REG) k = ovf[(j - REG) * BLOCK];
                        }
                        v3 pt = q0;  // (an unused slot: q0's own bits, kind -1)
                        int kind = -1;
                        if (k != HKEY_EMPTY) {
                            const float4* __restrict__ rec = A.s.ref.tris + 3 * A.ref_inv[(unsigned)k];
                            const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
                            const v3 a = mk(w0.x, w0.y, w0.z), b = add(a, mk(w0.w, w1.x, w1.y)),
                                     c = add(a, mk(w1.z, w1.w, w2.x));
                            float t0, toi;
                            (void)tsw_gate(Q, vmin3(a, b, c), vmax3(a, b, c), T, t0);
                            (void)tsw_tri(Q, rec, t0, T, toi, pt, kind);
                        }
                        if (A.out) {
                            float* o = A.out + 3 * (ob + j);
                            o[0] = pt.x;
                            o[1] = pt.y;
                            o[2] = pt.z;
                        }
                        if (A.kind) A.kind[ob + j] = kind;
                    }
                }
            }
            const unsigned cnt = all ? S.total : st;
            if (A.count) A.count[i] = (int)cnt;
            found += S.total != 0u;
            empty += S.total == 0u;
            stored += st;
            counted += cnt;
        }
    }
    const unsigned v[TC_NCOUNT] = {tris, found, 0u, 0u, walked, exhc, empty, 0u, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < TC_NCOUNT; k++) {
        if (k == TC_STORED || k == TC_COUNTED || k == TC_NODES || k == TC_GATED || k == TC_PAIRS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted), n64 = wave_sum64(nodes),
                             g64 = wave_sum64(gated), p64 = wave_sum64(pairs);
    if (lane == 0 && s64) atomicAdd(A.counters + TC_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + TC_COUNTED, c64);
    if (lane == 0 && n64) atomicAdd(A.counters + TC_NODES, n64);
    if (lane == 0 && g64) atomicAdd(A.counters + TC_GATED, g64);
    if (lane == 0 && p64) atomicAdd(A.counters + TC_PAIRS, p64);
}

}  // namespace rtd
