// rt_contacts.hpp — contact queries: the k earliest contacts of each caller-supplied moving sphere with the mesh and the
// number of contacts (rt_sweep_contacts, rt_hip.h): rt_sweep_spheres' plural form, as rt_neighbours.hpp is
// rt_nearest_points' and rt_hits.hpp the closest hit's.
//
// Query i is rt_sweep_spheres' own (centre c + t d, radius r, 0 <= t <= T = fminf(t_max[i], FLT_MAX)) and so is its
// candidate set, in its order:
//   S_i = { j : toi(i, record j) exists and toi <= T }, ordered by (toi ascending, original triangle index ascending),
// empty under the sweep's rules (a non-finite c, d or r, r < 0, a NaN or negative t_max[i]; decided before any walk).
// toi is rt_sweep.hpp's sweep_tri, called and not restated. The answer is the first max_tris entries of S_i and
// min(|S_i|, max_tris), or |S_i| itself with count_all. That is a total order, so the answer depends on no view, lane or
// visiting order.
//
// toi of a pair does not depend on sweep_tri's tend argument: tend enters the gate as the first value of the interval's
// END (a1) alone, t0 is built from 0 and the plane times, and everything after the gate reads t0, never a1 or tend. tend
// only decides rejection -- the gate's a0 <= a1 and the last toi <= tend. So a record that is accepted under two
// different limits has the same toi bits under both, which is what lets the limit shrink during a walk.
//
// The per-sweep list is rt_hits.hpp's (HState): up to CAP 64-bit keys toi_bits << 32 | original index (toi >= +0: t0
// starts at +0 and only grows by fmaxf, u >= 0, so one unsigned compare is the lexicographic one), kept sorted, the
// first 8 in registers, keys 9..16 of the fast kernel's 16-key build in a per-lane LDS column. Insertion is
// rt_neighbours.hpp's neighbours_take on toi's keys. Instantiated for CAP = 0 (counting only), 4, 8 and 16; a request
// runs the smallest that holds max_tris.
//
// The limit: lim (S.bound) = fminf(T, the max_tris-th stored toi once the list is full), and T alone for the whole walk
// with count_all. It is handed to sweep_gate and sweep_tri in T's place, for slots and records alike.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK sweeps per returning atomic, one sweep per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig; each
//                     accepted toi is counted and offered to the list. The checker.
//   RT_KERNEL_FAST    sweep_wide's walk of the full wide view (per-level LDS stack entries (node, slots still to try),
//                     the node decoded again on a pop, slots taken in order of their gate t0, ties: the lowest slot)
//                     with the list's limit in the place of the best toi. A slot is kept while t0 <= lim and dropped
//                     only when t0 is STRICTLY greater. A scene without a wide view (RT_ACCEL_REFERENCE) and a sweep
//                     outside sweep_domain run the exhaustive loop under either kernel (exhaustive_spheres).
// contacts_wide is a sibling of sweep_wide, not a generalisation of it: rt_sweep.hpp is untouched, so k_sweep compiles
// to the code it had.
//
// Why the answer is the definition's, in two parts.
// 1. Nothing that belongs is pruned. lim never grows during a walk: it starts at T and is only ever replaced by the
//    max_tris-th key's toi, which an insertion can only lower; with count_all it stays T. So the final max_tris-th toi
//    is <= every earlier lim. A member of the answer has toi <= the final max_tris-th toi (or <= T, with count_all or a
//    list that never fills), hence toi <= lim at every moment. By (P1) of rt_sweep.hpp its own gate t0 <= toi <= lim. By
//    (P2) every slot on its path has t0(slot) <= t0(record) and a gate interval that contains the record's: with the
//    interval's end clipped to lim >= toi >= t0(record), neither the slot's interval nor the record's is empty, and
//    t0(slot) <= lim. So no slot on its path is dropped (the drop needs an empty interval or t0 > lim), whatever was
//    found before, and sweep_tri under lim accepts the record with the toi it has under T (above). An entry that ties
//    the k-th toi with a lower index has toi == lim: it is still reached (<=), its key is smaller, and it displaces the
//    k-th.
// 2. Each record is offered at most once per sweep; a repeated offer would duplicate an entry or inflate a count. The
//    walk relies on all of: (a) the wide view holds each record in exactly one leaf slot (tests/test_gpu_hits.py checks
//    the views' tri_orig for duplicates); (b) a slot leaves the level's mask m before it is tested or entered, and a
//    stack entry's mask is that m, so it holds only untried slots: a pop neither tests a leaf slot nor enters a child
//    again; (c) the entry mask of a freshly entered node is all eight slots, and a child is entered only from its one
//    parent slot, hence once. The exhaustive loop offers record j at step j. The count tests of
//    tests/test_gpu_contacts.py (count_all counts equal to the yardstick's on every sweep; every triangle twice gives
//    exactly twice) pin this.
//
// The point output. The list holds keys, not Ps. After the walk P is recomputed for each stored entry by nearest_tri at
// the centre c + d*toi_j on the triangle's record of the REFERENCE tree, found through ref_inv (rt_neighbours.hpp: every
// view's records hold the same bits, so P has the bits k_sweep's point has). An unused slot holds c's own bits.
//
// LDS: the 2 x WSTACK ints of the per-level stack in the STACK-int column (34 KB per workgroup), plus the 8-key overflow
// column (16 KB) in the fast capacity-16 build: k_neighbours' budget. The exhaustive kernel holds no LDS.
#pragma once
#include "rt_neighbours.hpp"
#include "rt_sweep.hpp"

namespace rtd {

constexpr int CONTACTS_MAX = 16;  // RT_CONTACTS_MAX
enum { CT_SPHERES, CT_FOUND, CT_STORED, CT_COUNTED, CT_WALKED, CT_EXH, CT_EMPTY, CT_NODES, CT_TRIS, CT_ERR, CT_NCOUNT };

struct CArgs {
    DScene s;
    const float* centre;
    const float* motion;
    const float* radius;
    const float* t_max;  // nullable
    int* tri;            // [n][max_tris], nullable
    float* t;            // [n][max_tris], nullable
    float* out;          // [n][max_tris][3], nullable
    int* count;          // [n], nullable
    const int* ref_inv;  // original triangle index -> position in s.ref.tris (read only when out is set)
    unsigned long long* counters;  // CT_NCOUNT slots of the contacts query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    float c_max;  // sweep_domain's bound (SWArgs::c_max)
    int max_tris;
    int count_all;
};
static_assert(sizeof(CArgs) == sizeof(DScene) + 11 * 8 + 16, "kernel-argument layout: both passes must agree");

// one record's toi for the sweep under the list's limit: counted when in S_i, inserted when it sorts before the K-th
template <class ST>
__device__ __forceinline__ void contacts_take(ST& S, const SSphere& Q, const float4* __restrict__ rec, int orig, int K,
                                              bool all) {
    float toi;
    if (!sweep_tri(Q, rec, S.bound, toi)) return;
    neighbours_take(S, toi, orig, K, all);
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
template <class ST>
__device__ __forceinline__ void contacts_exhaustive(const DScene& s, const SSphere& Q, ST& S, int K, bool all) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) contacts_take(S, Q, s.ref.tris + 3 * j, s.ref.tri_orig[j], K, all);
}

// leaf slot sl's 1..4 records (meta = count << 5 | offset), each tested and offered to the list
template <class ST>
__device__ __forceinline__ void contacts_leaf(const DWide& W, const SSphere& Q, ST& S, int K, bool all, unsigned sl,
                                              unsigned m0, unsigned m1, int tbase, unsigned long long& tris) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
    for (int i = first; i < first + cnt; i++) {
        tris++;
        contacts_take(S, Q, W.tris + 3 * i, W.tri_orig[i], K, all);
    }
}

// sweep_wide's walk with the list's limit S.bound in the place of the best toi (header)
template <class ST>
__device__ __forceinline__ void contacts_wide(const DWide& W, const SSphere& Q, ST& S, int K, bool all,
                                              int* __restrict__ stk, unsigned long long& nodes,
                                              unsigned long long& tris, unsigned& err) {
    const gnodes nbase = walk_base(W.nodes);
    int node = 0, sp = 0;
    unsigned mask = 0xFFu;
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
            const bool open = sweep_gate(Q, L, H, S.bound, b[s]);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            if (((mask >> s) & 1u) && occ && open) m |= 1u << s;
        }
        bool descended = false;
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
            contacts_leaf(W, Q, S, K, all, (unsigned)sl, m0, m1, tbase, tris);
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
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(3)))
void k_contacts(CArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no LDS)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    constexpr int REG = hits_reg(CAP, STRICT);
    unsigned long long* ovf = nullptr;
    if constexpr (CAP > REG) {
        __shared__ unsigned long long lds_ovf[(CAP - REG) * BLOCK];
        ovf = lds_ovf + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    const int K = A.max_tris;
    const bool all = A.count_all != 0;
    unsigned spheres = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long stored = 0, counted = 0, nodes = 0, tris = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long i = (long long)ch * QUERY_CHUNK + pass * 64 + (int)lane_now();
            if (i >= A.n) continue;
            spheres++;
            const v3 c = mk(A.centre[3 * i], A.centre[3 * i + 1], A.centre[3 * i + 2]);
            const v3 d = mk(A.motion[3 * i], A.motion[3 * i + 1], A.motion[3 * i + 2]);
            const float r = A.radius[i];
            const float tm = A.t_max ? A.t_max[i] : FMAX;
            // a non-finite c, d or r, r < 0, a NaN or negative bound: the empty set, before any walk (k_sweep's test)
            const bool valid = finite3(c) && finite3(d) && r >= 0.0f && r <= FMAX && tm >= 0.0f;
            const SSphere Q = sweep_sphere(c, d, r);
            HState<CAP, REG> S;
            hits_init(S, fminf(tm, FMAX), ovf);
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr && sweep_domain(c, d, r, A.c_max);
                if (walk) contacts_wide(A.s.wide, Q, S, K, all, stk, nodes, tris, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    contacts_exhaustive(A.s, Q, S, K, all);
                    tris += (unsigned long long)A.s.n_tris;
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
                if (A.out) {  // each entry's contact point: nearest_tri at c + d*toi_j on the reference tree's record
#pragma unroll 1
                    for (int j = 0; j < K; j++) {
                        unsigned long long k = HKEY_EMPTY;
#pragma unroll
                        for (int u = 0; u < CAP; u++) k = u == j ? hits_key(S, u) : k;
                        v3 P = c;  // (an unused slot: c's own bits)
                        if (k != HKEY_EMPTY) {
                            const float toi = __uint_as_float((unsigned)(k >> 32));
                            (void)nearest_tri(add(c, mul(d, toi)), A.s.ref.tris + 3 * A.ref_inv[(unsigned)k], P);
                        }
                        float* o = A.out + 3 * (ob + j);
                        o[0] = P.x;
                        o[1] = P.y;
                        o[2] = P.z;
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
    const unsigned v[CT_NCOUNT] = {spheres, found, 0u, 0u, walked, exhc, empty, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < CT_NCOUNT; k++) {
        if (k == CT_STORED || k == CT_COUNTED || k == CT_NODES || k == CT_TRIS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted), n64 = wave_sum64(nodes),
                             t64 = wave_sum64(tris);
    if (lane == 0 && s64) atomicAdd(A.counters + CT_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + CT_COUNTED, c64);
    if (lane == 0 && n64) atomicAdd(A.counters + CT_NODES, n64);
    if (lane == 0 && t64) atomicAdd(A.counters + CT_TRIS, t64);
}

}  // namespace rtd
