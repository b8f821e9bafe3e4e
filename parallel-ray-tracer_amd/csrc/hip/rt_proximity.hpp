// rt_proximity.hpp — proximity queries: the k nearest mesh triangles of each caller-supplied triangle, their squared
// distances and pairs of closest points, and the number of mesh triangles within a margin (rt_proximity_triangles,
// rt_hip.h): rt_clearance_triangles' plural form, as rt_neighbours.hpp is rt_nearest_points'.
//
// Query i is a triangle q0, q1, q2 with an optional bound max_dist2[i]. Its candidate set is clearance's own,
//   S_i = { j : D(q, record j) <= min(max_dist2[i], FLT_MAX) }
// ordered by (D ascending, original triangle index ascending), D, the pair of points and the kind as rt_clearance.hpp's
// clear_tri computes them: called here, not restated. D of a pair depends on the query and the record alone, on no limit
// a walk holds, so a pair has the same bits wherever and whenever it is evaluated. The answer is the first max_tris
// entries of S_i and min(|S_i|, max_tris), or |S_i| itself with count_all; the list form writes members of S_i into the
// caller's CSR segments (rt_cut.hpp's rules). A total order, so the answer depends on no view, lane or visiting order.
//
// The per-query list is rt_hits.hpp's HState, filled by rt_neighbours.hpp's neighbours_take: up to CAP 64-bit keys
// D_bits << 32 | original index (D >= +0: one unsigned compare is the lexicographic one), kept sorted. Where the keys
// live, and the occupancy, are chosen per build (prox_reg and prox_waves below): clearance's walk
// already sits at the register cap of three waves per SIMD, and the list takes the place of the answer's points and kind.
//
// Two kernels of k_clearance's skeleton (persistent waves, QUERY_CHUNK queries per returning atomic, one query per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig, no
//                     pre-gate; each D within the bound is counted and offered to the list. The checker.
//   RT_KERNEL_FAST    clear_wide's walk (slot_box_bound, the per-level two-word LDS stack, reload and re-prune on a pop,
//                     leaf slots first) with the list's limit as neighbours_wide has it: lim = min(the query's bound,
//                     the max_tris-th stored D once the list is full). With count_all, and in the list form, whose
//                     segments take members beyond the max_tris-th, lim is the query's bound alone for the whole walk:
//                     without a bound that is a full traversal. A slot is dropped only when its bound is STRICTLY
//                     greater than lim. A record of a kept leaf slot is skipped (pairs_gated) when the bound of its own
//                     corner box exceeds lim, or when the list is full, lim follows the list, and the least key the
//                     record could have, bound_bits << 32 | index, exceeds the list's last key: pure pruning. A scene
//                     without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
//
// Why nothing that belongs in the answer is pruned. rt_clearance.hpp's argument gives: the COMPUTED bound of a record's
// own corner box and of every slot box on its path is <= the record's COMPUTED D, with no margin. lim never grows during
// a walk and the final max_tris-th D is <= every earlier lim. A record that belongs in the list has D <= the final
// max_tris-th D (or <= the query's bound, where lim is the bound alone), hence D <= lim at every moment, hence every
// bound on its path <= lim: it is reached whatever was found before it. The key gate: a record's key is at least
// bound_bits << 32 | index (D >= its bound >= +0 and non-negative floats order as their bits), so one whose least key
// exceeds the list's last key cannot enter the full list, and no count depends on it since lim follows the list only
// without count_all.
//
// Each triangle at most once per query. A repeated offer would duplicate an entry or inflate a count. rt_neighbours.hpp's
// (a)-(c) carry over because the walk is leaf-first: (a) the wide view holds each triangle in exactly one leaf slot;
// (b) a node's leaf slots are tested at the node's first visit only -- every leaf slot within the limit is tested before
// anything is pushed, and the pushed mask is m & imask, interior slots only, so a pop offers no leaf again; (c) an
// interior slot leaves m before its child is entered, so a child is entered at most once.
//
// The list holds keys, not points. When on_query, on_mesh or kind is asked for, clear_tri is evaluated again after the
// walk for each stored entry, on the record of the REFERENCE tree found through ref_inv (rt_neighbours.hpp). Every
// view's records are made from the same coordinates by the same code, so that record holds the bits the walk read and
// the pair has the walk's bits. The list form's writes happen at acceptance, where the pair's points are live.
//
// LDS: the walk's 2 x WSTACK ints of the per-level stack in the STACK-int column (34,816 B per workgroup), plus the
// overflow column of CAP - REG keys per lane in the builds that have one (prox_reg below).
#pragma once
#include "rt_clearance.hpp"
#include "rt_neighbours.hpp"

namespace rtd {

constexpr int PROXIMITY_MAX = 16;  // RT_PROXIMITY_MAX
enum { PX_TRIS, PX_FOUND, PX_STORED, PX_COUNTED, PX_LISTED, PX_WALKED, PX_EXH, PX_EMPTY, PX_NODES, PX_GATED, PX_PAIRS,
       PX_ERR, PX_NCOUNT };

struct PXArgs {
    DScene s;
    const float* tris;       // [n][3][3]
    const float* max_dist2;  // nullable
    const int* offsets;      // [n + 1], nullable (with list)
    int* tri;                // [n][max_tris], nullable
    float* d2;               // [n][max_tris], nullable
    float* on_query;         // [n][max_tris][3], nullable
    float* on_mesh;          // [n][max_tris][3], nullable
    int* kind;               // [n][max_tris], nullable
    int* count;              // [n], nullable
    int* list;               // nullable (with offsets)
    float* list_d2;          // [offsets[n]], nullable (only with list)
    float* list_points;      // [offsets[n]][2][3], nullable (only with list)
    int* list_kind;          // [offsets[n]], nullable (only with list)
    const int* ref_inv;      // original triangle index -> position in s.ref.tris (read only for the points and kinds)
    unsigned long long* counters;  // PX_NCOUNT slots of the proximity query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    int max_tris;
    int count_all;
    int pad;
};
static_assert(sizeof(PXArgs) == sizeof(DScene) + 16 * 8 + 16, "kernel-argument layout: both passes must agree");

// Where a build's keys live, from the code object's figures. prox_reg of the CAP keys are in registers,
// the other CAP - prox_reg in the lane's LDS column. Beside clearance's walk (168 VGPRs, the cap of three waves per SIMD)
// no placement of 4, 8 or 16 keys is free of scratch, not even all of them in LDS; so the walk's list builds are
// compiled for two waves per SIMD and keep rt_hits.hpp's placement (8 in registers, keys 9..16 in LDS). The counting
// walk has no list and stays at three. The exhaustive kernels have no walk and stay at three with 4 keys in registers
// and the rest in LDS.
constexpr int prox_reg(int cap, bool strict) { return strict ? (cap <= 4 ? cap : 4) : hits_reg(cap, false); }
constexpr int prox_waves(int cap, bool strict) { return !strict && cap > 0 ? 2 : 3; }

// the list form's segments and the outputs of one member
struct PXList {
    const int* offsets;
    int* list;
    float* d2;
    float* points;
    int* kind;
};

// query i's segment [first, end) of the list (an entry that decreases, or a negative one: a segment of no length)
__device__ __forceinline__ void prox_segment(const int* __restrict__ offsets, long long i, long long& first,
                                             long long& end) {
    const long long a = offsets[i], b = offsets[i + 1];
    first = a;
    end = a >= 0 && b > a ? b : a;
}

// one pair's D: a member of S_i is written to query i's segment while it has room (the segment is read again here, not
// held across the walk: its four registers are what the walk lacks), counted and offered to the list (neighbours_take;
// `wide`: lim stays the query's bound)
template <class ST>
__device__ __forceinline__ void prox_take(ST& S, float D, v3 pq, v3 pm, int kind, int orig, int K, bool wide,
                                          const PXList& L, long long i) {
    if (L.list && D <= S.bound) {  // (wide whenever there is a list: S.bound is the query's bound)
        long long at, end;
        prox_segment(L.offsets, i, at, end);
        at += (long long)S.total;
        if (at < end) {
            L.list[at] = orig;
            if (L.d2) L.d2[at] = D;
            if (L.points) {
                float* o = L.points + 6 * at;
                o[0] = pq.x;
                o[1] = pq.y;
                o[2] = pq.z;
                o[3] = pm.x;
                o[4] = pm.y;
                o[5] = pm.z;
            }
            if (L.kind) L.kind[at] = kind;
        }
    }
    neighbours_take(S, D, orig, K, wide);
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform), no pre-gate
template <class ST>
__device__ __forceinline__ void prox_exhaustive(const DScene& s, const CLTri& Q, ST& S, int K, bool wide,
                                                const PXList& L, long long i) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        v3 pq, pm;
        int kind;
        const float D = clear_tri(Q, s.ref.tris + 3 * j, pq, pm, kind);
        prox_take(S, D, pq, pm, kind, s.ref.tri_orig[j], K, wide, L, i);
    }
}

// leaf slot sl's 1..4 records (meta = count << 5 | offset): clear_leaf's gate with the list's last key in the place of
// the best key (header), then tested and offered
template <class ST>
__device__ __forceinline__ void prox_leaf(const DWide& W, const CLTri& Q, ST& S, int K, bool wide, const PXList& L,
                                          long long qi, unsigned sl, unsigned m0, unsigned m1, int tbase,
                                          unsigned long long& gated, unsigned long long& pairs) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
#pragma unroll 1
    for (int i = first; i < first + cnt; i++) {
        const float4* __restrict__ tri = W.tris + 3 * i;
        const float4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
        const v3 a = mk(t0.x, t0.y, t0.z), b = add(a, mk(t0.w, t1.x, t1.y)), c = add(a, mk(t1.z, t1.w, t2.x));
        const float bnd = box_bound(Q.lo, Q.hi, vmin3(a, b, c), vmax3(a, b, c));
        const int orig = W.tri_orig[i];
        // (S.kth is HKEY_EMPTY until the first K slots are full: no key exceeds it)
        if (bnd > S.bound || (!wide && (((unsigned long long)__float_as_uint(bnd) << 32) | (unsigned)orig) > S.kth)) {
            gated++;
            continue;
        }
        v3 pq, pm;
        int kind;
        pairs++;
        const float D = clear_tri(Q, tri, pq, pm, kind);
        prox_take(S, D, pq, pm, kind, orig, K, wide, L, qi);
    }
}

// clear_wide's walk with the list's limit S.bound in the place of min(bound, best D) (header)
template <class ST>
__device__ __forceinline__ void prox_wide(const DWide& W, const CLTri& Q, ST& S, int K, bool wide, const PXList& L,
                                          long long qi, int* __restrict__ stk, unsigned long long& nodes, unsigned long long& gated,
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
        unsigned m = 0u;  // the slots still to try: in the entry's mask, occupied, bound <= lim
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int j = s >> 1, sh = 16 * (s & 1);
            b[s] = slot_box_bound(Q.lo, Q.hi, p, sc, wx[j] >> sh, wy[j] >> sh, wz[j] >> sh);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            if (((mask >> s) & 1u) && occ && b[s] <= S.bound) m |= 1u << s;
        }
        {  // every leaf slot still within the limit, in slot order, before any interior child; none is pushed
            unsigned lh = m & ~imask;
            m &= imask;
            while (lh) {
                const unsigned sl = (unsigned)__builtin_ctz(lh);
                lh &= lh - 1u;
                float bs = b[0];
#pragma unroll
                for (int s = 1; s < 8; s++) bs = sl == (unsigned)s ? b[s] : bs;
                if (!(bs <= S.bound)) continue;
                prox_leaf(W, Q, S, K, wide, L, qi, sl, m0, m1, tbase, gated, pairs);
            }
        }
        // the nearest remaining interior slot whose bound does not exceed the (possibly smaller) limit; ties: the
        // lowest slot
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
        if (sl >= 0) {
            m &= ~(1u << sl);  // (before the child is entered: a pushed mask holds slots not yet entered only)
            if (m) {           // the rest of this level waits (re-tested against the limit of then)
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
            continue;
        }
        if (sp == 0) return;
        --sp;
        node = stk[(2 * sp) * BLOCK];
        mask = (unsigned)stk[(2 * sp + 1) * BLOCK];
    }
}

// CAP: the list's capacity (0: counting only). STRICT: the exhaustive kernel.
template <int CAP, bool STRICT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(prox_waves(CAP, STRICT))))
void k_proximity(PXArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no LDS)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    constexpr int REG = prox_reg(CAP, STRICT);
    unsigned long long* ovf = nullptr;
    if constexpr (CAP > REG) {
        __shared__ unsigned long long lds_ovf[(CAP - REG) * BLOCK];
        ovf = lds_ovf + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    const int K = A.max_tris;
    const bool all = A.count_all != 0;
    const bool wide = all || A.list != nullptr;  // lim is the query's bound alone (header)
    const PXList L = {A.offsets, A.list, A.list_d2, A.list_points, A.list_kind};
    const bool want_pairs = A.on_query != nullptr || A.on_mesh != nullptr || A.kind != nullptr;
    unsigned tris = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long stored = 0, counted = 0, listed = 0, nodes = 0, gated = 0, pairs = 0;
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
            const float md = A.max_dist2 ? A.max_dist2[i] : FMAX;
            // a NaN or negative bound, a non-finite corner: the empty set, before any walk
            const bool valid = md >= 0.0f && finite3(q0) && finite3(q1) && finite3(q2);
            const CLTri Q = clear_query(q0, q1, q2);
            HState<CAP, REG> S;  // (S.bound is the walk's lim)
            hits_init(S, fminf(md, FMAX), ovf);
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr;
                if (walk) prox_wide(A.s.wide, Q, S, K, wide, L, i, stk, nodes, gated, pairs, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    prox_exhaustive(A.s, Q, S, K, wide, L, i);
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
                        if (A.d2) A.d2[ob + j] = e ? FMAX : __uint_as_float((unsigned)(k >> 32));
                        st += e ? 0u : 1u;
                    }
                }
                if (want_pairs) {  // the pair of every stored entry: clear_tri again, on the reference tree's record
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
                        v3 pq = q0, pm = q0;  // (an unused slot: q0's own bits, kind -1)
                        int kind = -1;
                        if (k != HKEY_EMPTY) (void)clear_tri(Q, A.s.ref.tris + 3 * A.ref_inv[(unsigned)k], pq, pm, kind);
                        if (A.on_query) {
                            float* o = A.on_query + 3 * (ob + j);
                            o[0] = pq.x;
                            o[1] = pq.y;
                            o[2] = pq.z;
                        }
                        if (A.on_mesh) {
                            float* o = A.on_mesh + 3 * (ob + j);
                            o[0] = pm.x;
                            o[1] = pm.y;
                            o[2] = pm.z;
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
            long long room = 0;
            if (A.list) {
                long long first, end;
                prox_segment(A.offsets, i, first, end);
                room = end - first;
            }
            listed += (unsigned long long)((long long)S.total < room ? (long long)S.total : room);
        }
    }
    const unsigned v[PX_NCOUNT] = {tris, found, 0u, 0u, 0u, walked, exhc, empty, 0u, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < PX_NCOUNT; k++) {
        if (k == PX_STORED || k == PX_COUNTED || k == PX_LISTED || k == PX_NODES || k == PX_GATED || k == PX_PAIRS)
            continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted), l64 = wave_sum64(listed),
                             n64 = wave_sum64(nodes), g64 = wave_sum64(gated), p64 = wave_sum64(pairs);
    if (lane == 0 && s64) atomicAdd(A.counters + PX_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + PX_COUNTED, c64);
    if (lane == 0 && l64) atomicAdd(A.counters + PX_LISTED, l64);
    if (lane == 0 && n64) atomicAdd(A.counters + PX_NODES, n64);
    if (lane == 0 && g64) atomicAdd(A.counters + PX_GATED, g64);
    if (lane == 0 && p64) atomicAdd(A.counters + PX_PAIRS, p64);
}

}  // namespace rtd
