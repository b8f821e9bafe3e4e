// rt_neighbours.hpp — neighbour queries: the k nearest triangles of caller-supplied points and the number of triangles
// within a radius (rt_nearest_tris, rt_hip.h): rt_nearest_points' plural form, as rt_hits.hpp is the closest hit's.
//
// For point q (optional bound max_dist2[i]) the candidate set is rt_nearest_points' own,
//   S_i = { j : D(q, triangle j) <= min(max_dist2[i], FLT_MAX) }
// ordered by (D ascending, original triangle index ascending), D and P as rt_nearest.hpp's nearest_tri computes them
// (rt_hip.h states the sequence). The answer is the first max_tris entries of S_i and min(|S_i|, max_tris), or |S_i|
// itself with count_all. That is a total order, so the answer depends on no view, lane or visiting order.
//
// The per-point list is rt_hits.hpp's (HState): up to CAP 64-bit keys D_bits << 32 | original index (D >= 0: one
// unsigned compare is the lexicographic one), kept sorted, the first 8 in registers, keys 9..16 of the fast kernel's
// 16-key build in a per-lane LDS column. Instantiated for CAP = 0 (counting only), 4, 8 and 16; a request runs the
// smallest that holds max_tris.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK points per returning atomic, one point per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig; each
//                     accepted D is counted and offered to the list. The checker.
//   RT_KERNEL_FAST    nearest_wide's walk of the full wide view (per-level stack entries, nearest interior child first,
//                     the pop-time reload) with the list's limit: lim = min(the point's bound, the max_tris-th stored D
//                     once the list is full), and the point's bound alone for the whole walk with count_all. A slot is
//                     dropped only when its bound is STRICTLY greater than lim, so a triangle whose D equals the last
//                     kept entry's and whose index is smaller is still reached and displaces it. A scene without a wide
//                     view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
//
// Why nothing that belongs in the answer is pruned. rt_nearest.hpp's argument carries over unchanged: the COMPUTED
// bound of every slot on a triangle's path is <= the triangle's COMPUTED D, term by term and sum by sum, with no
// margin. lim never grows during a walk, and the final max_tris-th D is <= every earlier lim. A triangle that belongs
// in the list has D <= the final max_tris-th D (or <= the point's bound, with count_all), hence D <= lim at every
// moment of the walk, hence a slot bound <= lim on its whole path: it is reached whatever was found before it.
//
// Each triangle at most once per point. For k = 1 a repeated offer is harmless; here it would duplicate an entry or
// inflate a count. (a) The wide view holds each triangle in exactly one leaf slot (tests/test_gpu_hits.py checks the
// views' tri_orig for duplicates). (b) A node's leaf slots are tested at the node's first visit only: with
// PRT_NEAREST_LEAF_FIRST every leaf slot within the limit is tested before anything is pushed and the pushed mask is
// m & imask, interior slots only; without it a slot leaves m before it is tested or entered. Either way the mask of a
// stack entry holds untested slots only, so a pop offers no leaf again. (c) An interior slot leaves m before its child
// is entered, so a child is entered at most once and the walk visits each node's leaf slots once. The count tests of
// tests/test_gpu_neighbours.py (radius counts equal to the yardstick's on every point) pin this.
//
// The point output. The list holds keys, not Ps (16 x 3 floats per lane do not fit beside the walk). After the walk P
// is recomputed for each stored entry by the same nearest_tri on the triangle's record of the REFERENCE tree, found
// through ref_inv (original index -> position in s.ref.tris, built on the device on first use after an upload: that
// order changes under no refit or rebuild). Every view's records are made from the same coordinates by the same code
// (tri_records / k_tri_records: a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)), so the wide view's record and the
// reference tree's hold the same bits and P has the walk's bits.
//
// LDS: the 2 x WSTACK ints of the per-level stack in the STACK-int column (34 KB per workgroup), plus the 8-key
// overflow column (16 KB) in the fast capacity-16 build: k_hits' budget. The exhaustive kernel holds no LDS.
#pragma once
#include "rt_hits.hpp"
#include "rt_nearest.hpp"

namespace rtd {

constexpr int NEIGHBOURS_MAX = 16;  // RT_NEIGHBOURS_MAX
enum { B_POINTS, B_FOUND, B_STORED, B_COUNTED, B_WALKED, B_EXH, B_EMPTY, B_NODES, B_TRIS, B_ERR, B_NCOUNT };

struct BArgs {
    DScene s;
    const float* point;
    const float* max_dist2;  // nullable
    int* tri;                // [n][max_tris], nullable
    float* d2;               // [n][max_tris], nullable
    float* out;              // [n][max_tris][3], nullable
    int* count;              // [n], nullable
    const int* ref_inv;      // original triangle index -> position in s.ref.tris (read only when out is set)
    unsigned long long* counters;  // B_NCOUNT slots of the neighbours query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    int max_tris;
    int count_all;
    int pad;
};
static_assert(sizeof(BArgs) == sizeof(DScene) + 9 * 8 + 16, "kernel-argument layout: both passes must agree");

// one triangle's D for the point: counted when it is in S_i and inserted when it sorts before the K-th entry (hits_take's
// insertion on D's keys; S.bound is the walk's lim: the point's bound, then the K-th stored D once the first K slots
// are full -- never with count_all)
template <class ST>
__device__ __forceinline__ void neighbours_take(ST& S, float D, int orig, int K, bool all) {
    constexpr int CAP = ST::CAP, REG = ST::REG;
    if (!(D <= S.bound)) return;  // (an overflowed or NaN D is in no S_i)
    S.total++;
    if constexpr (CAP > 0) {
        const unsigned long long k0 = ((unsigned long long)__float_as_uint(D) << 32) | (unsigned)orig;
        if (k0 < S.kth) {
            unsigned long long k = k0;
#pragma unroll
            for (int j = 0; j < REG; j++) {  // sorted insertion; the largest key falls off the end
                const unsigned long long a = S.key[j];
                const bool lt = k < a;
                S.key[j] = lt ? k : a;
                k = lt ? a : k;
            }
            unsigned long long kth = HKEY_EMPTY;
            if constexpr (CAP > REG) {  // K > REG here (the smaller capacities serve the others): the K-th is in LDS
#pragma unroll 1
                for (int j = 0; j < CAP - REG && k != HKEY_EMPTY; j++) {
                    const unsigned long long a = S.ovf[j * BLOCK];
                    if (k < a) {
                        S.ovf[j * BLOCK] = k;
                        k = a;
                    }
                }
                kth = S.ovf[(K - 1 - REG) * BLOCK];
            } else {
#pragma unroll
                for (int j = 0; j < REG; j++) kth = j == K - 1 ? S.key[j] : kth;
            }
            S.kth = kth;
            if (!all && kth != HKEY_EMPTY) S.bound = __uint_as_float((unsigned)(kth >> 32));
        }
    }
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
template <class ST>
__device__ __forceinline__ void neighbours_exhaustive(const DScene& s, v3 q, ST& S, int K, bool all) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        v3 P;
        const float D = nearest_tri(q, s.ref.tris + 3 * j, P);
        neighbours_take(S, D, s.ref.tri_orig[j], K, all);
    }
}

// leaf slot sl's 1..4 triangles (meta = count << 5 | offset), each tested and offered to the list
template <class ST>
__device__ __forceinline__ void neighbours_leaf(const DWide& W, v3 q, ST& S, int K, bool all, unsigned sl, unsigned m0,
                                                unsigned m1, int tbase, unsigned long long& tris) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
    for (int i = first; i < first + cnt; i++) {
        v3 P;
        const float D = nearest_tri(q, W.tris + 3 * i, P);
        tris++;
        neighbours_take(S, D, W.tri_orig[i], K, all);
    }
}

// nearest_wide's walk with the list's limit S.bound in the place of the best D (header)
template <class ST>
__device__ __forceinline__ void neighbours_wide(const DWide& W, v3 q, ST& S, int K, bool all, int* __restrict__ stk,
                                                unsigned long long& nodes, unsigned long long& tris, unsigned& err) {
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
        unsigned m = 0u;  // the slots still to try: in the entry's mask, occupied, bound <= lim
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int j = s >> 1, sh = 16 * (s & 1);
            b[s] = slot_bound(q, p, sc, wx[j] >> sh, wy[j] >> sh, wz[j] >> sh);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            if (((mask >> s) & 1u) && occ && b[s] <= S.bound) m |= 1u << s;
        }
#if PRT_NEAREST_LEAF_FIRST
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
                neighbours_leaf(W, q, S, K, all, sl, m0, m1, tbase, tris);
            }
        }
#endif
        bool descended = false;
        for (;;) {
            // the nearest remaining slot whose bound does not exceed the (possibly smaller) limit; ties: the lowest slot
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
            m &= ~(1u << sl);  // (before the slot is tested or entered: a pushed mask holds untested slots only)
            if (PRT_NEAREST_LEAF_FIRST || ((imask >> sl) & 1u)) {  // (leaf first: only interior slots are left)
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
            neighbours_leaf(W, q, S, K, all, (unsigned)sl, m0, m1, tbase, tris);
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
void k_neighbours(BArgs A) {
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
    unsigned points = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long stored = 0, counted = 0, nodes = 0, tris = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long i = (long long)ch * QUERY_CHUNK + pass * 64 + (int)lane_now();
            if (i >= A.n) continue;
            points++;
            const v3 q = mk(A.point[3 * i], A.point[3 * i + 1], A.point[3 * i + 2]);
            const float md = A.max_dist2 ? A.max_dist2[i] : FMAX;
            // a NaN or negative bound, a non-finite point: the empty set, before any walk
            const bool valid = md >= 0.0f && finite3(q);
            HState<CAP, REG> S;
            hits_init(S, fminf(md, FMAX), ovf);
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr;
                if (walk) neighbours_wide(A.s.wide, q, S, K, all, stk, nodes, tris, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    neighbours_exhaustive(A.s, q, S, K, all);
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
                        if (A.d2) A.d2[ob + j] = e ? FMAX : __uint_as_float((unsigned)(k >> 32));
                        st += e ? 0u : 1u;
                    }
                }
                if (A.out) {  // P of every stored entry: nearest_tri again, on the reference tree's record (header)
#pragma unroll 1
                    for (int j = 0; j < K; j++) {
                        unsigned long long k = HKEY_EMPTY;
#pragma unroll
                        for (int u = 0; u < CAP; u++) k = u == j ? hits_key(S, u) : k;
                        v3 P = q;  // (an unused slot: q's own bits)
                        if (k != HKEY_EMPTY) (void)nearest_tri(q, A.s.ref.tris + 3 * A.ref_inv[(unsigned)k], P);
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
    const unsigned v[B_NCOUNT] = {points, found, 0u, 0u, walked, exhc, empty, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < B_NCOUNT; k++) {
        if (k == B_STORED || k == B_COUNTED || k == B_NODES || k == B_TRIS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted), n64 = wave_sum64(nodes),
                             t64 = wave_sum64(tris);
    if (lane == 0 && s64) atomicAdd(A.counters + B_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + B_COUNTED, c64);
    if (lane == 0 && n64) atomicAdd(A.counters + B_NODES, n64);
    if (lane == 0 && t64) atomicAdd(A.counters + B_TRIS, t64);
}

// ref_inv (header): inv[orig[j]] = j over the reference tree's records
__global__ void k_invert_orig(const int* __restrict__ orig, int n, int* __restrict__ inv) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) {
        const int o = orig[j];
        if (o >= 0 && o < n) inv[o] = j;
    }
}

}  // namespace rtd
