// rt_nearest.hpp — nearest-surface queries: the closest triangle and the closest point on it, per caller-supplied point
// (rt_nearest_points, rt_hip.h).
//
// For point q (optional bound max_dist2[i]) the candidate set is
//   S_i = { j : D(q, triangle j) <= min(max_dist2[i], FLT_MAX) }
// ordered by (D ascending, original triangle index ascending); the answer is its first element. That is a total order,
// so the answer depends on no view, lane or visiting order.
//
// D and the closest point P are defined on what a triangle RECORD holds (a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)), so
// every vertex update already refits them. nearest_tri below is Ericson's region algorithm (Real-Time Collision
// Detection 5.1.5), every operation one float32 operation, dot as vec.c's x*x + y*y + z*z left to right, nothing
// contracted (the library's build: -ffp-contract=off, IEEE division, subnormals kept, IEEE fminf / fmaxf), with one
// addition: p is clamped, per component, into the box of the record's corners a, fl(a + e1), fl(a + e2):
//   P = fminf(fmaxf(p, lo), hi)     (a NaN operand loses)
// The clamp makes P finite for every finite record -- a degenerate triangle's 0 / 0 becomes a corner of its box, which
// need not lie on the triangle -- and it is what lets the walk prune with no tuned margin (below). The one division of
// a region is shared: the numerator and denominator the region names are selected first and divided once, which is the
// region's own operation on the region's own operands. tests/nearest_ref.py restates all of it in numpy float32.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK points per returning atomic, one point per lane):
//   RT_KERNEL_STRICT  exhaustive: every lane's point against every record of s.ref.tris in stored order (a wave-uniform
//                     loop: the record loads broadcast), indices through s.ref.tri_orig; keeps the smallest 64-bit key
//                     D_bits << 32 | index (D >= 0: one unsigned compare is the lexicographic one). The checker.
//   RT_KERNEL_FAST    walks the full wide view s.wide only (the unit and primary views are subsets of it). Per node the
//                     8 child boxes are decoded and each child's lower bound computed; empty slots and slots whose bound
//                     is strictly greater than lim = min(the point's bound, the best D so far) are dropped -- a box
//                     whose bound EQUALS the best is still entered, so an equal D with a smaller index is found --; the
//                     remaining leaf slots' 1..4 triangles are tested with nearest_tri and offered to the key (each
//                     slot's bound compared with the limit of that moment), then the nearest remaining interior child
//                     is entered. A scene without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop.
//
// The stack. The wide trees are at most WSTACK = 16 levels deep and up to 7 siblings may wait at every level; a
// per-child stack with bounds does not fit LDS. An entry here is per LEVEL: two words (node, mask of slots still to
// try) in the existing STACK-int LDS column (2 * WSTACK = 32 <= STACK ints; the walk's LDS is k_hits' capacity-8
// build's 34 KB). An entry is pushed only while slots remain, so at most depth - 1 entries wait. On a pop the node is
// loaded and decoded again and its bounds are tested against the now smaller best: that reload is the pop-time prune
// (no child is ever entered whose bound exceeds the current best). The node word is a full int, so an entry holds any
// node index a view can have (no packed 2^24 bound applies, and no call falls back for the tree's size).
//
// The lower bound, and why it needs no margin. Per axis e = fmaxf(fmaxf(lo - q, q - hi), 0) with lo, hi the child box's
// planes decoded as the builders decode them (fmaf(2^e, 1024 + qplane, p), rt_quant.hpp decode); the bound is
// e.x*e.x + e.y*e.y + e.z*e.z left to right with no FMA -- the same three products and two sums as D.
//   - P is clamped into the box of the record's corners a, fl(a + e1), fl(a + e2).
//   - That box lies inside the decoded box of every slot on the triangle's path: a slot's planes are the exact extent
//     of its triangles' VERTICES moved outward by the inflation (2^-16 of the scene's coordinate magnitude mx = 256 ulp
//     of mx) and then quantised outward with the very decode used here (quantise_axis checks decode(q) <= lo and
//     decode(q) >= hi), so the decode adds nothing to undo; fl(a + fl(v1 - v0)) differs from v1 by at most two roundings
//     at magnitudes <= 2 mx, i.e. <= 2 ulp of mx against the 256.
//   - Hence |q - P| >= max(lo - q, q - hi, 0) per axis as real numbers.
//   - Float32 subtraction, multiplication and addition are monotone (and fl(P - q) = -fl(q - P)), so the COMPUTED bound
//     is <= the COMPUTED D, per axis term and in the left-to-right sums.
// So no triangle of S_i's head is ever pruned and the fast answer has the exhaustive one's bits; an overflowing bound
// (a far point) implies an overflowing D, which is in no S_i either way.
#pragma once
#include "rt_hits.hpp"

// PRT_NEAREST_LEAF_FIRST 1 (the default): a node's leaf slots within the limit are tested, in slot order, before its
// nearest interior child is entered, so the choice loop runs over interior slots only; 0: leaf and interior slots alike
// in order of their bounds. Same answers; measured in DESIGN.md §3p.
#ifndef PRT_NEAREST_LEAF_FIRST
#define PRT_NEAREST_LEAF_FIRST 1
#endif

namespace rtd {

enum { N_POINTS, N_FOUND, N_WALKED, N_EXH, N_EMPTY, N_NODES, N_TRIS, N_ERR, N_NCOUNT };

struct NArgs {
    DScene s;
    const float* point;
    const float* max_dist2;  // nullable
    int* tri;                // [n], nullable
    float* d2;               // [n], nullable
    float* out;              // [n][3], nullable
    unsigned long long* counters;  // N_NCOUNT slots of the nearest query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    int pad;
};
static_assert(sizeof(NArgs) == sizeof(DScene) + 7 * 8 + 8, "kernel-argument layout: both passes must agree");

__device__ __forceinline__ v3 vmin3(v3 a, v3 b, v3 c) {
    return mk(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z));
}
__device__ __forceinline__ v3 vmax3(v3 a, v3 b, v3 c) {
    return mk(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z));
}

// D(q, record) and the closest point P (header)
__device__ __forceinline__ float nearest_tri(v3 q, const float4* __restrict__ tri, v3& P) {
    const float4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
    const v3 a = mk(t0.x, t0.y, t0.z), e1 = mk(t0.w, t1.x, t1.y), e2 = mk(t1.z, t1.w, t2.x);
    const v3 ap = sub(q, a);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const v3 bp = sub(ap, e1);
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    const v3 cp = sub(ap, e2);
    const float d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float x = d4 - d3, y = d5 - d6;
    const v3 b = add(a, e1), c = add(a, e2);
    // the first region whose condition holds
    int r = 6;
    if (d1 <= 0.0f && d2 <= 0.0f) r = 0;
    else if (d3 >= 0.0f && d4 <= d3) r = 1;
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) r = 2;
    else if (d6 >= 0.0f && d5 <= d6) r = 3;
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) r = 4;
    else if (va <= 0.0f && x >= 0.0f && y >= 0.0f) r = 5;
    // the region's one division: d1 / (d1 - d3), d2 / (d2 - d6), x / (x + y) or 1 / ((va + vb) + vc)
    const float num = r == 2 ? d1 : r == 4 ? d2 : r == 5 ? x : 1.0f;
    const float den = r == 2 ? d1 - d3 : r == 4 ? d2 - d6 : r == 5 ? x + y : (va + vb) + vc;
    const float s = num / den;
    v3 p;
    if (r == 0) p = a;
    else if (r == 1) p = b;
    else if (r == 3) p = c;
    else if (r == 2) p = add(a, mul(e1, s));
    else if (r == 4) p = add(a, mul(e2, s));
    else if (r == 5) p = add(b, mul(sub(e2, e1), s));
    else p = add(add(a, mul(e1, vb * s)), mul(e2, vc * s));
    const v3 lo = vmin3(a, b, c), hi = vmax3(a, b, c);
    P = mk(fminf(fmaxf(p.x, lo.x), hi.x), fminf(fmaxf(p.y, lo.y), hi.y), fminf(fmaxf(p.z, lo.z), hi.z));
    const v3 df = sub(q, P);
    return dot(df, df);
}

// one point's answer so far: the smallest key D_bits << 32 | original index, its P, and the pruning limit
struct NState {
    unsigned long long key;
    v3 P;
    float bound;  // min(max_dist2, FLT_MAX): membership of S_i
    float lim;    // min(bound, the best D so far): the walk's prune
};
__device__ __forceinline__ void nearest_take(NState& S, float D, v3 P, int orig) {
    if (!(D <= S.bound)) return;  // (an overflowed or NaN D is in no S_i)
    const unsigned long long k = ((unsigned long long)__float_as_uint(D) << 32) | (unsigned)orig;
    if (k < S.key) {
        S.key = k;
        S.P = P;
        S.lim = D;
    }
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
__device__ __forceinline__ void nearest_exhaustive(const DScene& s, v3 q, NState& S) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        v3 P;
        const float D = nearest_tri(q, s.ref.tris + 3 * j, P);
        nearest_take(S, D, P, s.ref.tri_orig[j]);
    }
}

// slot s's lower bound on D: its decoded box against q (header)
__device__ __forceinline__ float slot_bound(v3 q, v3 p, v3 sc, unsigned wx, unsigned wy, unsigned wz) {
    const float lx = __builtin_fmaf(sc.x, (float)(QBIAS + (wx & 0xFFu)), p.x);
    const float hx = __builtin_fmaf(sc.x, (float)(QBIAS + ((wx >> 8) & 0xFFu)), p.x);
    const float ly = __builtin_fmaf(sc.y, (float)(QBIAS + (wy & 0xFFu)), p.y);
    const float hy = __builtin_fmaf(sc.y, (float)(QBIAS + ((wy >> 8) & 0xFFu)), p.y);
    const float lz = __builtin_fmaf(sc.z, (float)(QBIAS + (wz & 0xFFu)), p.z);
    const float hz = __builtin_fmaf(sc.z, (float)(QBIAS + ((wz >> 8) & 0xFFu)), p.z);
    const float ex = fmaxf(fmaxf(lx - q.x, q.x - hx), 0.0f);
    const float ey = fmaxf(fmaxf(ly - q.y, q.y - hy), 0.0f);
    const float ez = fmaxf(fmaxf(lz - q.z, q.z - hz), 0.0f);
    return ex * ex + ey * ey + ez * ez;
}
__device__ __forceinline__ float pow2_bits(unsigned e8) {  // 2^e of a node's signed exponent byte (-126 .. 110)
    return __uint_as_float((unsigned)((int)(signed char)e8 + 127) << 23);
}

// leaf slot sl's 1..4 triangles (meta = count << 5 | offset), each tested and offered to the key
__device__ __forceinline__ void nearest_leaf(const DWide& W, v3 q, NState& S, unsigned sl, unsigned m0, unsigned m1,
                                             int tbase, unsigned long long& tris) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
    for (int i = first; i < first + cnt; i++) {
        v3 P;
        const float D = nearest_tri(q, W.tris + 3 * i, P);
        tris++;
        nearest_take(S, D, P, W.tri_orig[i]);
    }
}

// the walk of the full wide view (header): per-level stack entries (node, slots still to try), nearest child first
__device__ __forceinline__ void nearest_wide(const DWide& W, v3 q, NState& S, int* __restrict__ stk,
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
            if (((mask >> s) & 1u) && occ && b[s] <= S.lim) m |= 1u << s;
        }
#if PRT_NEAREST_LEAF_FIRST
        {  // every leaf slot still within the limit, in slot order, before any interior child
            unsigned lh = m & ~imask;
            m &= imask;
            while (lh) {
                const unsigned sl = (unsigned)__builtin_ctz(lh);
                lh &= lh - 1u;
                float bs = b[0];
#pragma unroll
                for (int s = 1; s < 8; s++) bs = sl == (unsigned)s ? b[s] : bs;
                if (!(bs <= S.lim)) continue;
                nearest_leaf(W, q, S, sl, m0, m1, tbase, tris);
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
                const bool in = ((m >> s) & 1u) != 0u && b[s] <= S.lim;
                if (in && (sl < 0 || b[s] < bb)) {
                    sl = s;
                    bb = b[s];
                }
            }
            if (sl < 0) break;
            m &= ~(1u << sl);
            if (PRT_NEAREST_LEAF_FIRST || ((imask >> sl) & 1u)) {  // (leaf first: only interior slots are left)
                if (m) {  // the rest of this level waits (re-tested against the best of then)
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
            nearest_leaf(W, q, S, (unsigned)sl, m0, m1, tbase, tris);
        }
        if (descended) continue;
        if (sp == 0) return;
        --sp;
        node = stk[(2 * sp) * BLOCK];
        mask = (unsigned)stk[(2 * sp + 1) * BLOCK];
    }
}

// STRICT: the exhaustive kernel
template <bool STRICT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(3)))
void k_nearest(NArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no LDS)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    unsigned points = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long nodes = 0, tris = 0;
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
            NState S;
            S.key = HKEY_EMPTY;
            S.P = q;
            S.bound = fminf(md, FMAX);
            S.lim = S.bound;
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr;
                if (walk) nearest_wide(A.s.wide, q, S, stk, nodes, tris, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    nearest_exhaustive(A.s, q, S);
                    tris += (unsigned long long)A.s.n_tris;
                }
            }
            exhc += exh;
            const bool none = S.key == HKEY_EMPTY;
            if (A.tri) A.tri[i] = none ? -1 : (int)(unsigned)S.key;
            if (A.d2) A.d2[i] = none ? FMAX : __uint_as_float((unsigned)(S.key >> 32));
            if (A.out) {
                const v3 P = none ? q : S.P;  // (the empty set: q's own bits)
                A.out[3 * i] = P.x;
                A.out[3 * i + 1] = P.y;
                A.out[3 * i + 2] = P.z;
            }
            found += none ? 0u : 1u;
            empty += none ? 1u : 0u;
        }
    }
    const unsigned v[N_NCOUNT] = {points, found, walked, exhc, empty, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < N_NCOUNT; k++) {
        if (k == N_NODES || k == N_TRIS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long n64 = wave_sum64(nodes), t64 = wave_sum64(tris);
    if (lane == 0 && n64) atomicAdd(A.counters + N_NODES, n64);
    if (lane == 0 && t64) atomicAdd(A.counters + N_TRIS, t64);
}

}  // namespace rtd
