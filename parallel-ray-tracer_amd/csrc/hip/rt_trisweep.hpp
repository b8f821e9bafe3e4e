// rt_trisweep.hpp — triangle sweep queries: the first contact of each caller-supplied moving triangle with the mesh
// (rt_sweep_triangles, rt_hip.h): rt_clearance_triangles' motion form, as rt_sweep_spheres is a point query's.
//
// Query i is a triangle q0, q1, q2 that translates without rotating: its corners at time t are q + t d,
// 0 <= t <= T = fminf(t_max[i], FLT_MAX). Its answer is the first element of
//   S_i = { j : toi(i, record j) exists and <= T }, ordered by (toi ascending, original triangle index ascending),
// empty when one of the twelve numbers is non-finite or t_max[i] is NaN or negative (decided before any walk). That is
// a total order, so the answer depends on no view, lane or visiting order.
//
// toi is defined on what a triangle RECORD holds (a, e1, e2; corners a, b = fl(a + e1), c = fl(a + e2), corner box
// [tlo, thi]) and on the query made a record the same way (rt_clearance.hpp: f1, f2, qb, qc and the box [qlo, qhi] of the
// FIVE points). tsw_tri below is the sequence rt_hip.h states and tests/trisweep_ref.py restates in numpy float32, every
// operation one float32 operation, dot left to right, nothing contracted, IEEE division:
//   1. the gate: the interval of t in [0, T] at which the query's box, moved by t d, meets the record's corner box, by
//      slabs (one subtraction and one multiplication by the sweep's own 1 / d.k per plane); t0 is where it starts;
//   2. recentre: every query corner + d t0; f1 and f2 keep their bits;
//   3. a start in contact: cut_tri (unchanged) on the recentred raw corners holds -> toi = t0, kind 15, the cut
//      segment's first end;
//   4. else the least valid of fifteen candidates u >= 0 measured from t0, in clearance's order, a later one replacing
//      the best only when strictly smaller: the recentred query corners as rays along d against the mesh record (0..2),
//      the mesh corners as rays along -d against the recentred query record (3..5) -- one ray-triangle function,
//      tsw_ray --, and the nine edge pairs, query edge major (6..14), tsw_edge; toi = t0 + u.
// The contact point lies on the mesh triangle and is clamped into [tlo, thi].
//
// Why the walk needs no margin: rt_sweep.hpp's argument with the query's box in the sphere's place.
// (P1) toi >= t0: step 3 returns t0 and step 4 adds u >= 0. (P2) the gate is made of subtractions, one multiplication by
// a per-query constant, comparisons, fminf and fmaxf, all monotone in the mesh-side box planes, so tsw_gate on a box
// [L, H] that contains the record's corner box gives an interval that contains the record's and a t0 that is <= the
// record's, and is empty only if the record's is. The decoded slot boxes of the full wide view contain the corner box of
// every record below them (rt_nearest.hpp's header). Hence a slot whose interval is empty, or whose t0 is STRICTLY
// greater than the best toi so far, holds no record that precedes the best in the order; a slot whose t0 EQUALS the best
// is entered, so an equal toi with a lower index is found. The walk hands tsw_gate the current limit
// lim = fminf(T, best toi) in T's place, for slots and records alike: by (P1) a record that this turns away has
// toi >= t0 > lim and precedes nothing. t0 does not depend on the limit, so a pair's toi has the same bits in both
// kernels. Monotonicity fails only where the gate makes a NaN (0 * inf, inf - inf): tsw_domain keeps 1 / d.k finite and
// nonzero and every difference finite. A query outside it runs the exhaustive loop and counts in `exhaustive`.
//
// Two kernels of k_sweep's skeleton (persistent waves, QUERY_CHUNK queries per returning atomic, one query per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig; keeps the
//                     smallest key toi_bits << 32 | index. The checker.
//   RT_KERNEL_FAST    sweep_wide's walk: per-level LDS stack (node, slots still to try; decoded again on a pop), a
//                     node's slots, leaf and interior alike, in order of their gate t0 (ties: the lowest slot); a leaf
//                     slot's 1..4 records pass their own gate (else counted in pairs_gated) before tsw_tri. A scene
//                     without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
#pragma once
#include "rt_clearance.hpp"
#include "rt_sweep.hpp"

namespace rtd {

enum { TS_TRIS, TS_FOUND, TS_WALKED, TS_EXH, TS_EMPTY, TS_NODES, TS_GATED, TS_PAIRS, TS_ERR, TS_NCOUNT };

struct TSArgs {
    DScene s;
    const float* tris;    // [n][3][3]
    const float* motion;  // [n][3]
    const float* t_max;   // nullable
    int* tri;             // [n], nullable
    float* t;             // [n], nullable
    float* out;           // [n][3], nullable
    int* kind;            // [n], nullable
    unsigned long long* counters;  // TS_NCOUNT slots of the triangle sweep query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    float c_max;  // tsw_domain's bound on max|q| (2^20 x the scene's coordinate magnitude mx, rt_hip.hip)
};
static_assert(sizeof(TSArgs) == sizeof(DScene) + 9 * 8 + 8, "kernel-argument layout: both passes must agree");

// one query: its raw corners, its record, the five-point box, its motion and what every gate shares
struct TSTri {
    v3 q0, q1, q2, f1, f2, qb, qc, lo, hi;
    v3 d, inv;  // inv.k = 1 / d.k (unused where d.k == 0)
};
__device__ __forceinline__ TSTri tsw_query(v3 q0, v3 q1, v3 q2, v3 d) {
    TSTri Q;
    Q.q0 = q0;
    Q.q1 = q1;
    Q.q2 = q2;
    Q.f1 = sub(q1, q0);
    Q.f2 = sub(q2, q0);
    Q.qb = add(q0, Q.f1);
    Q.qc = add(q0, Q.f2);
    const v3 l = vmin3(q0, q1, q2), h = vmax3(q0, q1, q2);
    Q.lo = vmin3(l, Q.qb, Q.qc);
    Q.hi = vmax3(h, Q.qb, Q.qc);
    Q.d = d;
    Q.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    return Q;
}

// The walk's domain: every |q| <= c_max = 2^20 mx and every NONZERO |d.k| in [2^-64, 2^64]. Then 1 / d.k is finite,
// normal and nonzero, every plane difference lo - qhi, hi - qlo is finite for planes within 2 mx, and the gate's
// products are a finite number times a finite nonzero one: no NaN, which is all (P2) needs (an overflow to +-inf keeps
// the order).
__device__ __forceinline__ bool tsw_domain(v3 q0, v3 q1, v3 q2, v3 d, float c_max) {
    return sweep_domain(q0, d, 0.0f, c_max) && maxabs(q1) <= c_max && maxabs(q2) <= c_max;
}

// step 1 on the box [lo, hi]: the interval of t in [0, tend] at which [qlo, qhi] + t d meets [lo, hi]; false when
// empty. An axis with d.k == 0 contributes the overlap of the two boxes on it alone. One formula for records and slots.
__device__ __forceinline__ bool tsw_gate(const TSTri& Q, v3 lo, v3 hi, float tend, float& t0) {
    float a0 = 0.0f, a1 = tend;
    bool in = true;
    {
        const bool z = Q.d.x == 0.0f;
        const float ta = (lo.x - Q.hi.x) * Q.inv.x, tb = (hi.x - Q.lo.x) * Q.inv.x;
        a0 = fmaxf(a0, z ? a0 : fminf(ta, tb));
        a1 = fminf(a1, z ? a1 : fmaxf(ta, tb));
        in = in && (!z || (Q.lo.x <= hi.x && lo.x <= Q.hi.x));
    }
    {
        const bool z = Q.d.y == 0.0f;
        const float ta = (lo.y - Q.hi.y) * Q.inv.y, tb = (hi.y - Q.lo.y) * Q.inv.y;
        a0 = fmaxf(a0, z ? a0 : fminf(ta, tb));
        a1 = fminf(a1, z ? a1 : fmaxf(ta, tb));
        in = in && (!z || (Q.lo.y <= hi.y && lo.y <= Q.hi.y));
    }
    {
        const bool z = Q.d.z == 0.0f;
        const float ta = (lo.z - Q.hi.z) * Q.inv.z, tb = (hi.z - Q.lo.z) * Q.inv.z;
        a0 = fmaxf(a0, z ? a0 : fminf(ta, tb));
        a1 = fminf(a1, z ? a1 : fmaxf(ta, tb));
        in = in && (!z || (Q.lo.z <= hi.z && lo.z <= Q.hi.z));
    }
    t0 = a0;
    return in && a0 <= a1;
}

// one pair's best candidate so far
struct TSPair {
    float u;
    v3 pt;
    int kind;
};
__device__ __forceinline__ void tsw_offer(TSPair& R, float u, v3 pt, int kind) {
    if (u < R.u) {
        R.u = u;
        R.pt = pt;
        R.kind = kind;
    }
}

// candidates 0..5: the ray o + u dr against the record (a, e1, e2), with no EPSILON culls (header)
__device__ __forceinline__ bool tsw_ray(v3 o, v3 dr, v3 a, v3 e1, v3 e2, float& u) {
    const v3 h = cut_cross(dr, e2);
    const float det = dot(e1, h);
    const float inv = 1.0f / det;
    const v3 s = sub(o, a);
    const float bu = dot(s, h) * inv;
    const v3 qv = cut_cross(s, e1);
    const float bv = dot(dr, qv) * inv;
    u = dot(e2, qv) * inv;
    return det != 0.0f && bu >= 0.0f && bv >= 0.0f && bu + bv <= 1.0f && u >= 0.0f;
}

// candidates 6..14: the query edge (p, f) moving along d against the mesh edge (m, e) (header). The two edge parameters
// are needed only for a u that would replace the best: a skipped one changes nothing.
__device__ __forceinline__ void tsw_edge(v3 p, v3 f, v3 m, v3 e, v3 d, TSPair& R, int kind) {
    const v3 n = cut_cross(f, e);
    const float nn = dot(n, n), dn = dot(d, n);
    const v3 w0 = sub(m, p);
    const float u = dot(w0, n) / dn;
    if (!(nn > 0.0f && dn != 0.0f && u >= 0.0f && u < R.u)) return;
    const float rn = 1.0f / nn;
    const v3 w = sub(w0, mul(d, u));
    const float s = dot(cut_cross(w, e), n) * rn, t = dot(cut_cross(w, f), n) * rn;
    if (s >= 0.0f && s <= 1.0f && t >= 0.0f && t <= 1.0f) tsw_offer(R, u, add(m, mul(e, t)), kind);
}

// toi(query, record) for a record whose own gate opened at t0 (header): false when no candidate is valid or toi > tend
__device__ __forceinline__ bool tsw_tri(const TSTri& Q, const float4* __restrict__ tri, float t0, float tend, float& toi,
                                        v3& pt, int& kind) {
    const float4 w0 = tri[0], w1 = tri[1], w2 = tri[2];
    const v3 a = mk(w0.x, w0.y, w0.z), e1 = mk(w0.w, w1.x, w1.y), e2 = mk(w1.z, w1.w, w2.x);
    const v3 b = add(a, e1), c = add(a, e2);
    const v3 tlo = vmin3(a, b, c), thi = vmax3(a, b, c);
    const v3 sh = mul(Q.d, t0);  // 2.
    const v3 r0 = add(Q.q0, sh), rb = add(Q.qb, sh), rc = add(Q.qc, sh);
    {  // 3.
        const XTri X = cut_query(r0, add(Q.q1, sh), add(Q.q2, sh));
        v3 s0, s1;
        if (cut_tri(X, tri, s0, s1)) {
            toi = t0;
            pt = clamp3(s0, tlo, thi);
            kind = 15;
            return true;  // (t0 <= tend: the gate opened)
        }
    }
    TSPair R;  // 4.
    R.u = __builtin_inff();
    R.pt = a;
    R.kind = -1;
#pragma unroll
    for (int k = 0; k < 3; k++) {  // 0..2
        const v3 o = k == 0 ? r0 : k == 1 ? rb : rc;
        float u;
        if (tsw_ray(o, Q.d, a, e1, e2, u)) tsw_offer(R, u, add(o, mul(Q.d, u)), k);
    }
    const v3 nd = mk(-Q.d.x, -Q.d.y, -Q.d.z);
#pragma unroll
    for (int k = 0; k < 3; k++) {  // 3..5
        const v3 v = k == 0 ? a : k == 1 ? b : c;
        float u;
        if (tsw_ray(v, nd, r0, Q.f1, Q.f2, u)) tsw_offer(R, u, v, 3 + k);
    }
    const v3 f3 = sub(Q.f2, Q.f1), e3 = sub(e2, e1);
    // 6..14, query edge major. Kept a loop nest, as clear_tri's
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const v3 p1 = i == 2 ? rb : r0, d1 = i == 0 ? Q.f1 : i == 1 ? Q.f2 : f3;
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            const v3 p2 = j == 2 ? b : a, d2 = j == 0 ? e1 : j == 1 ? e2 : e3;
            tsw_edge(p1, d1, p2, d2, Q.d, R, 6 + 3 * i + j);
        }
    }
    toi = t0 + R.u;  // (no valid candidate: +inf, in no S_i)
    pt = clamp3(R.pt, tlo, thi);
    kind = R.kind;
    return toi <= tend;
}

// one query's answer so far: the smallest key toi_bits << 32 | original index, its point and kind, and the limit
struct TSState {
    unsigned long long key;
    v3 pt;
    int kind;
    float lim;  // fminf(T, the best toi so far): membership of S_i and the walk's prune
};
// the record's own gate, then toi: false when the gate turned the record away (no evaluation of toi)
__device__ __forceinline__ bool tsw_take(TSState& S, const TSTri& Q, const float4* __restrict__ rec, int orig) {
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
    const v3 a = mk(w0.x, w0.y, w0.z), b = add(a, mk(w0.w, w1.x, w1.y)), c = add(a, mk(w1.z, w1.w, w2.x));
    float t0;
    if (!tsw_gate(Q, vmin3(a, b, c), vmax3(a, b, c), S.lim, t0)) return false;
    float toi;
    v3 pt;
    int kind;
    if (tsw_tri(Q, rec, t0, S.lim, toi, pt, kind)) {
        const unsigned long long k = ((unsigned long long)__float_as_uint(toi) << 32) | (unsigned)orig;
        if (k < S.key) {
            S.key = k;
            S.pt = pt;
            S.kind = kind;
            S.lim = toi;
        }
    }
    return true;
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
__device__ __forceinline__ void tsw_exhaustive(const DScene& s, const TSTri& Q, TSState& S) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) (void)tsw_take(S, Q, s.ref.tris + 3 * j, s.ref.tri_orig[j]);
}

// leaf slot sl's 1..4 records (meta = count << 5 | offset), each gated, tested and offered to the key
__device__ __forceinline__ void tsw_leaf(const DWide& W, const TSTri& Q, TSState& S, unsigned sl, unsigned m0,
                                         unsigned m1, int tbase, unsigned long long& gated, unsigned long long& pairs) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
#pragma unroll 1
    for (int i = first; i < first + cnt; i++) {
        // (two sums, not a branch between the counters: the compiler made that an indexed pair in scratch)
        const unsigned tested = tsw_take(S, Q, W.tris + 3 * i, W.tri_orig[i]) ? 1u : 0u;
        pairs += tested;
        gated += 1u - tested;
    }
}

// the walk of the full wide view (header): sweep_wide with the box-against-box gate, earliest slot first
__device__ __forceinline__ void tsw_wide(const DWide& W, const TSTri& Q, TSState& S, int* __restrict__ stk,
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
            const bool open = tsw_gate(Q, L, H, S.lim, b[s]);
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
                const bool in = ((m >> s) & 1u) != 0u && b[s] <= S.lim;
                if (in && (sl < 0 || b[s] < bb)) {
                    sl = s;
                    bb = b[s];
                }
            }
            if (sl < 0) break;
            m &= ~(1u << sl);
            if ((imask >> sl) & 1u) {
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
            tsw_leaf(W, Q, S, (unsigned)sl, m0, m1, tbase, gated, pairs);
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
void k_trisweep(TSArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no LDS)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    unsigned tris = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long nodes = 0, gated = 0, pairs = 0;
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
            // a non-finite corner or motion, a NaN or negative bound: the empty set, before any walk
            const bool valid = finite3(q0) && finite3(q1) && finite3(q2) && finite3(d) && tm >= 0.0f;
            const TSTri Q = tsw_query(q0, q1, q2, d);
            TSState S;
            S.key = HKEY_EMPTY;
            S.pt = q0;
            S.kind = -1;
            S.lim = fminf(tm, FMAX);
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr && tsw_domain(q0, q1, q2, d, A.c_max);
                if (walk) tsw_wide(A.s.wide, Q, S, stk, nodes, gated, pairs, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    tsw_exhaustive(A.s, Q, S);
                    pairs += (unsigned long long)A.s.n_tris;
                }
            }
            exhc += exh;
            const bool none = S.key == HKEY_EMPTY;  // (then the point is q0's own bits and kind is -1, as set above)
            if (A.tri) A.tri[i] = none ? -1 : (int)(unsigned)S.key;
            if (A.t) A.t[i] = none ? FMAX : __uint_as_float((unsigned)(S.key >> 32));
            if (A.out) {
                A.out[3 * i] = S.pt.x;
                A.out[3 * i + 1] = S.pt.y;
                A.out[3 * i + 2] = S.pt.z;
            }
            if (A.kind) A.kind[i] = S.kind;
            found += none ? 0u : 1u;
            empty += none ? 1u : 0u;
        }
    }
    const unsigned v[TS_NCOUNT] = {tris, found, walked, exhc, empty, 0u, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < TS_NCOUNT; k++) {
        if (k == TS_NODES || k == TS_GATED || k == TS_PAIRS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long n64 = wave_sum64(nodes), g64 = wave_sum64(gated), p64 = wave_sum64(pairs);
    if (lane == 0 && n64) atomicAdd(A.counters + TS_NODES, n64);
    if (lane == 0 && g64) atomicAdd(A.counters + TS_GATED, g64);
    if (lane == 0 && p64) atomicAdd(A.counters + TS_PAIRS, p64);
}

}  // namespace rtd
