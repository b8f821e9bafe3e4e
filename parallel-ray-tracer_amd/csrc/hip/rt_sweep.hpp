// rt_sweep.hpp — sweep queries: the first contact of each caller-supplied moving sphere with the mesh
// (rt_sweep_spheres, rt_hip.h): raycast, overlap, sweep.
//
// Query i is a sphere of radius r whose centre is c + t d at time t, 0 <= t <= T = fminf(t_max[i], FLT_MAX). Its answer
// is the first element of
//   S_i = { j : toi(i, record j) exists }, ordered by (toi ascending, original triangle index ascending),
// empty when c, d or r is non-finite, r < 0, or t_max[i] is NaN or negative (decided before any walk). That is a total
// order, so the answer depends on no view, lane or visiting order.
//
// toi is defined on what a triangle RECORD holds (a, e1, e2: nearest_tri's operands), every operation one float32
// operation, dot left to right, nothing contracted, IEEE division and sqrtf. sweep_tri below is the sequence rt_hip.h
// states and tests/sweep_ref.py restates in numpy float32:
//   1. the gate: the interval of t in [0, T] at which the centre lies in the record's corner box grown by r, by slabs
//      (one subtraction and one multiplication by the sweep's own 1 / d.k per plane); t0 is where it starts;
//   2. recentre at c0 = c + d t0; D(c0, record) <= r2 (nearest_tri's own D): toi = t0;
//   3. else the least valid of seven candidates u >= 0 measured from c0 (from c for the face): the face plane moved by
//      r with the region algorithm's interior case at the touching centre, three edge cylinders, three vertex spheres;
//      toi = t0 + u, in S_i iff toi <= T.
// The contact point is nearest_tri's P of the centre c + d toi on the answering record, computed once per sweep.
//
// Why the walk needs no margin. (P1) toi >= t0: step 2 returns t0 and step 3 adds u >= 0. (P2) the gate
// is made of subtractions, one multiplication by a per-sweep constant, comparisons, fminf and fmaxf, all monotone in the
// box planes, so the same sweep_gate on a box [L, H] that contains the record's corner box gives an interval that
// contains the record's and a t0 that is <= the record's, and is empty only if the record's is. The decoded slot boxes of
// the full wide view contain the corner box of every record below them (rt_nearest.hpp's header). Hence a slot whose
// interval is empty, or whose t0 is STRICTLY greater than the best toi so far, holds no record that precedes the best in
// the order; a slot whose t0 EQUALS the best is entered, so an equal toi with a lower index is found. The walk hands
// sweep_gate the current limit lim = fminf(T, best toi) in T's place, for slots and records alike: by (P1) a record
// that this turns away has toi >= t0 > lim and precedes nothing.
// Monotonicity fails only where the gate makes a NaN (0 * inf, inf - inf): sweep_domain below keeps 1 / d.k finite and
// nonzero and every difference finite. A sweep outside it runs the exhaustive loop and counts in exhaustive_spheres.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK sweeps per returning atomic, one sweep per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order (a wave-uniform loop: the record loads
//                     broadcast), indices through s.ref.tri_orig; keeps the smallest key toi_bits << 32 | index
//                     (toi >= +0: one unsigned compare is the lexicographic one). The checker.
//   RT_KERNEL_FAST    walks the full wide view with rt_nearest.hpp's per-level LDS stack (node, slots still to try; the
//                     node is decoded again on a pop, so the pop-time prune is against the smaller best). A node's
//                     slots, leaf and interior alike, are taken in order of their gate t0 (ties: the lowest slot); a
//                     leaf slot's 1..4 records are tested with sweep_tri. A scene without a wide view
//                     (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
// The stack: 2 x WSTACK ints of the STACK-int LDS column; an entry is pushed only while slots remain, so at most
// depth - 1 <= WSTACK entries wait; a deeper view counts SW_ERR and ends that walk (no access out of range).
#pragma once
#include "rt_overlap.hpp"

// PRT_SWEEP_LEAF_FIRST 0 (the default): a node's leaf and interior slots alike are taken in order of their gate t0, so
// a contact found in a near leaf prunes the slots behind it; 1: rt_nearest.hpp's order, a node's leaf slots within the
// limit first, in slot order, then its interior slots by t0. Same answers; measured in DESIGN.md §3u.
#ifndef PRT_SWEEP_LEAF_FIRST
#define PRT_SWEEP_LEAF_FIRST 0
#endif

namespace rtd {

enum { SW_SPHERES, SW_FOUND, SW_WALKED, SW_EXH, SW_EMPTY, SW_NODES, SW_TRIS, SW_ERR, SW_NCOUNT };

struct SWArgs {
    DScene s;
    const float* centre;
    const float* motion;
    const float* radius;
    const float* t_max;  // nullable
    int* tri;            // [n], nullable
    float* t;            // [n], nullable
    float* out;          // [n][3], nullable
    unsigned long long* counters;  // SW_NCOUNT slots of the sweep query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    float c_max;  // sweep_domain's bound on max|c| and on r (2^20 x the scene's coordinate magnitude mx, rt_hip.hip)
};
static_assert(sizeof(SWArgs) == sizeof(DScene) + 9 * 8 + 8, "kernel-argument layout: both passes must agree");

// one sweep: its centre, motion and radius, and what every gate and candidate shares
struct SSphere {
    v3 c, d, inv;  // inv.k = 1 / d.k (unused where d.k == 0)
    float r, r2, dd;
};
__device__ __forceinline__ SSphere sweep_sphere(v3 c, v3 d, float r) {
    SSphere Q;
    Q.c = c;
    Q.d = d;
    Q.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    Q.r = r;
    Q.r2 = r * r;
    Q.dd = dot(d, d);
    return Q;
}

// The walk's domain: max|c| <= c_max and r <= c_max = 2^20 mx, and every NONZERO |d.k| in [2^-64, 2^64]. Then 1 / d.k
// is finite, normal and nonzero, every plane difference (L - r) - c is finite for planes within 2 mx, and the gate's
// products are a finite number times a finite nonzero one: no NaN, which is all (P2) needs (an overflow to +-inf keeps
// the order).
__device__ __forceinline__ bool sweep_domain(v3 c, v3 d, float r, float c_max) {
    const v3 ad = mk(__builtin_fabsf(d.x), __builtin_fabsf(d.y), __builtin_fabsf(d.z));
    const bool dx = ad.x == 0.0f || (ad.x >= 0x1p-64f && ad.x <= 0x1p64f);
    const bool dy = ad.y == 0.0f || (ad.y >= 0x1p-64f && ad.y <= 0x1p64f);
    const bool dz = ad.z == 0.0f || (ad.z >= 0x1p-64f && ad.z <= 0x1p64f);
    return dx && dy && dz && maxabs(c) <= c_max && r <= c_max;
}

// step 1 on the box [lo, hi]: the interval of t in [0, tend] with c + t d inside [lo - r, hi + r]; false when empty.
// An axis with d.k == 0 contributes the containment of c.k alone. One formula for records and slots (P2).
__device__ __forceinline__ bool sweep_gate(const SSphere& Q, v3 lo, v3 hi, float tend, float& t0) {
    const v3 glo = mk(lo.x - Q.r, lo.y - Q.r, lo.z - Q.r), ghi = mk(hi.x + Q.r, hi.y + Q.r, hi.z + Q.r);
    float a0 = 0.0f, a1 = tend;
    bool in = true;
    {
        const bool z = Q.d.x == 0.0f;
        const float ta = (glo.x - Q.c.x) * Q.inv.x, tb = (ghi.x - Q.c.x) * Q.inv.x;
        a0 = fmaxf(a0, z ? a0 : fminf(ta, tb));
        a1 = fminf(a1, z ? a1 : fmaxf(ta, tb));
        in = in && (!z || (glo.x <= Q.c.x && Q.c.x <= ghi.x));
    }
    {
        const bool z = Q.d.y == 0.0f;
        const float ta = (glo.y - Q.c.y) * Q.inv.y, tb = (ghi.y - Q.c.y) * Q.inv.y;
        a0 = fmaxf(a0, z ? a0 : fminf(ta, tb));
        a1 = fminf(a1, z ? a1 : fmaxf(ta, tb));
        in = in && (!z || (glo.y <= Q.c.y && Q.c.y <= ghi.y));
    }
    {
        const bool z = Q.d.z == 0.0f;
        const float ta = (glo.z - Q.c.z) * Q.inv.z, tb = (ghi.z - Q.c.z) * Q.inv.z;
        a0 = fmaxf(a0, z ? a0 : fminf(ta, tb));
        a1 = fminf(a1, z ? a1 : fmaxf(ta, tb));
        in = in && (!z || (glo.z <= Q.c.z && Q.c.z <= ghi.z));
    }
    t0 = a0;
    return in && a0 <= a1;
}

// the nearest query's region algorithm at q: does it reach its last case (the interior)?
__device__ __forceinline__ bool sweep_interior(v3 q, v3 a, v3 e1, v3 e2) {
    const v3 ap = sub(q, a);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const v3 bp = sub(ap, e1);
    const float d3 = dot(e1, bp), d4 = dot(e2, bp);
    const v3 cp = sub(ap, e2);
    const float d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float x = d4 - d3, y = d5 - d6;
    return !((d1 <= 0.0f && d2 <= 0.0f) || (d3 >= 0.0f && d4 <= d3) || (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) ||
             (d6 >= 0.0f && d5 <= d6) || (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) ||
             (va <= 0.0f && x >= 0.0f && y >= 0.0f));
}

// step 3's edge (p, f) and vertex candidates from the recentred c0: u when valid and below the least so far
__device__ __forceinline__ float sweep_edge(const SSphere& Q, v3 c0, v3 p, v3 f, float least) {
    const v3 m = sub(c0, p);
    const float md = dot(m, f), nd = dot(Q.d, f), ff = dot(f, f);
    const float A = ff * Q.dd - nd * nd;
    const float K = dot(m, m) - Q.r2;
    const float Cq = ff * K - md * md;
    const float Bq = ff * dot(m, Q.d) - nd * md;
    const float disc = Bq * Bq - A * Cq;
    const float u = (-Bq - sqrtf(disc)) / A;
    const float s = md + u * nd;
    const bool valid = A > 0.0f && disc >= 0.0f && u >= 0.0f && 0.0f <= s && s <= ff;
    return valid && u < least ? u : least;
}
__device__ __forceinline__ float sweep_vertex(const SSphere& Q, v3 c0, v3 v, float least) {
    const v3 m = sub(c0, v);
    const float Bv = dot(m, Q.d), Cv = dot(m, m) - Q.r2;
    const float disc = Bv * Bv - Q.dd * Cv;
    const float u = (-Bv - sqrtf(disc)) / Q.dd;
    const bool valid = Q.dd > 0.0f && disc >= 0.0f && u >= 0.0f;
    return valid && u < least ? u : least;
}

// toi(sweep, record) (header): false when the record is not in S_i as far as tend = fminf(T, the best toi so far) tells
__device__ __forceinline__ bool sweep_tri(const SSphere& Q, const float4* __restrict__ tri, float tend, float& toi) {
    const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2];
    const v3 a = mk(q0.x, q0.y, q0.z), e1 = mk(q0.w, q1.x, q1.y), e2 = mk(q1.z, q1.w, q2.x);
    const v3 b = add(a, e1), cc = add(a, e2);
    float t0;
    if (!sweep_gate(Q, vmin3(a, b, cc), vmax3(a, b, cc), tend, t0)) return false;  // 1.
    const v3 c0 = add(Q.c, mul(Q.d, t0));
    v3 P;
    if (nearest_tri(c0, tri, P) <= Q.r2) {  // 2.
        toi = t0;
        return true;
    }
    float u = __builtin_inff();  // 3. the least valid candidate
    {
        const v3 n = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
        const float nn = dot(n, n), ln = sqrtf(nn);
        const float so = dot(n, sub(Q.c, a)), dn = dot(n, Q.d);
        const float sg = so < 0.0f ? -1.0f : 1.0f;
        const float tf = (sg * (Q.r * ln) - so) / dn;
        if (nn > 0.0f && dn * sg < 0.0f && tf >= 0.0f && sweep_interior(add(Q.c, mul(Q.d, tf)), a, e1, e2))
            u = fmaxf(tf - t0, 0.0f);
    }
    u = sweep_edge(Q, c0, a, e1, u);
    u = sweep_edge(Q, c0, a, e2, u);
    u = sweep_edge(Q, c0, b, sub(e2, e1), u);
    u = sweep_vertex(Q, c0, a, u);
    u = sweep_vertex(Q, c0, b, u);
    u = sweep_vertex(Q, c0, cc, u);
    toi = t0 + u;  // (no valid candidate: +inf, in no S_i)
    return toi <= tend;
}

// one sweep's answer so far: the smallest key toi_bits << 32 | original index, the record that gave it, and the limit
struct SWState {
    unsigned long long key;
    const float4* rec;
    float lim;  // fminf(T, the best toi so far): membership of S_i and the walk's prune
};
__device__ __forceinline__ void sweep_take(SWState& S, const SSphere& Q, const float4* __restrict__ rec, int orig) {
    float toi;
    if (!sweep_tri(Q, rec, S.lim, toi)) return;
    const unsigned long long k = ((unsigned long long)__float_as_uint(toi) << 32) | (unsigned)orig;
    if (k < S.key) {
        S.key = k;
        S.rec = rec;
        S.lim = toi;
    }
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
__device__ __forceinline__ void sweep_exhaustive(const DScene& s, const SSphere& Q, SWState& S) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) sweep_take(S, Q, s.ref.tris + 3 * j, s.ref.tri_orig[j]);
}

// leaf slot sl's 1..4 records (meta = count << 5 | offset), each tested and offered to the key
__device__ __forceinline__ void sweep_leaf(const DWide& W, const SSphere& Q, SWState& S, unsigned sl, unsigned m0,
                                           unsigned m1, int tbase, unsigned long long& tris) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
    for (int i = first; i < first + cnt; i++) {
        tris++;
        sweep_take(S, Q, W.tris + 3 * i, W.tri_orig[i]);
    }
}

// the walk of the full wide view (header): per-level stack entries (node, slots still to try), earliest slot first
__device__ __forceinline__ void sweep_wide(const DWide& W, const SSphere& Q, SWState& S, int* __restrict__ stk,
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
            const bool open = sweep_gate(Q, L, H, S.lim, b[s]);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            if (((mask >> s) & 1u) && occ && open) m |= 1u << s;
        }
#if PRT_SWEEP_LEAF_FIRST
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
                sweep_leaf(W, Q, S, sl, m0, m1, tbase, tris);
            }
        }
#endif
        bool descended = false;
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
            if (PRT_SWEEP_LEAF_FIRST || ((imask >> sl) & 1u)) {  // (leaf first: only interior slots are left)
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
            sweep_leaf(W, Q, S, (unsigned)sl, m0, m1, tbase, tris);
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
void k_sweep(SWArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no LDS)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    unsigned spheres = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long nodes = 0, tris = 0;
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
            // a non-finite c, d or r, r < 0, a NaN or negative bound: the empty set, before any walk
            const bool valid = finite3(c) && finite3(d) && r >= 0.0f && r <= FMAX && tm >= 0.0f;
            const SSphere Q = sweep_sphere(c, d, r);
            SWState S;
            S.key = HKEY_EMPTY;
            S.rec = nullptr;
            S.lim = fminf(tm, FMAX);
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr && sweep_domain(c, d, r, A.c_max);
                if (walk) sweep_wide(A.s.wide, Q, S, stk, nodes, tris, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    sweep_exhaustive(A.s, Q, S);
                    tris += (unsigned long long)A.s.n_tris;
                }
            }
            exhc += exh;
            const bool none = S.key == HKEY_EMPTY;
            const float toi = none ? FMAX : __uint_as_float((unsigned)(S.key >> 32));
            if (A.tri) A.tri[i] = none ? -1 : (int)(unsigned)S.key;
            if (A.t) A.t[i] = toi;
            if (A.out) {
                v3 P = c;  // (the empty set: c's own bits)
                if (!none) (void)nearest_tri(add(c, mul(d, toi)), S.rec, P);  // the contact point (header)
                A.out[3 * i] = P.x;
                A.out[3 * i + 1] = P.y;
                A.out[3 * i + 2] = P.z;
            }
            found += none ? 0u : 1u;
            empty += none ? 1u : 0u;
        }
    }
    const unsigned v[SW_NCOUNT] = {spheres, found, walked, exhc, empty, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < SW_NCOUNT; k++) {
        if (k == SW_NODES || k == SW_TRIS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long n64 = wave_sum64(nodes), t64 = wave_sum64(tris);
    if (lane == 0 && n64) atomicAdd(A.counters + SW_NODES, n64);
    if (lane == 0 && t64) atomicAdd(A.counters + SW_TRIS, t64);
}

}  // namespace rtd
