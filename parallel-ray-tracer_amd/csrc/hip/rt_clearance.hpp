// rt_clearance.hpp — clearance queries: the mesh triangle nearest each caller-supplied triangle, the squared distance
// and the pair of points where the two come closest (rt_clearance_triangles, rt_hip.h): rt_cut_triangles' distance form,
// as rt_nearest_points is the distance form of a point query.
//
// Query i is a triangle q0, q1, q2 with an optional bound max_dist2[i]. Its candidate set is
//   S_i = { j : D(q, record j) <= min(max_dist2[i], FLT_MAX) }
// ordered by (D ascending, original triangle index ascending); the answer is its first element. That is a total order,
// so the answer depends on no view, lane or visiting order.
//
// D is defined on what a triangle RECORD holds (a, e1, e2; corners a, b = fl(a + e1), c = fl(a + e2), corner box
// [tlo, thi]) and on the query made a record the same way (f1 = fl(q1 - q0), f2 = fl(q2 - q0), qb = fl(q0 + f1),
// qc = fl(q0 + f2)); [qlo, qhi] is the box of the FIVE points q0, q1, q2, qb, qc: it holds the raw corners that cut_tri
// gates on and the record corners the candidates use. clear_tri below is the sequence rt_hip.h states and
// tests/clearance_ref.py restates in numpy float32, every operation one float32 operation, nothing contracted:
//   candidates 0..2    q0, qb, qc against the mesh record: nearest_tri's own D and P, the pair (corner, P);
//   candidates 3..5    a, b, c against the query record (q0, f1, f2): the same function, the pair (P, corner);
//   candidates 6..14   the nine edge pairs, query edge major: clear_edges, a segment-segment closest pair (Ericson,
//                      Real-Time Collision Detection 5.1.9) whose two points are clamped into [qlo, qhi] and [tlo, thi];
//   a candidate replaces the pair's best only when its D is strictly smaller;
//   the crossing       if cut_tri (unchanged, on the raw corners) holds, D = 0 and both points are the cut segment's
//                      first end s0: kind 15.
//
// Two kernels of k_nearest's skeleton (persistent waves, QUERY_CHUNK queries per returning atomic, one query per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig, no
//                     pre-gate; keeps the smallest 64-bit key D_bits << 32 | index. The checker.
//   RT_KERNEL_FAST    walks the full wide view as nearest_wide does (per-level two-word LDS stack, reload and re-prune
//                     on a pop, leaf slots first), with the box-to-box bound in place of the point-to-box one: per axis
//                     e = fmaxf(fmaxf(lo - qhi, qlo - hi), 0), bound = e.x*e.x + e.y*e.y + e.z*e.z, no FMA. A slot is
//                     dropped only when its bound is strictly greater than lim = min(the query's bound, the best D so
//                     far). The pair function is expensive, so a record of a kept leaf slot is skipped (counted in
//                     pairs_gated) when the same bound on its own corner box exceeds lim, or when the least key the
//                     record could have, bound_bits << 32 | index, exceeds the best key (a bound equal to the best D
//                     at a higher index: once a crossing is found, every record above its index): pure pruning. A
//                     scene without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
//
// Why no margin is needed. Every candidate's two points lie in [qlo, qhi] and [tlo, thi]: the corners by construction,
// nearest_tri's P by its own clamp into the corner box of the record it is given, clear_edges' points by its clamps.
// [tlo, thi] lies inside the decoded box of every slot on the record's path (rt_nearest.hpp's header). So per axis
// |pq - pm| >= max(lo - qhi, qlo - hi, 0) as real numbers, for the record's own box and for every slot box above it.
// Float32 subtraction, multiplication and addition are monotone, so the COMPUTED bound is <= the COMPUTED D, term by
// term and in the left-to-right sums. A crossing pair passed cut_tri's gate -- the raw corner box, which lies inside
// [qlo, qhi], meets [tlo, thi] -- so its bound is exactly 0 = its D. Hence no record of S_i's head is ever pruned and the
// fast answer has the exhaustive one's bits.
#pragma once
#include "rt_cut.hpp"

namespace rtd {

enum { CL_TRIS, CL_FOUND, CL_WALKED, CL_EXH, CL_EMPTY, CL_NODES, CL_GATED, CL_PAIRS, CL_ERR, CL_NCOUNT };

struct CLArgs {
    DScene s;
    const float* tris;       // [n][3][3]
    const float* max_dist2;  // nullable
    int* tri;                // [n], nullable
    float* d2;               // [n], nullable
    float* on_query;         // [n][3], nullable
    float* on_mesh;          // [n][3], nullable
    int* kind;               // [n], nullable
    unsigned long long* counters;  // CL_NCOUNT slots of the clearance query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    int pad;
};
static_assert(sizeof(CLArgs) == sizeof(DScene) + 9 * 8 + 8, "kernel-argument layout: both passes must agree");

// one query triangle: cut_tri's form of it (raw corners, plane normal, raw corner box), its record and the five-point box
struct CLTri {
    XTri X;
    v3 f1, f2, qb, qc, lo, hi;
};
__device__ __forceinline__ CLTri clear_query(v3 q0, v3 q1, v3 q2) {
    CLTri Q;
    Q.X = cut_query(q0, q1, q2);
    Q.f1 = sub(q1, q0);
    Q.f2 = sub(q2, q0);
    Q.qb = add(q0, Q.f1);
    Q.qc = add(q0, Q.f2);
    const v3 l = vmin3(q0, q1, q2), h = vmax3(q0, q1, q2);
    Q.lo = vmin3(l, Q.qb, Q.qc);
    Q.hi = vmax3(h, Q.qb, Q.qc);
    return Q;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ v3 clamp3(v3 p, v3 lo, v3 hi) {
    return mk(fminf(fmaxf(p.x, lo.x), hi.x), fminf(fmaxf(p.y, lo.y), hi.y), fminf(fmaxf(p.z, lo.z), hi.z));
}

// the lower bound on D of everything inside [lo, hi] (header)
__device__ __forceinline__ float box_bound(v3 qlo, v3 qhi, v3 lo, v3 hi) {
    const float ex = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.0f);
    const float ey = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.0f);
    const float ez = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.0f);
    return ex * ex + ey * ey + ez * ez;
}
// slot_bound with the query's box in place of the point
__device__ __forceinline__ float slot_box_bound(v3 qlo, v3 qhi, v3 p, v3 sc, unsigned wx, unsigned wy, unsigned wz) {
    const float lx = __builtin_fmaf(sc.x, (float)(QBIAS + (wx & 0xFFu)), p.x);
    const float hx = __builtin_fmaf(sc.x, (float)(QBIAS + ((wx >> 8) & 0xFFu)), p.x);
    const float ly = __builtin_fmaf(sc.y, (float)(QBIAS + (wy & 0xFFu)), p.y);
    const float hy = __builtin_fmaf(sc.y, (float)(QBIAS + ((wy >> 8) & 0xFFu)), p.y);
    const float lz = __builtin_fmaf(sc.z, (float)(QBIAS + (wz & 0xFFu)), p.z);
    const float hz = __builtin_fmaf(sc.z, (float)(QBIAS + ((wz >> 8) & 0xFFu)), p.z);
    return box_bound(qlo, qhi, mk(lx, ly, lz), mk(hx, hy, hz));
}

// one pair's best candidate so far
struct CLPair {
    float D;
    v3 pq, pm;
    int kind;
};
__device__ __forceinline__ void clear_offer(CLPair& R, float D, v3 pq, v3 pm, int kind) {
    if (D < R.D) {
        R.D = D;
        R.pq = pq;
        R.pm = pm;
        R.kind = kind;
    }
}

// candidates 6..14: the closest pair of the segments p1 + d1*s and p2 + d2*t, s, t in [0, 1] (header)
__device__ __forceinline__ void clear_edges(v3 p1, v3 d1, v3 p2, v3 d2, v3 qlo, v3 qhi, v3 tlo, v3 thi, CLPair& R,
                                            int kind) {
    const v3 r = sub(p1, p2);
    const float A = dot(d1, d1), E = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), B = dot(d1, d2);
    const float den = A * E - B * B;
    float s = den > 0.0f ? clamp01((B * f - c * E) / den) : 0.0f;
    float t = (B * s + f) / E;
    // the one division of s' second form, on the operands the case names: -c / A or (B - c) / A
    const bool under = t < 0.0f, over = !under && t > 1.0f;
    if (under || over) s = clamp01((under ? -c : B - c) / A);
    t = clamp01(t);
    const v3 c1 = clamp3(add(p1, mul(d1, s)), qlo, qhi), c2 = clamp3(add(p2, mul(d2, t)), tlo, thi);
    const v3 df = sub(c1, c2);
    clear_offer(R, dot(df, df), c1, c2, kind);
}

// D(q, record), the pair of points and the winning candidate's kind (header)
__device__ __forceinline__ float clear_tri(const CLTri& Q, const float4* __restrict__ tri, v3& pq, v3& pm, int& kind) {
    const float4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
    const v3 a = mk(t0.x, t0.y, t0.z), e1 = mk(t0.w, t1.x, t1.y), e2 = mk(t1.z, t1.w, t2.x);
    const v3 b = add(a, e1), c = add(a, e2);
    const v3 tlo = vmin3(a, b, c), thi = vmax3(a, b, c);
    const v3 q0 = Q.X.q0;
    CLPair R;
    R.D = __builtin_inff();  // (a D that is no number of S_i either way: the first finite candidate replaces it)
    R.pq = q0;
    R.pm = a;
    R.kind = -1;
#pragma unroll
    for (int k = 0; k < 3; k++) {  // 0..2
        const v3 v = k == 0 ? q0 : k == 1 ? Q.qb : Q.qc;
        v3 P;
        const float D = nearest_tri(v, tri, P);
        clear_offer(R, D, v, P, k);
    }
    const float4 qr[3] = {make_float4(q0.x, q0.y, q0.z, Q.f1.x), make_float4(Q.f1.y, Q.f1.z, Q.f2.x, Q.f2.y),
                          make_float4(Q.f2.z, 0.0f, 0.0f, 0.0f)};  // the query as a record
#pragma unroll
    for (int k = 0; k < 3; k++) {  // 3..5
        const v3 v = k == 0 ? a : k == 1 ? b : c;
        v3 P;
        const float D = nearest_tri(v, qr, P);
        clear_offer(R, D, P, v, 3 + k);
    }
    const v3 f3 = sub(Q.f2, Q.f1), e3 = sub(e2, e1);
    // 6..14, query edge major. Kept a loop nest: unrolled, the nine closest pairs push the fast kernel past the 168
    // registers of three waves per SIMD and into scratch
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const v3 p1 = i == 2 ? Q.qb : q0, d1 = i == 0 ? Q.f1 : i == 1 ? Q.f2 : f3;
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            const v3 p2 = j == 2 ? b : a, d2 = j == 0 ? e1 : j == 1 ? e2 : e3;
            clear_edges(p1, d1, p2, d2, Q.lo, Q.hi, tlo, thi, R, 6 + 3 * i + j);
        }
    }
    v3 s0, s1;
    if (cut_tri(Q.X, tri, s0, s1)) {  // the crossing
        R.D = 0.0f;
        R.pq = s0;
        R.pm = s0;
        R.kind = 15;
    }
    pq = R.pq;
    pm = R.pm;
    kind = R.kind;
    return R.D;
}

// one query's answer so far: the smallest key D_bits << 32 | original index, its points and kind, the pruning limit
struct CLState {
    unsigned long long key;
    v3 pq, pm;
    int kind;
    float bound;  // min(max_dist2, FLT_MAX): membership of S_i
    float lim;    // min(bound, the best D so far): the walk's prune
};
__device__ __forceinline__ void clear_take(CLState& S, float D, v3 pq, v3 pm, int kind, int orig) {
    if (!(D <= S.bound)) return;  // (an overflowed or NaN D is in no S_i)
    const unsigned long long k = ((unsigned long long)__float_as_uint(D) << 32) | (unsigned)orig;
    if (k < S.key) {
        S.key = k;
        S.pq = pq;
        S.pm = pm;
        S.kind = kind;
        S.lim = D;
    }
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform), no pre-gate
__device__ __forceinline__ void clear_exhaustive(const DScene& s, const CLTri& Q, CLState& S) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        v3 pq, pm;
        int kind;
        const float D = clear_tri(Q, s.ref.tris + 3 * j, pq, pm, kind);
        clear_take(S, D, pq, pm, kind, s.ref.tri_orig[j]);
    }
}

// leaf slot sl's 1..4 records (meta = count << 5 | offset): each gated by its own corner box (D >= its bound >= +0, so
// the record's key is at least bound_bits << 32 | index), then tested and offered
__device__ __forceinline__ void clear_leaf(const DWide& W, const CLTri& Q, CLState& S, unsigned sl, unsigned m0,
                                           unsigned m1, int tbase, unsigned long long& gated,
                                           unsigned long long& pairs) {
    const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
    const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
#pragma unroll 1
    for (int i = first; i < first + cnt; i++) {
        const float4* __restrict__ tri = W.tris + 3 * i;
        const float4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
        const v3 a = mk(t0.x, t0.y, t0.z), b = add(a, mk(t0.w, t1.x, t1.y)), c = add(a, mk(t1.z, t1.w, t2.x));
        const float bnd = box_bound(Q.lo, Q.hi, vmin3(a, b, c), vmax3(a, b, c));
        const int orig = W.tri_orig[i];
        if (bnd > S.lim || (((unsigned long long)__float_as_uint(bnd) << 32) | (unsigned)orig) > S.key) {
            gated++;
            continue;
        }
        v3 pq, pm;
        int kind;
        pairs++;
        const float D = clear_tri(Q, tri, pq, pm, kind);
        clear_take(S, D, pq, pm, kind, orig);
    }
}

// the walk of the full wide view (header): nearest_wide with the box-to-box bound, leaf slots first
__device__ __forceinline__ void clear_wide(const DWide& W, const CLTri& Q, CLState& S, int* __restrict__ stk,
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
        unsigned m = 0u;  // the slots still to try: in the entry's mask, occupied, bound <= lim
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int j = s >> 1, sh = 16 * (s & 1);
            b[s] = slot_box_bound(Q.lo, Q.hi, p, sc, wx[j] >> sh, wy[j] >> sh, wz[j] >> sh);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            if (((mask >> s) & 1u) && occ && b[s] <= S.lim) m |= 1u << s;
        }
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
                clear_leaf(W, Q, S, sl, m0, m1, tbase, gated, pairs);
            }
        }
        // the nearest remaining interior slot whose bound does not exceed the (possibly smaller) limit; ties: the
        // lowest slot
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
        if (sl >= 0) {
            m &= ~(1u << sl);
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
            continue;
        }
        if (sp == 0) return;
        --sp;
        node = stk[(2 * sp) * BLOCK];
        mask = (unsigned)stk[(2 * sp + 1) * BLOCK];
    }
}

// STRICT: the exhaustive kernel
template <bool STRICT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(3)))
void k_clearance(CLArgs A) {
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
            const float md = A.max_dist2 ? A.max_dist2[i] : FMAX;
            // a NaN or negative bound, a non-finite corner: the empty set, before any walk
            const bool valid = md >= 0.0f && finite3(q0) && finite3(q1) && finite3(q2);
            const CLTri Q = clear_query(q0, q1, q2);
            CLState S;
            S.key = HKEY_EMPTY;
            S.pq = q0;
            S.pm = q0;
            S.kind = -1;
            S.bound = fminf(md, FMAX);
            S.lim = S.bound;
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr;
                if (walk) clear_wide(A.s.wide, Q, S, stk, nodes, gated, pairs, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    clear_exhaustive(A.s, Q, S);
                    pairs += (unsigned long long)A.s.n_tris;
                }
            }
            exhc += exh;
            const bool none = S.key == HKEY_EMPTY;  // (then the points are q0's own bits and kind is -1, as set above)
            if (A.tri) A.tri[i] = none ? -1 : (int)(unsigned)S.key;
            if (A.d2) A.d2[i] = none ? FMAX : __uint_as_float((unsigned)(S.key >> 32));
            if (A.on_query) {
                A.on_query[3 * i] = S.pq.x;
                A.on_query[3 * i + 1] = S.pq.y;
                A.on_query[3 * i + 2] = S.pq.z;
            }
            if (A.on_mesh) {
                A.on_mesh[3 * i] = S.pm.x;
                A.on_mesh[3 * i + 1] = S.pm.y;
                A.on_mesh[3 * i + 2] = S.pm.z;
            }
            if (A.kind) A.kind[i] = S.kind;
            found += none ? 0u : 1u;
            empty += none ? 1u : 0u;
        }
    }
    const unsigned v[CL_NCOUNT] = {tris, found, walked, exhc, empty, 0u, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < CL_NCOUNT; k++) {
        if (k == CL_NODES || k == CL_GATED || k == CL_PAIRS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long n64 = wave_sum64(nodes), g64 = wave_sum64(gated), p64 = wave_sum64(pairs);
    if (lane == 0 && n64) atomicAdd(A.counters + CL_NODES, n64);
    if (lane == 0 && g64) atomicAdd(A.counters + CL_GATED, g64);
    if (lane == 0 && p64) atomicAdd(A.counters + CL_PAIRS, p64);
}

}  // namespace rtd
