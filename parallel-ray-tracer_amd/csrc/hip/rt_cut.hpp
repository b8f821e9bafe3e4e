// rt_cut.hpp — cut queries: the mesh triangles that each caller-supplied triangle crosses, how many, and the segment
// along which each pair crosses (rt_cut_triangles, rt_hip.h): the query for the shape the scene itself is made of,
// beside the ray, point, box and sphere queries.
//
// Query i is a triangle q0, q1, q2. Its answer is
//   S_i = { j : X(q, record j) }, ordered by original triangle index ascending,
// empty when any of the nine numbers is non-finite (decided before any walk). X is defined on what a triangle RECORD
// holds (a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)), every operation one float32 operation, nothing contracted (the
// library's build: -ffp-contract=off, IEEE division, IEEE fminf / fmaxf). cut_tri below is the sequence rt_hip.h states
// and tests/cut_ref.py restates in numpy float32: with b = fl(a + e1), c = fl(a + e2), f1 = fl(q1 - q0), f2 = fl(q2 - q0)
//   1. the gate: the corner box of a, b, c against the corner box of q0, q1, q2, comparisons only;
//   2. a, b, c against the query's plane (normal nq = f1 x f2): all on one side, or all in it -> false;
//   3. q0, q1, q2 against the record's plane (normal nm = e1 x e2): the same;
//   4. the line of the two planes, D = nq x nm, and its largest axis k;
//   5. Moller's interval of each triangle on that line: the two points where its edges cross the other's plane, their
//      k coordinates;
//   6. X is true iff the two closed intervals overlap. The cut segment runs from the later start to the earlier end.
// A coplanar pair and a query of zero area are not members (2. or 3. finds all three distances zero). That is a set
// with a total order, so the answer depends on no view, lane or visiting order.
//
// The per-triangle list is rt_overlap.hpp's OState, the list form its CSR segments; cut_take is overlap_take with the
// segment written beside the index (list_seg[p] with list[p]). Instantiated for CAP = 0 (counting only), 4, 8 and 16.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK triangles per returning atomic, one per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig. The checker.
//   RT_KERNEL_FAST    walks the full wide view as overlap_wide does, against the query's corner box [qlo, qhi]: per
//                     node the 8 slot boxes are decoded; an occupied slot is kept unless L.k > qhi.k or H.k < qlo.k on
//                     some axis; every triangle of a kept leaf slot is tested with cut_tri; the kept interior slots are
//                     entered in slot order, the rest of the level waiting on the per-level LDS stack. No slot is
//                     accepted untested: a slot inside the query's box says nothing about a crossing. A scene without a
//                     wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
//
// Why the walk needs no margin: rt_overlap.hpp's argument with the query's corner box in place of the query box. Step 1
// is part of X and uses comparisons only: a member of S_i has tlo.k <= qhi.k and thi.k >= qlo.k on every axis, exactly.
// The corner box [tlo, thi] of a, b, c lies inside the decoded box [L, H] of every slot on the record's path
// (rt_nearest.hpp's header). So L.k <= tlo.k <= qhi.k and H.k >= thi.k >= qlo.k: no slot on the path of a member is
// dropped, however steps 2..6 round. Each record is offered at most once per query, as in overlap_wide: one leaf slot
// per record, a stack entry holds interior slots not yet entered only, a pop decodes nothing.
//
// The stack: overlap_wide's, one two-word entry per level in the STACK-int LDS column (34 KB per workgroup), plus the
// 8-key column (8 KB) in the fast capacity-16 build. The exhaustive kernel holds no LDS.
#pragma once
#include "rt_overlap.hpp"

namespace rtd {

constexpr int CUTS_MAX = 16;  // RT_CUTS_MAX
enum { X_TRIS, X_FOUND, X_STORED, X_COUNTED, X_LISTED, X_WALKED, X_EXH, X_EMPTY, X_NODES, X_PAIRS, X_ERR, X_NCOUNT };

struct XArgs {
    DScene s;
    const float* tris;   // [n][3][3]
    const int* offsets;  // [n + 1], nullable (with list)
    int* tri;            // [n][max_tris], nullable
    int* count;          // [n], nullable
    int* list;           // nullable (with offsets)
    float* list_seg;     // [offsets[n]][2][3], nullable (only with list)
    unsigned long long* counters;  // X_NCOUNT slots of the cut query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    int max_tris;
    int count_all;
    int pad;
};
static_assert(sizeof(XArgs) == sizeof(DScene) + 8 * 8 + 16, "kernel-argument layout: both passes must agree");

// one query triangle: its corners, its plane's normal, its corner box
struct XTri {
    v3 q0, q1, q2, nq, lo, hi;
};
__device__ __forceinline__ v3 cut_cross(v3 u, v3 v) {  // (overlap_tri's nrm)
    return mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
__device__ __forceinline__ float cut_dot(v3 u, v3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ XTri cut_query(v3 q0, v3 q1, v3 q2) {
    XTri Q;
    Q.q0 = q0;
    Q.q1 = q1;
    Q.q2 = q2;
    Q.nq = cut_cross(sub(q1, q0), sub(q2, q0));
    Q.lo = vmin3(q0, q1, q2);
    Q.hi = vmax3(q0, q1, q2);
    return Q;
}

// all three on one side of the plane, or all three in it
__device__ __forceinline__ bool cut_apart(float d0, float d1, float d2) {
    return (d0 > 0.0f && d1 > 0.0f && d2 > 0.0f) || (d0 < 0.0f && d1 < 0.0f && d2 < 0.0f) ||
           (d0 == 0.0f && d1 == 0.0f && d2 == 0.0f);
}
__device__ __forceinline__ float cut_comp(v3 p, int k) { return k == 0 ? p.x : k == 1 ? p.y : p.z; }
__device__ __forceinline__ v3 cut_pick(int i, v3 a, v3 b, v3 c) { return i == 0 ? a : i == 1 ? b : c; }

// step 5: one triangle's interval on the line, from its corners and their distances to the other's plane
struct XIv {
    v3 ps, pe;  // the start and the end point
    float lo, hi;
};
__device__ __forceinline__ XIv cut_interval(v3 v0, v3 v1, v3 v2, float d0, float d1, float d2, int k) {
    const int s0 = (d0 > 0.0f) - (d0 < 0.0f), s1 = (d1 > 0.0f) - (d1 < 0.0f), s2 = (d2 > 0.0f) - (d2 < 0.0f);
    int al = 2;  // the lone corner
    if (s0 == s1 && s0 != 0) al = 2;
    else if (s0 == s2 && s0 != 0) al = 1;
    else if ((s1 == s2 && s1 != 0) || s0 != 0) al = 0;
    else if (s1 != 0) al = 1;
    const v3 va = cut_pick(al, v0, v1, v2), vx = cut_pick(al, v1, v2, v0), vy = cut_pick(al, v2, v0, v1);
    const float da = al == 0 ? d0 : al == 1 ? d1 : d2, dx = al == 0 ? d1 : al == 1 ? d2 : d0,
                dy = al == 0 ? d2 : al == 1 ? d0 : d1;
    const float lx = da / (da - dx), ly = da / (da - dy);
    const v3 px = add(va, mul(sub(vx, va), lx)), py = add(va, mul(sub(vy, va), ly));
    const float tx = cut_comp(px, k), ty = cut_comp(py, k);
    const bool fwd = tx <= ty;
    XIv I;
    I.ps = fwd ? px : py;
    I.pe = fwd ? py : px;
    I.lo = fminf(tx, ty);
    I.hi = fmaxf(tx, ty);
    return I;
}

// X(q, record) (header); the cut segment of a member in s0, s1
__device__ __forceinline__ bool cut_tri(const XTri& Q, const float4* __restrict__ tri, v3& s0, v3& s1) {
    const float4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
    const v3 a = mk(t0.x, t0.y, t0.z), e1 = mk(t0.w, t1.x, t1.y), e2 = mk(t1.z, t1.w, t2.x);
    const v3 b = add(a, e1), c = add(a, e2);
    const v3 tlo = vmin3(a, b, c), thi = vmax3(a, b, c);
    if (!(tlo.x <= Q.hi.x && thi.x >= Q.lo.x && tlo.y <= Q.hi.y && thi.y >= Q.lo.y && tlo.z <= Q.hi.z &&
          thi.z >= Q.lo.z))
        return false;  // 1.
    const float dm0 = cut_dot(Q.nq, sub(a, Q.q0)), dm1 = cut_dot(Q.nq, sub(b, Q.q0)), dm2 = cut_dot(Q.nq, sub(c, Q.q0));
    if (cut_apart(dm0, dm1, dm2)) return false;  // 2.
    const v3 nm = cut_cross(e1, e2);
    const float dq0 = cut_dot(nm, sub(Q.q0, a)), dq1 = cut_dot(nm, sub(Q.q1, a)), dq2 = cut_dot(nm, sub(Q.q2, a));
    if (cut_apart(dq0, dq1, dq2)) return false;  // 3.
    const v3 D = cut_cross(Q.nq, nm);           // 4.
    int k = 0;
    float best = fabsf(D.x);
    if (fabsf(D.y) > best) {
        k = 1;
        best = fabsf(D.y);
    }
    if (fabsf(D.z) > best) k = 2;
    const XIv M = cut_interval(a, b, c, dm0, dm1, dm2, k);              // 5.
    const XIv I = cut_interval(Q.q0, Q.q1, Q.q2, dq0, dq1, dq2, k);
    if (!(M.lo <= I.hi && I.lo <= M.hi)) return false;                  // 6.
    s0 = I.lo > M.lo ? I.ps : M.ps;
    s1 = I.hi < M.hi ? I.pe : M.pe;
    return true;
}

// one member of S_i: overlap_take, with the segment written beside the index
template <class ST>
__device__ __forceinline__ void cut_take(ST& S, int orig, int K, int* __restrict__ list, float* __restrict__ seg,
                                         v3 s0, v3 s1) {
    if (list && seg) {
        const long long at = S.seg + (long long)S.total;
        if (at < S.seg_end) {
            float* o = seg + 6 * at;
            o[0] = s0.x;
            o[1] = s0.y;
            o[2] = s0.z;
            o[3] = s1.x;
            o[4] = s1.y;
            o[5] = s1.z;
        }
    }
    overlap_take(S, orig, K, list);
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
template <class ST>
__device__ __forceinline__ void cut_exhaustive(const DScene& s, const XTri& Q, ST& S, int K, int* __restrict__ list,
                                               float* __restrict__ seg) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        v3 s0, s1;
        if (cut_tri(Q, s.ref.tris + 3 * j, s0, s1)) cut_take(S, s.ref.tri_orig[j], K, list, seg, s0, s1);
    }
}

// the walk of the full wide view (header): overlap_wide against [Q.lo, Q.hi], every kept leaf slot's triangles tested
template <class ST>
__device__ __forceinline__ void cut_wide(const DWide& W, const XTri& Q, ST& S, int K, int* __restrict__ list,
                                         float* __restrict__ seg, int* __restrict__ stk, unsigned long long& nodes,
                                         unsigned long long& pairs, unsigned& err) {
    const gnodes nbase = walk_base(W.nodes);
    int node = 0, sp = 0;
    for (;;) {
        const WNode N = wload_at(nbase, node);
        nodes++;
        const unsigned e = __float_as_uint(N.f0.w);
        unsigned imask = e >> 24;
        int cbase = __float_as_int(N.f1.x);
        const int tbase = __float_as_int(N.f1.y);
        const unsigned m0 = __float_as_uint(N.f1.z), m1 = __float_as_uint(N.f1.w);
        const v3 p = mk(N.f0.x, N.f0.y, N.f0.z);
        const v3 sc = mk(pow2_bits(e & 0xFFu), pow2_bits((e >> 8) & 0xFFu), pow2_bits((e >> 16) & 0xFFu));
        const unsigned wx[4] = {__float_as_uint(N.f2.x), __float_as_uint(N.f2.y), __float_as_uint(N.f2.z),
                                __float_as_uint(N.f2.w)},
                       wy[4] = {__float_as_uint(N.f3.x), __float_as_uint(N.f3.y), __float_as_uint(N.f3.z),
                                __float_as_uint(N.f3.w)},
                       wz[4] = {__float_as_uint(N.f4.x), __float_as_uint(N.f4.y), __float_as_uint(N.f4.z),
                                __float_as_uint(N.f4.w)};
        unsigned keep = 0u;  // occupied slots whose box meets the query's corner box
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int j = s >> 1, sh = 16 * (s & 1);
            const unsigned qx = wx[j] >> sh, qy = wy[j] >> sh, qz = wz[j] >> sh;
            const float lx = __builtin_fmaf(sc.x, (float)(QBIAS + (qx & 0xFFu)), p.x);
            const float hx = __builtin_fmaf(sc.x, (float)(QBIAS + ((qx >> 8) & 0xFFu)), p.x);
            const float ly = __builtin_fmaf(sc.y, (float)(QBIAS + (qy & 0xFFu)), p.y);
            const float hy = __builtin_fmaf(sc.y, (float)(QBIAS + ((qy >> 8) & 0xFFu)), p.y);
            const float lz = __builtin_fmaf(sc.z, (float)(QBIAS + (qz & 0xFFu)), p.z);
            const float hz = __builtin_fmaf(sc.z, (float)(QBIAS + ((qz >> 8) & 0xFFu)), p.z);
            const unsigned meta = ((s < 4 ? m0 : m1) >> (8 * (s & 3))) & 0xFFu;
            const bool occ = ((imask >> s) & 1u) != 0u || meta != 0u;
            const bool drop = lx > Q.hi.x || hx < Q.lo.x || ly > Q.hi.y || hy < Q.lo.y || lz > Q.hi.z || hz < Q.lo.z;
            if (occ && !drop) keep |= 1u << s;
        }
        unsigned lh = keep & ~imask;  // the kept leaf slots, in slot order; none is pushed
        while (lh) {
            const unsigned sl = (unsigned)__builtin_ctz(lh);
            lh &= lh - 1u;
            const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
            const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
            for (int i = first; i < first + cnt; i++) {
                v3 s0, s1;
                pairs++;
                if (cut_tri(Q, W.tris + 3 * i, s0, s1)) cut_take(S, W.tri_orig[i], K, list, seg, s0, s1);
            }
        }
        unsigned m = keep & imask;  // the kept interior slots
        if (!m) {                   // nothing to enter here: the next slot of the nearest waiting level
            if (sp == 0) return;
            --sp;
            cbase = stk[(2 * sp) * BLOCK];
            const unsigned w = (unsigned)stk[(2 * sp + 1) * BLOCK];
            imask = w >> 8;
            m = w & 0xFFu;
        }
        const unsigned sl = (unsigned)__builtin_ctz(m);
        m &= m - 1u;  // (before the child is entered: a pushed mask holds slots not yet entered only)
        if (m) {      // the rest of this level waits
            if (sp >= WSTACK) {
                err++;
                return;
            }
            stk[(2 * sp) * BLOCK] = cbase;
            stk[(2 * sp + 1) * BLOCK] = (int)(imask << 8 | m);
            sp++;
        }
        node = cbase + __builtin_popcount(imask & ((1u << sl) - 1u));
    }
}

// CAP: the list's capacity (0: counting only). STRICT: the exhaustive kernel.
template <int CAP, bool STRICT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(3)))
void k_cut(XArgs A) {
    int* stk = nullptr;
    if constexpr (!STRICT) {  // (the exhaustive kernel walks nothing and holds no LDS)
        __shared__ int lds[STACK * BLOCK];
        stk = lds + threadIdx.x;
    }
    constexpr int REG = overlap_reg(CAP, STRICT);
    unsigned* ovf = nullptr;
    if constexpr (CAP > REG) {
        __shared__ unsigned lds_ovf[(CAP - REG) * BLOCK];
        ovf = lds_ovf + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    const int K = A.max_tris;
    const bool all = A.count_all != 0;
    unsigned tris = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long stored = 0, counted = 0, listed = 0, nodes = 0, pairs = 0;
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
            const bool valid = finite3(q0) && finite3(q1) && finite3(q2);  // else the empty set, before any walk
            const XTri Q = cut_query(q0, q1, q2);
            OState<CAP, REG> S;
#pragma unroll
            for (int j = 0; j < (REG > 0 ? REG : 1); j++) S.key[j] = OKEY_EMPTY;
            S.ovf = ovf;
            if constexpr (CAP > REG) {
#pragma unroll
                for (int j = 0; j < CAP - REG; j++) ovf[j * BLOCK] = OKEY_EMPTY;
            }
            S.kth = OKEY_EMPTY;
            S.total = 0u;
            S.seg = 0;
            S.seg_end = 0;
            if (A.list) {  // (an entry that decreases, or a negative one: a segment of no length)
                const long long a = A.offsets[i], b = A.offsets[i + 1];
                S.seg = a;
                S.seg_end = a >= 0 && b > a ? b : a;
            }
            bool exh = valid;
            if constexpr (!STRICT) {
                const bool walk = valid && A.s.wide.nodes != nullptr;
                if (walk) cut_wide(A.s.wide, Q, S, K, A.list, A.list_seg, stk, nodes, pairs, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    cut_exhaustive(A.s, Q, S, K, A.list, A.list_seg);
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
                        unsigned k = S.key[j < REG ? j : 0];
                        if constexpr (CAP > REG) {
                            if (j >= REG) k = ovf[(j - REG) * BLOCK];
                        }
                        if (A.tri) A.tri[ob + j] = (int)k;  // (OKEY_EMPTY is -1)
                        st += k == OKEY_EMPTY ? 0u : 1u;
                    }
                }
            }
            const unsigned cnt = all ? S.total : st;
            if (A.count) A.count[i] = (int)cnt;
            found += S.total != 0u;
            empty += S.total == 0u;
            stored += st;
            counted += cnt;
            const long long room = S.seg_end - S.seg;
            listed += (unsigned long long)((long long)S.total < room ? (long long)S.total : room);
        }
    }
    const unsigned v[X_NCOUNT] = {tris, found, 0u, 0u, 0u, walked, exhc, empty, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < X_NCOUNT; k++) {
        if (k == X_STORED || k == X_COUNTED || k == X_LISTED || k == X_NODES || k == X_PAIRS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted), l64 = wave_sum64(listed),
                             n64 = wave_sum64(nodes), p64 = wave_sum64(pairs);
    if (lane == 0 && s64) atomicAdd(A.counters + X_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + X_COUNTED, c64);
    if (lane == 0 && l64) atomicAdd(A.counters + X_LISTED, l64);
    if (lane == 0 && n64) atomicAdd(A.counters + X_NODES, n64);
    if (lane == 0 && p64) atomicAdd(A.counters + X_PAIRS, p64);
}

}  // namespace rtd
