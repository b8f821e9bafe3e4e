// rt_overlap.hpp — overlap queries: the triangles that touch each caller-supplied axis-aligned box, and how many
// (rt_overlap_boxes, rt_hip.h): the query for a volume, beside the ray queries and the point queries.
//
// Query i is a closed box [lo, hi]. Its answer is
//   S_i = { j : T(lo, hi, record j) }, ordered by original triangle index ascending,
// empty when any of the six numbers is non-finite or lo > hi on an axis (decided before any walk). T is defined on what
// a triangle RECORD holds (a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0), nearest_tri's operands), every operation one
// float32 operation, nothing contracted (the library's build: -ffp-contract=off, IEEE fminf / fmaxf). overlap_tri below
// is the sequence rt_hip.h states and tests/overlap_ref.py restates in numpy float32: with b = fl(a + e1), c = fl(a + e2)
//   1. the corner box of a, b, c against the query box, comparisons only: no overlap on an axis -> false;
//   2. the corner box inside the query box, comparisons only -> true;
//   3. Akenine-Moller's separating axes about the box centre: nine edge x axis cross products and the plane.
// That is a set with a total order, so the answer depends on no view, lane or visiting order.
//
// The per-box list is rt_hits.hpp's HState on 32-bit keys: the max_tris SMALLEST original indices of S_i, kept sorted
// (OState: the unrolled compare-exchange insertion of hits_take on indices alone; OKEY_EMPTY = 0xFFFFFFFF sorts after
// every index), the first 8 in registers, keys 9..16 of the fast kernel's 16-key build in a per-lane LDS column: 16 keys
// in registers beside this walk spill inside its loop (168 VGPRs, 53 spilled, by the compiler's remarks; DESIGN.md
// §3r). The exhaustive kernel has no walk and holds all 16 in registers. Instantiated for CAP = 0 (counting only), 4,
// 8 and 16; a request runs the smallest that holds max_tris.
// The list form: with offsets, every member of S_i is also written, as it is found, to list[offsets[i] + the lane's
// running count] while that lies below offsets[i + 1] -- no atomics, no order; the count goes on past a full segment.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK boxes per returning atomic, one box per lane):
//   RT_KERNEL_STRICT  exhaustive: every record of s.ref.tris in stored order, indices through s.ref.tri_orig. The checker.
//   RT_KERNEL_FAST    walks the full wide view. Per node the 8 slot boxes are decoded (slot_bound's own decode); an
//                     occupied slot is kept unless L.k > hi.k or H.k < lo.k on some axis; the kept leaf slots' 1..4
//                     triangles are tested with overlap_tri -- or taken untested when the slot's decoded box lies
//                     inside the query box: step 2 then holds for each of them --; the kept interior slots are entered
//                     in slot order, the rest of the level waiting on the per-level LDS stack. No ordering by
//                     distance, no limit that moves. A scene without a wide view (RT_ACCEL_REFERENCE) runs the
//                     exhaustive loop under either kernel.
//
// Why the walk needs no margin. Step 1 is part of T and uses comparisons only: a triangle in S_i has
// tlo.k <= hi.k and thi.k >= lo.k on every axis, exactly. The corner box [tlo, thi] of a, b, c lies inside the decoded
// box [L, H] of every slot on the triangle's path (rt_nearest.hpp's header: the planes are the vertices' extent moved
// outward by 256 ulp of the scene's magnitude and quantised outward with the decode used here; fl(a + fl(v1 - v0)) is
// within 2 ulp of v1). So L.k <= tlo.k <= hi.k and H.k >= thi.k >= lo.k: no slot on the path of a member of S_i is
// dropped, however step 3 rounds. A slot whose decoded box lies inside the query box holds only triangles with
// lo.k <= L.k <= tlo.k and thi.k <= H.k <= hi.k: step 2 is true for them, whatever step 3 would have said.
// Whole interior subtrees are never accepted unseen: the nodes hold no triangle counts.
//
// Each triangle at most once per box; a repeated offer would duplicate an entry or inflate a count. (a) The wide view
// holds each triangle in exactly one leaf slot (tests/test_gpu_hits.py checks the views' tri_orig for duplicates). (b) A
// node's leaf slots are tested only where the node is decoded; a stack entry holds interior slots only (the pushed mask
// is a subset of keep & imask) and a pop decodes nothing: it continues with the entry's next interior slot. (c) An
// interior slot leaves the mask before its child is entered, so a child is entered, and a node decoded, at most once.
// The count tests of tests/test_gpu_overlap.py (counts equal to the yardstick's on every box) pin this.
//
// The stack: one entry per LEVEL, two words: the node's first-child index, and imask << 8 | the kept interior slots
// still to enter -- all a pop needs, so a waiting level costs no second load of its node. An entry is pushed only while
// slots remain, so at most depth - 1 <= WSTACK entries wait: 2 x WSTACK ints of the STACK-int LDS column (34 KB per
// workgroup, k_nearest's budget), plus the 8-key column (8 KB) in the fast capacity-16 build. The exhaustive kernel
// holds no LDS.
#pragma once
#include "rt_nearest.hpp"

namespace rtd {

constexpr int OVERLAPS_MAX = 16;  // RT_OVERLAPS_MAX
enum { O_BOXES, O_FOUND, O_STORED, O_COUNTED, O_LISTED, O_WALKED, O_EXH, O_EMPTY, O_NODES, O_TRIS, O_ERR, O_NCOUNT };

struct OArgs {
    DScene s;
    const float* lo;
    const float* hi;
    const int* offsets;  // [n + 1], nullable (with list)
    int* tri;            // [n][max_tris], nullable
    int* count;          // [n], nullable
    int* list;           // nullable (with offsets)
    unsigned long long* counters;  // O_NCOUNT slots of the overlap query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    int max_tris;
    int count_all;
    int pad;
};
static_assert(sizeof(OArgs) == sizeof(DScene) + 8 * 8 + 16, "kernel-argument layout: both passes must agree");

// one query box: its planes, and step 3's centre and half-widths (ctr = fl(fl(0.5 lo) + fl(0.5 hi)),
// h = fl(fl(0.5 hi) - fl(0.5 lo)))
struct OBox {
    v3 lo, hi, ctr, h;
};
__device__ __forceinline__ OBox overlap_box(v3 lo, v3 hi) {
    OBox B;
    B.lo = lo;
    B.hi = hi;
    const v3 l2 = mul(lo, 0.5f), h2 = mul(hi, 0.5f);
    B.ctr = add(l2, h2);
    B.h = sub(h2, l2);
    return B;
}

// one of step 3's nine axes: edge f crossed with box axis k, (i, j) = (k + 1, k + 2) mod 3; vmi = v_m.i, vmj = v_m.j
__device__ __forceinline__ bool overlap_axis(float v0i, float v0j, float v1i, float v1j, float v2i, float v2j, float fi,
                                             float fj, float hi, float hj) {
    const float p0 = v0j * fi - v0i * fj, p1 = v1j * fi - v1i * fj, p2 = v2j * fi - v2i * fj;
    const float rad = hi * fabsf(fj) + hj * fabsf(fi);
    return fminf(fminf(p0, p1), p2) > rad || fmaxf(fmaxf(p0, p1), p2) < -rad;  // (a NaN operand separates nothing)
}
__device__ __forceinline__ bool overlap_edge(v3 v0, v3 v1, v3 v2, v3 f, v3 h) {
    return overlap_axis(v0.y, v0.z, v1.y, v1.z, v2.y, v2.z, f.y, f.z, h.y, h.z) ||  // k = x: i = y, j = z
           overlap_axis(v0.z, v0.x, v1.z, v1.x, v2.z, v2.x, f.z, f.x, h.z, h.x) ||  // k = y: i = z, j = x
           overlap_axis(v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, f.x, f.y, h.x, h.y);    // k = z: i = x, j = y
}

// T(lo, hi, record) (header)
__device__ __forceinline__ bool overlap_tri(const OBox& B, const float4* __restrict__ tri) {
    const float4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
    const v3 a = mk(t0.x, t0.y, t0.z), e1 = mk(t0.w, t1.x, t1.y), e2 = mk(t1.z, t1.w, t2.x);
    const v3 b = add(a, e1), c = add(a, e2);
    const v3 tlo = vmin3(a, b, c), thi = vmax3(a, b, c);
    if (!(tlo.x <= B.hi.x && thi.x >= B.lo.x && tlo.y <= B.hi.y && thi.y >= B.lo.y && tlo.z <= B.hi.z &&
          thi.z >= B.lo.z))
        return false;  // 1.
    if (tlo.x >= B.lo.x && thi.x <= B.hi.x && tlo.y >= B.lo.y && thi.y <= B.hi.y && tlo.z >= B.lo.z &&
        thi.z <= B.hi.z)
        return true;  // 2.
    const v3 v0 = sub(a, B.ctr), v1 = sub(b, B.ctr), v2 = sub(c, B.ctr);
    if (overlap_edge(v0, v1, v2, e1, B.h) || overlap_edge(v0, v1, v2, sub(e2, e1), B.h) ||
        overlap_edge(v0, v1, v2, e2, B.h))
        return false;
    const v3 nrm = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    const float d = nrm.x * v0.x + nrm.y * v0.y + nrm.z * v0.z;
    const float r = B.h.x * fabsf(nrm.x) + B.h.y * fabsf(nrm.y) + B.h.z * fabsf(nrm.z);
    return !(fabsf(d) > r);
}

// one box's state: the K smallest indices so far, sorted -- the first REG of them in registers, the other CAP - REG in
// the lane's LDS column ovf ([j][lane]) --; the running count; the list segment
constexpr unsigned OKEY_EMPTY = ~0u;
constexpr int overlap_reg(int cap, bool strict) { return strict || cap <= 8 ? cap : 8; }
template <int CAP_, int REG_>
struct OState {
    static constexpr int CAP = CAP_, REG = REG_;
    unsigned key[REG > 0 ? REG : 1];
    unsigned* ovf;
    unsigned kth;    // the K-th stored index (K = max_tris, wave-uniform), OKEY_EMPTY while fewer than K are stored
    unsigned total;  // members of S_i so far
    long long seg, seg_end;  // list[seg + total] is the next free entry while it lies below seg_end
};

// one member of S_i: counted, written to the list segment while there is room, inserted when it sorts before the K-th
template <class ST>
__device__ __forceinline__ void overlap_take(ST& S, int orig, int K, int* __restrict__ list) {
    constexpr int CAP = ST::CAP, REG = ST::REG;
    if (list) {
        const long long at = S.seg + (long long)S.total;
        if (at < S.seg_end) list[at] = orig;
    }
    S.total++;
    if constexpr (CAP > 0) {
        unsigned k = (unsigned)orig;
        if (k < S.kth) {
#pragma unroll
            for (int j = 0; j < REG; j++) {  // sorted insertion; the largest key falls off the end
                const unsigned a = S.key[j];
                const bool lt = k < a;
                S.key[j] = lt ? k : a;
                k = lt ? a : k;
            }
            unsigned kth = OKEY_EMPTY;
            if constexpr (CAP > REG) {  // K > REG here (the smaller capacities serve the others): the K-th is in LDS
#pragma unroll 1
                for (int j = 0; j < CAP - REG && k != OKEY_EMPTY; j++) {
                    const unsigned a = S.ovf[j * BLOCK];
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
        }
    }
}

// every record of the scene: the reference tree's records in stored order (j is wave-uniform)
template <class ST>
__device__ __forceinline__ void overlap_exhaustive(const DScene& s, const OBox& B, ST& S, int K,
                                                   int* __restrict__ list) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        if (overlap_tri(B, s.ref.tris + 3 * j)) overlap_take(S, s.ref.tri_orig[j], K, list);
    }
}

// the walk of the full wide view (header): keep the occupied slots whose decoded box meets the query box, test the
// kept leaf slots' triangles, enter the kept interior slots in slot order
template <class ST>
__device__ __forceinline__ void overlap_wide(const DWide& W, const OBox& B, ST& S, int K, int* __restrict__ list,
                                             int* __restrict__ stk, unsigned long long& nodes,
                                             unsigned long long& tris, unsigned& err) {
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
        unsigned keep = 0u, inside = 0u;  // occupied slots whose box meets the query box; those wholly inside it
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
            const bool drop = lx > B.hi.x || hx < B.lo.x || ly > B.hi.y || hy < B.lo.y || lz > B.hi.z || hz < B.lo.z;
            const bool in = lx >= B.lo.x && hx <= B.hi.x && ly >= B.lo.y && hy <= B.hi.y && lz >= B.lo.z &&
                            hz <= B.hi.z;
            if (occ && !drop) keep |= 1u << s;
            if (in) inside |= 1u << s;
        }
        unsigned lh = keep & ~imask;  // the kept leaf slots, in slot order; none is pushed
        while (lh) {
            const unsigned sl = (unsigned)__builtin_ctz(lh);
            lh &= lh - 1u;
            const unsigned meta = ((sl < 4u ? m0 : m1) >> (8u * (sl & 3u))) & 0xFFu;
            const int first = tbase + (int)(meta & 31u), cnt = (int)(meta >> 5);
            const bool in = ((inside >> sl) & 1u) != 0u;
            for (int i = first; i < first + cnt; i++) {
                bool t = in;  // (a slot inside the query box: step 2 holds for its triangles, header)
                if (!in) {
                    t = overlap_tri(B, W.tris + 3 * i);
                    tris++;
                }
                if (t) overlap_take(S, W.tri_orig[i], K, list);
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
void k_overlap(OArgs A) {
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
    unsigned boxes = 0, found = 0, walked = 0, exhc = 0, empty = 0, err = 0;
    unsigned long long stored = 0, counted = 0, listed = 0, nodes = 0, tris = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long i = (long long)ch * QUERY_CHUNK + pass * 64 + (int)lane_now();
            if (i >= A.n) continue;
            boxes++;
            const v3 lo = mk(A.lo[3 * i], A.lo[3 * i + 1], A.lo[3 * i + 2]);
            const v3 hi = mk(A.hi[3 * i], A.hi[3 * i + 1], A.hi[3 * i + 2]);
            // a non-finite plane, lo > hi on an axis: the empty set, before any walk
            const bool valid = finite3(lo) && finite3(hi) && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
            const OBox B = overlap_box(lo, hi);
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
                if (walk) overlap_wide(A.s.wide, B, S, K, A.list, stk, nodes, tris, err);
                walked += walk;
                exh = valid && !walk;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) {
                    overlap_exhaustive(A.s, B, S, K, A.list);
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
    const unsigned v[O_NCOUNT] = {boxes, found, 0u, 0u, 0u, walked, exhc, empty, 0u, 0u, err};
#pragma unroll
    for (int k = 0; k < O_NCOUNT; k++) {
        if (k == O_STORED || k == O_COUNTED || k == O_LISTED || k == O_NODES || k == O_TRIS) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted), l64 = wave_sum64(listed),
                             n64 = wave_sum64(nodes), t64 = wave_sum64(tris);
    if (lane == 0 && s64) atomicAdd(A.counters + O_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + O_COUNTED, c64);
    if (lane == 0 && l64) atomicAdd(A.counters + O_LISTED, l64);
    if (lane == 0 && n64) atomicAdd(A.counters + O_NODES, n64);
    if (lane == 0 && t64) atomicAdd(A.counters + O_TRIS, t64);
}

}  // namespace rtd
