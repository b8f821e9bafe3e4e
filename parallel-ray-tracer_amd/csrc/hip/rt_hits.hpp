// rt_hits.hpp — multi-hit queries: the k nearest hits and the hit count of caller-supplied rays (rt_trace_hits, rt_hip.h).
//
// For ray i (origin o, direction d, not normalised; optional bound t_max[i]) the hit set is
//   S_i = { j : hit_triangle(o, d, triangles[j]) = t_j < FLT_MAX and t_j <= t_max[i] }
// with hit_triangle = cpu/src/raytracer.c:35-59 (its |det| < EPSILON and t > EPSILON culls, the reference's operand
// order; the bits the kernels' hit_triangle returns), ordered by (t ascending, original triangle index ascending). That
// is a total order, so the answer depends on no BVH, view, lane or visiting order: it is what the reference's brute-force
// path sees (USE_BVH 0, raytracer.c:115-129), NOT what bvh_traverse sees. The one known difference (DESIGN.md §2 item
// 2): for a direction with a zero component from an origin on a box face the reference's BVH walk divides 0 by 0 and
// misses geometry that brute force finds. Here that geometry is found.
//
// Two kernels of k_query's skeleton (persistent waves, QUERY_CHUNK rays per returning atomic, one ray per lane,
// lockstep; no pool form):
//   RT_KERNEL_STRICT  exhaustive: every lane's ray against every triangle of the scene, the reference tree's records in
//                     stored order (a wave-uniform loop: the record loads broadcast), indices through tri_orig.
//                     Bit-exact by construction; the checker. It is as slow as that sounds: rays x triangles tests.
//   RT_KERNEL_FAST    a ray inside query_domain walks the view ray_view picks (hits_wide: closest_wide's loop); the
//                     box limit is closest_lim(bound), bound = the k-th stored t once the list is full (never with
//                     count_all), else t_max, else FLT_MAX. PRUNE_SLACK stays on that bound, so a triangle whose t
//                     equals the k-th entry's and whose index is smaller is still reached and displaces it. No tie
//                     flag, no re-walk of the reference tree, no ref_reaches: none applies to this definition. Scenes
//                     without a wide view walk the binary acceleration tree (hits_binary: closest_walk<false>'s box test
//                     and limit). Rays outside query_domain (non-finite, max|d_i| outside [2^-20, 2^20], |o| > 4 mx) run
//                     the exhaustive loop after the wave's fast walks, together (exhaustive_rays).
//
// Zero direction components stay on the wide walk. The argument, from safe_dir and wide_node: let d.x = 0 and let
// hit_triangle accept a triangle at t. The hit point o + t d lies in the triangle's plane region, and its x is o.x up
// to the test's rounding, so o.x lies within the triangle's x extent up to that rounding, hence inside every box on the
// triangle's path by the inflation (2^-16 mx per side, planes then quantised outward) less that rounding: at least
// ~2^-17 mx from both x planes. safe_dir replaces d.x by 1e-20, ray_pre_closest makes ix = 1e20 * 2^-40 > 0, and
// wide_node computes the planes' t as fma(q, kx, fma(p.x, ix, -ox)): (plane - o.x) * ix with a relative rounding of a
// few ulp of max(|plane|, |o.x|) <= 4 mx, i.e. an absolute error below 2^-20 mx * ix against a distance of at least
// 2^-17 mx * ix. So the near x plane's t keeps its sign (negative: the clamp makes it 0) and the far plane's is positive
// and at least 2^-17 mx * ix = 700 mx in the rescaled t, where every hit of a ray in query_domain lies below 9 mx 2^-20:
// the x slab contains [0, t] for every such hit, whatever the origin -- on a face of the REFERENCE tree or not, since a
// wide view's planes are never the reference's faces but the triangles' extents moved outward by the inflation. The
// other axes are tested as for any ray. Hence the wide box test never rejects a box that holds a triangle hit_triangle
// accepts for such a ray (tests/test_gpu_hits.py: the degenerate rows and columns and the origin-on-a-face camera).
// The binary acceleration tree gives no such margin when it is the reference tree itself (RT_ACCEL_REFERENCE: boxes
// not inflated, box_fast's plane minus origin is then a rounding residual of either sign), so on scenes without a wide
// view every ray with a zero direction component runs the exhaustive loop.
//
// The per-ray list: up to CAP (t, original index) pairs as 64-bit keys t_bits << 32 | index -- for positive t the
// float bits order as unsigned integers, so one unsigned compare is the lexicographic one -- kept sorted. Up to 8 keys
// live in REGISTERS (an unrolled compare-exchange insertion, compile-time indices only). The fast kernel's 16-key build
// keeps keys 9..16 in a per-lane LDS column, where the key that falls off the registers is inserted: by the code
// object's numbers 16 keys in registers beside the wide walk need 168 VGPRs plus 200 spilled, inside the
// walk loop; 16 keys in LDS are 32 KB per workgroup beside the 34 KB of stacks, 2 workgroups per CU; 8 + 8 is 50 KB,
// 3 workgroups, no spill. The exhaustive kernel has no walk and holds all 16 in registers (106 VGPRs).
// Instantiated for CAP = 0 (counting only), 4, 8 and 16; a request runs the smallest that holds max_hits. The view
// position is mapped to the original index (tri_orig) at insertion. A view holds each triangle once and a walk visits
// each node once, so a triangle is tested, and inserted, at most once per ray (tests/test_gpu_hits.py checks the views'
// tri_orig for duplicates).
// Packed triangle tests through the wave's LDS queue (TQ) are left out.
#pragma once
#include "rt_query.hpp"

namespace rtd {

constexpr int HITS_MAX = 16;  // RT_HITS_MAX
enum { H_RAYS, H_RAYS_HIT, H_STORED, H_COUNTED, H_UNIT, H_SHORT, H_FULL, H_EXH, H_ERR, H_NCOUNT };

struct HArgs {
    DScene s;
    const float* origin;
    const float* dir;
    const float* t_max;  // nullable
    int* tri;            // [n][max_hits], nullable
    float* t;            // [n][max_hits], nullable
    int* count;          // [n], nullable
    unsigned long long* counters;  // H_NCOUNT slots of the hits query's own block
    unsigned int* work;            // its own chunk counter
    int n;
    float o_max;  // query_domain's bound on max|o|
    int max_hits;
    int count_all;
};
static_assert(sizeof(HArgs) == sizeof(DScene) + 8 * 8 + 16, "kernel-argument layout: both passes must agree");

constexpr unsigned long long HKEY_EMPTY = ~0ull;  // sorts after every key (its t bits are a NaN's: no hit has them)

// one ray's state: the sorted keys -- the first REG of them in registers, the other CAP - REG in the lane's LDS column
// ovf ([j][lane], 8-byte words) --, the K-th of them (K = max_hits, wave-uniform), the walk's pruning bound
constexpr int hits_reg(int cap, bool strict) { return strict || cap <= 8 ? cap : 8; }
template <int CAP_, int REG_>
struct HState {
    static constexpr int CAP = CAP_, REG = REG_;
    unsigned long long key[REG > 0 ? REG : 1];
    unsigned long long* ovf;
    unsigned long long kth;
    float bound;     // min(t_max, FLT_MAX), then the K-th stored t once the first K slots are full (not with count_all)
    unsigned total;  // accepted hits so far (|S| with count_all)
};
template <class ST>
__device__ __forceinline__ void hits_init(ST& S, float bound, unsigned long long* ovf) {
#pragma unroll
    for (int j = 0; j < (ST::REG > 0 ? ST::REG : 1); j++) S.key[j] = HKEY_EMPTY;
    S.ovf = ovf;
    if constexpr (ST::CAP > ST::REG) {
#pragma unroll
        for (int j = 0; j < ST::CAP - ST::REG; j++) ovf[j * BLOCK] = HKEY_EMPTY;
    }
    S.kth = HKEY_EMPTY;
    S.bound = bound;
    S.total = 0u;
}
// entry j of the list (j a compile-time constant after unrolling)
template <class ST>
__device__ __forceinline__ unsigned long long hits_key(const ST& S, int j) {
    if constexpr (ST::CAP > ST::REG) {
        if (j >= ST::REG) return S.ovf[(j - ST::REG) * BLOCK];
    }
    return S.key[j < ST::REG ? j : 0];
}

// one triangle test's result for the ray: pos = the triangle's position in the walked view
template <class ST>
__device__ __forceinline__ void hits_take(ST& S, float tt, const int* __restrict__ tri_orig, int pos, int K, bool all) {
    constexpr int CAP = ST::CAP, REG = ST::REG;
    if (!(tt <= S.bound) || tt == FMAX) return;  // (bound <= t_max; FMAX: hit_triangle's miss)
    S.total++;
    if constexpr (CAP > 0) {
        const unsigned long long k0 = ((unsigned long long)__float_as_uint(tt) << 32) | (unsigned)tri_orig[pos];
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

// closest_wide's loop (wide_node, wide_step_next, the unconditional next-node load, BOX_TMIN) with the list's bound
template <class ST>
__device__ __forceinline__ void hits_wide(const DWide& W, v3 o, v3 d, ST& S, int K, bool all,
                                          int* __restrict__ stk, unsigned& err) {
    const RayPre p = ray_pre_closest(o, d);
    const unsigned oct = (p.ix < 0.0f ? 1u : 0u) | (p.iy < 0.0f ? 2u : 0u) | (p.iz < 0.0f ? 4u : 0u);
    int sp = 0;
    TopC tc;
    const gnodes nbase = walk_base(W.nodes);
    WNode N = wload_at(nbase, 0);
    for (;;) {
        unsigned nh, th, imask, nl;
        int cb, tb;
        pin_node(N);
        wide_node<false, LATE_TRIS, CLOSEST_CLAMP ? 2 : 0>(N, p, oct, closest_lim(S.bound), nh, th, cb, tb, imask, nl);
        const unsigned m0 = __float_as_uint(N.f1.z), m1 = __float_as_uint(N.f1.w);
        const int next = wide_step_next<false>(nh, cb, imask, oct, sp, tc, stk, WSTACK);
        N = wload_at(nbase, next >= 0 ? next : 0);  // unconditional (closest_wide)
        top_reload<false>(sp, tc, stk, WSTACK);
        if constexpr (LATE_TRIS) th = leaf_tris<false>(th, m0, m1, nl);
        while (th) {
            const int i = tb + __builtin_ctz(th);
            th &= th - 1u;
            int k;
            const float tt = hit_triangle<true>(o, d, W.tris + 3 * i, k);
            hits_take(S, tt, W.tri_orig, i, K, all);
        }
        if (next < 0) {
            if (next == -2) err++;
            break;
        }
    }
}

// closest_walk<false, false>'s loop (box_fast, visit<false>) on the binary acceleration tree
template <class ST>
__device__ __forceinline__ void hits_binary(const DBvh& B, v3 o, v3 d, ST& S, int K, bool all,
                                            int* __restrict__ stk, unsigned& err) {
    const RayPre p = ray_pre(o, d);
    int sp = 0, cur = B.root;
    for (;;) {
        if (cur < 0) {
            const int2 lf = B.leaves[~cur];
            for (int i = lf.x; i < lf.x + lf.y; ++i) {
                int k;
                const float tt = hit_triangle(o, d, B.tris + 3 * i, k);
                hits_take(S, tt, B.tri_orig, i, K, all);
            }
        } else {
            int ni, fi;
            float nt, ft;
            children<false>(B, cur, o, d, p, ni, nt, fi, ft);
            const bool vn = visit<false>(nt, S.bound), vf = visit<false>(ft, S.bound);
            if (sp + 2 > STACK) {
                err++;
                break;
            }
            if (vn) {
                if (vf) stk[(sp++) * BLOCK] = fi;
                cur = ni;
                continue;
            }
            if (vf) {
                cur = fi;
                continue;
            }
        }
        if (sp == 0) break;
        cur = stk[(--sp) * BLOCK];
    }
}

// every triangle of the scene: the reference tree's records in stored order (j is wave-uniform)
template <class ST>
__device__ __forceinline__ void hits_exhaustive(const DScene& s, v3 o, v3 d, ST& S, int K, bool all) {
    const int n = s.n_tris;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        int k;
        const float tt = hit_triangle(o, d, s.ref.tris + 3 * j, k);
        hits_take(S, tt, s.ref.tri_orig, j, K, all);
    }
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
    return v;
}

// CAP: the list's capacity (0: counting only). STRICT: the exhaustive kernel.
template <int CAP, bool STRICT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(3)))
void k_hits(HArgs A) {
    __shared__ int lds[STACK * BLOCK];
    int* stk = lds + threadIdx.x;
    constexpr int REG = hits_reg(CAP, STRICT);
    unsigned long long* ovf = nullptr;
    if constexpr (CAP > REG) {
        __shared__ unsigned long long lds_ovf[(CAP - REG) * BLOCK];
        ovf = lds_ovf + threadIdx.x;
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    const int K = A.max_hits;
    const bool all = A.count_all != 0;
    unsigned rays = 0, rays_hit = 0, unit = 0, shrt = 0, full = 0, exhc = 0, err = 0;
    unsigned long long stored = 0, counted = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long i = (long long)ch * QUERY_CHUNK + pass * 64 + (int)lane_now();
            if (i >= A.n) continue;
            rays++;
            const v3 o = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
            const v3 d = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
            const float tmax = A.t_max ? A.t_max[i] : FMAX;
            const bool valid = tmax > 0.0f;  // a NaN or non-positive bound: the empty set, before any walk
            HState<CAP, REG> S;
            hits_init(S, fminf(tmax, FMAX), ovf);
            bool exh = valid;
            if constexpr (!STRICT) {
                bool fast = valid && query_domain(o, d, A.o_max);
                if (A.s.wide.nodes) {
                    const int view = ray_view(A.s, d);
#pragma unroll 1
                    for (int v = 0; v < 3; v++) {  // the views the wave's rays chose, one after another (closest_q)
                        const bool mine = fast && view == v;
                        if (!__builtin_amdgcn_readfirstlane((int)(__ballot(mine) != 0ull))) continue;
                        const DWide W = v == 0 ? A.s.unit : v == 1 ? A.s.prim : A.s.wide;
                        if (mine) hits_wide(W, o, d, S, K, all, stk, err);
                    }
                    if (fast) {
                        unit += view == 0;
                        shrt += view == 1;
                        full += view == 2;
                    }
                } else {
                    fast = fast && !degenerate(d);  // (the binary tree's boxes may be the reference's own: header)
                    if (fast) {
                        hits_binary(A.s.acc, o, d, S, K, all, stk, err);
                        full++;
                    }
                }
                exh = valid && !fast;
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(exh) != 0ull))) {
                if (exh) hits_exhaustive(A.s, o, d, S, K, all);
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
            }
            const unsigned cnt = all ? S.total : st;
            if (A.count) A.count[i] = (int)cnt;
            rays_hit += S.total != 0u;
            stored += st;
            counted += cnt;
        }
    }
    const unsigned v[H_NCOUNT] = {rays, rays_hit, 0u, 0u, unit, shrt, full, exhc, err};
#pragma unroll
    for (int k = 0; k < H_NCOUNT; k++) {
        if (k == H_STORED || k == H_COUNTED) continue;
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
    const unsigned long long s64 = wave_sum64(stored), c64 = wave_sum64(counted);
    if (lane == 0 && s64) atomicAdd(A.counters + H_STORED, s64);
    if (lane == 0 && c64) atomicAdd(A.counters + H_COUNTED, c64);
}

}  // namespace rtd
