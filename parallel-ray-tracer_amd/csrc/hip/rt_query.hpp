// rt_query.hpp — ray queries: the reference's two traversals for caller-supplied rays (rt_trace_rays, rt_hip.h).
//
//   RT_QUERY_CLOSEST   (hit, t) = what bvh_traverse (cpu/src/bvh.c:317-358) leaves in index and t, the first-found rule
//                      at exact ties included; hit mapped to the original triangle index, t = FLT_MAX on a miss
//   RT_QUERY_OCCLUDED  !bvh_light_traverse (bvh.c:269-315) with light_dist2 = max_dist2 (no back-face early-out)
//
// k_query has two forms. RT_QUERY_OCCLUDED on a wide view runs the pool form (occluded_pool below: a lane whose walk
// ends takes the chunk's next ray), which the measurements kept; RT_QUERY_CLOSEST runs the lockstep form, whose pool
// form was built, measured and removed (it won on permuted rays and lost on row-major ones: DESIGN.md §3k). Lockstep: persistent waves take chunks of QUERY_CHUNK consecutive rays from one counter (one
// returning atomic per chunk) and walk them one ray per lane with the frame kernels' own walks (closest_wide /
// visible_wide / closest_walk / visible_walk, the 3-wave k_persist build's template choices). The frame kernels know
// their rays (a camera's primary directions, unit-length reflection and shadow rays from points of the scene); a
// query knows nothing about its rays, so every assumption the fast walks make is tested PER RAY here (query_domain,
// shadow_domain, ray_view) and a ray outside them walks the reference tree from the start.
#pragma once
#include "rt_kernels.hpp"
#include "rt_shpool.hpp"

namespace rtd {

constexpr int QUERY_CHUNK = 256;  // rays per dealt chunk: 4 lockstep passes of a wave
enum { Q_RAYS, Q_HITS, Q_UNIT, Q_SHORT, Q_FULL, Q_STRICT, Q_TIE, Q_ERR, Q_NCOUNT };

struct QArgs {
    DScene s;  // prim set whenever the scene has a primary view: the view is chosen per ray (ray_view)
    const float* origin;
    const float* dir;
    const float* max_dist2;
    int* hit;
    float* t;
    int* occluded;
    unsigned long long* counters;  // Q_NCOUNT slots of the query's own block
    unsigned int* work;            // the query's own chunk counter
    int n;
    float o_max;  // the fast walks' bound on max|o| (4 x the scene's coordinate magnitude mx, rt_hip.hip)
    int regroup;  // the pool form: idle lanes of a wave that trigger a refill (1..63)
    int pad;
};
static_assert(sizeof(QArgs) == sizeof(DScene) + 8 * 8 + 16, "kernel-argument layout: both passes must agree");

// what became of one ray (closest_q / visible_q), counted by the kernel: the view that served its fast walk, or
// QE_STRICT (outside the fast walks' domain: the reference tree from the start); QE_TIE: its fast walk was re-walked
enum : unsigned { QE_UNIT = 1, QE_SHORT = 2, QE_FULL = 4, QE_STRICT = 8, QE_TIE = 16 };

__device__ __forceinline__ bool finite3(v3 a) {
    return __builtin_fabsf(a.x) <= FMAX && __builtin_fabsf(a.y) <= FMAX && __builtin_fabsf(a.z) <= FMAX;  // (NaN: false)
}
__device__ __forceinline__ float maxabs(v3 a) {
    return fmaxf(fmaxf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z));
}

// The fast walks' domain, whatever the kind:
//   - every component of o and d finite;
//   - 2^-20 <= max|d_i| <= 2^20: the slab constants (1 / d, scaled by 2^-40 in ray_pre_closest and by a node's 2^e)
//     stay far from the denormals and from overflow, every hit distance of a ray that starts within o_max of the
//     scene stays below 2^20 * 9 mx, and a component below safe_dir's 1e-20 (treated as 0) moves the ray by less than
//     2^-40 mx over that distance, far inside the boxes' inflation;
//   - max|o_i| <= o_max = 4 mx: the slab tests' rounding reach grows with the origin's magnitude (o / d is rounded at
//     the origin's ulp); at 4 mx it is at most ~23 u mx / |d| against the inflation's 256 u mx / |d|. ray_pre_closest's
//     shift (o / d + BOX_TMIN) adds one rounding of u max(|o / d|, BOX_TMIN): the first is in the 23 u, the second is
//     u 1e-3 in t, u 1e-3 |d| in space -- at |d| = 2^20 that is 63 u mx for the smallest mx (16), 86 u mx in all,
//     a third of the inflation (the two would meet at |d| = 2^21.8).
__device__ __forceinline__ bool query_domain(v3 o, v3 d, float o_max) {
    const float dm = maxabs(d);
    return finite3(o) && finite3(d) && dm >= 0x1p-20f && dm <= 0x1p20f && maxabs(o) <= o_max;
}

// The view a ray may walk, from its computed squared length l2 = fl(d.d): three products and two sums of positive
// terms, so the true |d|^2 <= l2 / (1 - u)^3 <= l2 (1 + 3 u + 7 u^2), u = 2^-24.
//   unit view   : l2 <= 1 + 2 u (the float after 1) implies |d|^2 <= 1 + 5 u + 14 u^2 < (1 + 3 u)^2, the bound of the
//                 unit view's derivation (rt_hip.hip hittable);
//   primary view: l2 <= 9 - 2^-17 (8.99999237: 128 u below 9) implies |d|^2 < 9 (1 - 10 u) < 9 = PRIMARY_D^2;
//   else the full view. A false "no" costs speed only.
constexpr float UNIT_L2 = 0x1.000002p0f, PRIM_L2 = 0x1.1ffffp3f;
__device__ __forceinline__ int ray_view(const DScene& s, v3 d) {
    const float l2 = dot(d, d);
    if (l2 <= UNIT_L2 && s.unit.nodes) return 0;
    if (l2 <= PRIM_L2 && s.prim.nodes) return 1;
    return 2;
}

// The fast shadow walk (visible_wide / visible_walk<false>: shadow_reach, ray_pre_shadow) assumes |d| = 1 within
// 2 ulp and a finite positive reach: l2 in [1 - 4 u, 1 + 2 u] gives |d| in [1 - 4 u, 1 + 3 u] (its 1e-3 margin of the
// reach covers that 100x over), and a finite max_dist2 > 0 a finite reach (sqrt(FLT_MAX) * 1.001 + 1e-5 o_max is).
__device__ __forceinline__ bool shadow_domain(v3 o, v3 d, float ld2, float o_max) {
    const float l2 = dot(d, d);
    return query_domain(o, d, o_max) && l2 >= 0x1.fffff8p-1f && l2 <= UNIT_L2 && ld2 > 0.0f && ld2 <= FMAX;
}

// closest() for a query ray: the same policy (fast walk; a tie re-walked on the reference tree bounded at the tie; a
// degenerate ray on a face checked by ref_reaches), with the view chosen per ray and the domain tested first. The
// fast walks keep their view in scalar registers (walk_base), so the wave walks the views its rays chose one after
// another (a coherent ray set chooses one); the rays handed back and the rays outside the domain then walk the
// reference tree together. nd: the side of the winning triangle the ray hit (the walk's that answered), which a
// caller that shades the hit needs (rt_shade.hpp) and the closest-hit query does not.
template <bool TQ>
__device__ __forceinline__ int closest_q(const DScene& s, v3 o, v3 d, float o_max, float& best, int& nd,
                                         int* __restrict__ stk, Ctr& c, unsigned& ev, int* tq) {
    int hp = -1, orig = -1;
    bool tie = false, done = false;
    nd = 0;
    best = FMAX;
    const bool dom = query_domain(o, d, o_max);
    const bool deg = degenerate(d);
    const bool face = deg && !degenerate_ok(s, o, d);
    const bool chk = deg && s.ref_path != nullptr;  // (every degenerate ray's winner is checked: closest())
    const bool fast = dom && (!face || chk);
    if (s.wide.nodes) {
        const int view = ray_view(s, d);
#pragma unroll 1
        for (int v = 0; v < 3; v++) {
            const bool mine = fast && view == v;
            if (!__builtin_amdgcn_readfirstlane((int)(__ballot(mine) != 0ull))) continue;
            const DWide W = v == 0 ? s.unit : v == 1 ? s.prim : s.wide;
            if (mine) {
                closest_wide<false, false, false, TQ>(W, o, d, best, hp, nd, tie, stk, c, WSTACK, tq);
                if (!tie) {
                    orig = hp >= 0 ? W.tri_orig[hp] : -1;
                    done = true;
                }
            }
        }
        if (fast) ev |= view == 0 ? QE_UNIT : view == 1 ? QE_SHORT : QE_FULL;
    } else if (fast) {
        closest_walk<false, false>(s.acc, o, d, best, hp, nd, tie, stk, c);
        if (!tie) {
            orig = hp >= 0 ? s.acc.tri_orig[hp] : -1;
            done = true;
        }
        ev |= QE_FULL;
    }
    if (fast) {
        if (done && (!chk || orig < 0 || ref_reaches(s, orig, o, d))) return orig;
        ev |= QE_TIE;
    } else {
        ev |= QE_STRICT;
    }
    if (TIE_BOUNDED && fast && !done) {  // an exact tie at t = best (closest(): tie_bound, TIE_CUT)
        const float tb = tie_bound(o, best), cut = best - (tb - best);
        hp = -1;
        nd = 0;
        best = tb;
        closest_walk<true, false, true, TIE_CUT>(s.ref, o, d, best, hp, nd, tie, stk, c, cut);
        if (hp >= 0) return s.ref.tri_orig[hp];
    }
    hp = -1;
    best = FMAX;
    nd = 0;
    closest_walk<true, false>(s.ref, o, d, best, hp, nd, tie, stk, c);
    return hp >= 0 ? s.ref.tri_orig[hp] : -1;
}
template <bool TQ>
__device__ __forceinline__ int closest_q(const DScene& s, v3 o, v3 d, float o_max, float& best, int* __restrict__ stk,
                                         Ctr& c, unsigned& ev, int* tq) {
    int nd;
    return closest_q<TQ>(s, o, d, o_max, best, nd, stk, c, ev, tq);
}

// visible() for a query ray
template <bool TQ>
__device__ __forceinline__ bool visible_q(const DScene& s, v3 o, v3 d, float ld2, float o_max, int* __restrict__ stk,
                                          Ctr& c, unsigned& ev, int* tq) {
    if (shadow_domain(o, d, ld2, o_max) && (!degenerate(d) || degenerate_ok(s, o, d))) {
        if (s.wide.nodes) {
            ev |= s.unit.nodes ? QE_UNIT : QE_FULL;
            return visible_wide<false, false, false, TQ>(wide_for(s, true), o, d, ld2, stk, c, WSTACK, tq);
        }
        ev |= QE_FULL;
        return visible_walk<false, false>(s.acc, o, d, ld2, stk, c);
    }
    ev |= QE_STRICT;
    return visible_walk<true, false>(s.ref, o, d, ld2, stk, c);
}

// The pool form of RT_QUERY_OCCLUDED (wide views only): one chunk's rays as ONE per-wave pool -- shadow_pool's loop
// (rt_shpool.hpp) with the ray fetched from global memory instead of from (owner, level, light). The chunk is classified
// 64 rays at a time (advance: lane l tests ray 64 cl + l against shadow_domain; cm = the pass's rays the fast walk
// serves, still unassigned, in scalar registers; a lane remembers in `smine` which of its own rays are outside the
// domain); a lane whose walk ends takes the next unassigned ray of cm (the k-th idle lane the k-th set bit), the refill
// happening once `regroup` lanes are idle; no workgroup barrier. After the pool has drained, the rays outside the
// domain walk the reference tree, one pass at a time, together. Every ray's answer is the one the lockstep form
// computes: its walk does not depend on which lane runs it or when. Called by every lane of the wave.
template <bool TQ>
__device__ __forceinline__ void occluded_pool(const QArgs& A, long long base, int cnt, int* __restrict__ stk, int* tq,
                                              Ctr& c, unsigned& hits, unsigned& nunit, unsigned& nfull,
                                              unsigned& nstrict) {
    const DScene& s = A.s;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long all = uni64(__ballot(1));
    const DWide& W = wide_for(s, true);
    const gnodes nbase = walk_base(W.nodes);
    const int np = (cnt + 63) >> 6, regroup = A.regroup;
    int cl = -1;                // the pass being dealt (wave-uniform)
    unsigned long long cm = 0;  // its fast rays still unassigned
    unsigned smine = 0;         // bit p: this lane's ray of pass p walks the reference tree
    auto advance = [&]() {      // classify the next pass with fast rays (every lane takes part, busy or not)
        while (cm == 0 && cl + 1 < np) {
            cl = uni(cl + 1);
            const int off = 64 * cl + (int)lane;
            bool f = false, st = false;
            if (off < cnt) {
                const long long i = base + off;
                const v3 ro = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
                const v3 rd = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
                f = shadow_domain(ro, rd, A.max_dist2[i], A.o_max) && (!degenerate(rd) || degenerate_ok(s, ro, rd));
                st = !f;
            }
            if (st) smine |= 1u << cl;
            cm = uni64(__ballot(f));
            const unsigned nf = (unsigned)__builtin_popcountll(cm);
            const unsigned ns = (unsigned)__builtin_popcountll(uni64(__ballot(st)));
            if (lane == 0u) {  // (per-lane counters, summed over the wave at the end)
                if (s.unit.nodes) nunit += nf;
                else nfull += nf;
                nstrict += ns;
            }
        }
    };
    // this lane's ray (its offset in the chunk) and its walk state (visible_wide's)
    bool busy = false;
    int wo = 0;
    v3 o = mk(0.0f, 0.0f, 0.0f), d = o;
    RayPre p = {};
    unsigned oct = 0;
    float ld2 = 0.0f, reach = 0.0f, best = FMAX;
    int sp = 0;
    TopC tc;
    WNode N = {};
    for (;;) {
        advance();
        const unsigned long long idle = uni64(__ballot(!busy));
        if (idle == all && cm == 0) break;  // (advance left cm == 0: no pass is left)
        if (cm != 0) {  // refill every idle lane while there is work (shadow_pool's rounds, one per pass)
            unsigned long long req = idle;
            bool got = false;
            while (req != 0ull && cm != 0ull) {
                const unsigned nreq = (unsigned)__builtin_popcountll(req), nav = (unsigned)__builtin_popcountll(cm);
                const unsigned k = __builtin_amdgcn_mbcnt_hi((unsigned)(req >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((unsigned)req, 0u));
                if (((req >> lane) & 1ull) && k < nav) {
                    wo = kth_bit(cm, k) | (cl << 6);
                    got = true;
                }
                if (nreq >= nav) {
                    req = uni64(drop_low(req, nav));
                    cm = 0ull;
                    advance();
                } else {
                    cm = uni64(drop_low(cm, nreq));
                    req = 0ull;
                }
            }
            if (got) {
                const long long i = base + wo;
                o = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
                d = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
                ld2 = A.max_dist2[i];
                reach = shadow_reach(o, ld2);
                p = ray_pre_shadow(o, d, reach);
                oct = (p.ix < 0.0f ? 1u : 0u) | (p.iy < 0.0f ? 2u : 0u) | (p.iz < 0.0f ? 4u : 0u);
                best = FMAX;
                sp = 0;
                N = wload_at(nbase, 0);
                busy = true;
            }
        }
        // walk until the wave is idle, or enough of it to refill while work is left: visible_wide's loop, one
        // ballot per step
        const bool more = cm != 0 || cl + 1 < np;
        for (;;) {
            unsigned th = 0u;
            int tb = 0, next = -1;
            if (busy) {  // one step of visible_wide
                unsigned nh, imask, nlf;
                int cb;
                pin_node(N);
                wide_node<false, LATE_TRIS, SHADOW_CLAMP ? 1 : 0>(N, p, oct, fminf(best * PRUNE_SLACK, reach), nh, th, cb, tb,
                                                          imask, nlf, SHADOW_ORDER_XOR);
                const unsigned m0 = __float_as_uint(N.f1.z), m1 = __float_as_uint(N.f1.w);
                next = wide_step_next<false>(nh, cb, imask, oct ^ SHADOW_ORDER_XOR, sp, tc, stk, WSTACK);
                N = wload_at(nbase, next >= 0 ? next : 0);  // unconditional (closest_wide)
                top_reload<false>(sp, tc, stk, WSTACK);
                if constexpr (LATE_TRIS) th = leaf_tris<false>(th, m0, m1, nlf);
            }
            bool occ = false, seq = true;
            if constexpr (TQ) {  // packed triangle tests, as shadow_pool's
                const unsigned nt = (unsigned)__builtin_popcount(th);
                if (uni64(__ballot(nt >= TQ_MIN)) != 0ull) {
                    unsigned* cnt_w = reinterpret_cast<unsigned*>(tq + TQ_CNT);
                    unsigned pos = 0u;
                    if (nt) pos = atomicAdd(cnt_w, nt);
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    const unsigned T = (unsigned)uni((int)atomicAdd(cnt_w, 0u));
                    if (T <= (unsigned)TQ_CAP) {
                        seq = false;
                        for (unsigned m = th; m; m &= m - 1u) tq[pos++] = (int)((lane << 26) | (unsigned)(tb + __builtin_ctz(m)));
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                        for (unsigned jb = 0u; jb < T; jb += 64u) {
                            const unsigned j = jb + lane;
                            const unsigned job = j < T ? (unsigned)tq[j] : lane << 26;
                            const int ow = (int)(job >> 26);
                            const v3 oo = mk(__shfl(o.x, ow, 64), __shfl(o.y, ow, 64), __shfl(o.z, ow, 64));
                            const v3 dd = mk(__shfl(d.x, ow, 64), __shfl(d.y, ow, 64), __shfl(d.z, ow, 64));
                            const float l2 = __shfl(ld2, ow, 64);
                            if (j < T) {
                                int k;
                                const float tt = hit_triangle<SHADOW_RCP>(oo, dd, W.tris + 3 * (int)(job & 0x3FFFFFFu), k);
                                if (tt < FMAX) {
                                    const v3 q = add(oo, mul(dd, tt));
                                    const v3 oi = sub(oo, q);
                                    if (l2 > dot(oi, oi)) tq[TQ_OCC + ow] = 1;
                                    atomicMax(reinterpret_cast<unsigned*>(tq + TQ_T + ow), ~__float_as_uint(tt));
                                }
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                        if (nt) {
                            occ = tq[TQ_OCC + lane] != 0;
                            const unsigned tw = (unsigned)tq[TQ_T + lane];
                            if (tw) best = fminf(best, __uint_as_float(~tw));
                            tq[TQ_OCC + lane] = 0;
                            tq[TQ_T + lane] = 0;
                        }
                    }
                    if (lane == 0u) *cnt_w = 0u;
                }
            }
            if (busy) {
                while (seq && th) {
                    const int i = tb + __builtin_ctz(th);
                    th &= th - 1u;
                    int k;
                    const float tt = hit_triangle<SHADOW_RCP>(o, d, W.tris + 3 * i, k);
                    if (tt < best) {
                        best = tt;
                        const v3 q = add(o, mul(d, best));
                        const v3 oi = sub(o, q);
                        if (ld2 > dot(oi, oi)) {
                            occ = true;
                            break;
                        }
                    }
                }
                if (occ || next < 0) {
                    if (!occ && next == -2) c.err++;
                    A.occluded[base + wo] = occ ? 1 : 0;
                    hits += occ ? 1u : 0u;
                    busy = false;
                }
            }
            const unsigned long long id2 = uni64(__ballot(!busy));
            if (id2 == all || (more && __builtin_popcountll(id2) >= regroup)) break;
        }
    }
    if constexpr (TQ) tq_clear(tq);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    // the rays outside the fast walk's domain: the reference's walk, a pass at a time
    for (int ps = 0; ps < np; ps++) {
        if (!((smine >> ps) & 1u)) continue;
        const long long i = base + 64 * ps + (int)lane;
        const v3 ro = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
        const v3 rd = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
        const bool vis = visible_walk<true, false>(s.ref, ro, rd, A.max_dist2[i], stk, c);
        A.occluded[i] = vis ? 0 : 1;
        hits += vis ? 0u : 1u;
    }
}

// KIND: RT_QUERY_CLOSEST (0) / RT_QUERY_OCCLUDED (1). STRICT: every ray on the reference tree (RT_KERNEL_STRICT).
// TQ: packed triangle tests through the wave's LDS queue (the 3-wave k_persist build's; off for scenes of 2^26 or more
// triangles and under RT_FLAG_UNPACKED_TRIS).
// POOL: RT_QUERY_OCCLUDED's pool form (occluded_pool; fast kernel, wide views).
template <int KIND, bool STRICT, bool TQ, bool POOL = false>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(3)))
void k_query(QArgs A) {
    __shared__ int lds[STACK * BLOCK];
    int* stk = lds + threadIdx.x;
    int* tq = nullptr;
    if constexpr (TQ && !STRICT) {
        tq = tq_static();
        tq_clear(tq);
    }
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    Ctr c = {};
    unsigned rays = 0, hits = 0, unit = 0, shrt = 0, full = 0, strict = 0, ties = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        if constexpr (POOL) {
            static_assert(KIND == 1 && !STRICT, "the pool form serves the fast occlusion query");
            const long long base = (long long)ch * QUERY_CHUNK;
            const int cnt = (int)(A.n - base < QUERY_CHUNK ? A.n - base : QUERY_CHUNK);
            rays += lane == 0 ? (unsigned)cnt : 0u;
            occluded_pool<TQ>(A, base, cnt, stk, tq, c, hits, unit, full, strict);
            continue;
        }
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long i = (long long)ch * QUERY_CHUNK + pass * 64 + (int)lane_now();
            if (i >= A.n) continue;
            rays++;
            unsigned ev = 0;
            const v3 o = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
            const v3 d = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
            if constexpr (KIND == 0) {
                float best = FMAX;
                int orig;
                if constexpr (STRICT) {
                    int hp = -1, nd = 0;
                    bool tie = false;
                    closest_walk<true, false>(A.s.ref, o, d, best, hp, nd, tie, stk, c);
                    orig = hp >= 0 ? A.s.ref.tri_orig[hp] : -1;
                } else {
                    orig = closest_q<TQ>(A.s, o, d, A.o_max, best, stk, c, ev, tq);
                }
                if (orig >= 0) hits++;
                if (A.hit) A.hit[i] = orig;
                if (A.t) A.t[i] = best;
            } else {
                const float ld2 = A.max_dist2[i];
                bool vis;
                if constexpr (STRICT) vis = visible_walk<true, false>(A.s.ref, o, d, ld2, stk, c);
                else vis = visible_q<TQ>(A.s, o, d, ld2, A.o_max, stk, c, ev, tq);
                if (!vis) hits++;
                A.occluded[i] = vis ? 0 : 1;
            }
            unit += ev & QE_UNIT;
            shrt += (ev & QE_SHORT) >> 1;
            full += (ev & QE_FULL) >> 2;
            strict += (ev & QE_STRICT) >> 3;
            ties += (ev & QE_TIE) >> 4;
        }
    }
    const unsigned v[Q_NCOUNT] = {rays, hits, unit, shrt, full, strict, ties, c.err};
#pragma unroll
    for (int k = 0; k < Q_NCOUNT; k++) {
        const unsigned sum = wave_sum(v[k]);
        if (lane == 0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
}

}  // namespace rtd
