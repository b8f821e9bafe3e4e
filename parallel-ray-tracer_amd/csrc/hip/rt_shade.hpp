// rt_shade.hpp — radiance queries: the reference's raytrace() for caller-supplied rays (rt_shade_rays, rt_hip.h).
//
//   rgb[i] = vec_constrain(raytrace(o_i, d_i, 0), 0, 1) (cpu/src/raytracer.c:101-177, main.c:234), a frame's pixel for a
//   ray no pinhole camera on a pixel grid has to express; `unclamped`: raytrace()'s value as is.
//
// k_shade deals chunks of QUERY_CHUNK consecutive rays to persistent waves, as k_query does, and has two forms.
//
// Lockstep (shade_lockstep): one ray per lane through the reference recursion, path_step's (rt_kernels.hpp). What the
// frame kernels know about their rays holds here from level 1 on only: a reflection or shadow ray is a unit-length ray
// from a point of the scene, whoever sent the path. Level 0 is the caller's ray, so its closest hit goes through
// closest_q (rt_query.hpp: the per-ray domain test, the per-ray view, the tie re-walk, ref_reaches) and is shaded by
// path_shade, path_step's second half. A path whose level-0 ray is outside query_domain may hit a triangle at a point
// o + d * t rounded far from the scene (an origin 2^20 directions away, a direction of 2^30): nothing is known about
// its later rays either, so it walks the reference tree at every level and for every shadow ray (counted in
// strict_paths). The strict walks return the reference's bits for any ray, so this is routing only.
//
// Pool (shade_pool; the fast kernel on a wide view): trace_path_dfr (rt_shpool.hpp), the frame kernels' all-levels
// shadow pool, for a pass of 64 rays: the closest hits level by level (level 0 through closest_q), every level's
// shadow rays of the 64 paths as one pool, then the levels' colours and the fold. A strictly routed path stays out of
// it (its lane walks other paths' shadow rays) and runs path_step's recursion on the reference tree afterwards, its
// levels in its own path-buffer slots.
#pragma once
#include "rt_query.hpp"

namespace rtd {

enum { S_RAYS, S_HITS, S_REFL, S_SHAD, S_SKIP, S_STRICT, S_TIE, S_ERR, S_NCOUNT };

struct SArgs {
    DScene s;  // prim set whenever the scene has a primary view: the view is chosen per ray (ray_view)
    const float* origin;
    const float* dir;
    float* rgb;
    unsigned* bgra;
    int* hit;
    float* t;
    int* bounce_hit;
    unsigned long long* counters;  // S_NCOUNT slots of the shade query's own block
    unsigned int* work;            // its own chunk counter
    int n, bounces;
    float o_max;    // the fast walks' bound on max|o| (QArgs::o_max)
    int regroup;    // the pool form: idle lanes of a wave that trigger a refill (1..63)
    int unclamped;  // raytrace()'s value, not the pixel's
    int pad;
};
static_assert(sizeof(SArgs) == sizeof(DScene) + 9 * 8 + 24, "kernel-argument layout: both passes must agree");

// dynamic LDS of the pool form: [wave][level][lane] float4 path buffer, [wave][level][lane] hit triangles, the waves'
// packed-triangle queues (the PB = 2 kernels' layout, rt_shpool.hpp, without their dynamic stack in front)
template <int MAXB>
__host__ __device__ constexpr size_t shade_pool_lds(bool tq) {
    return sizeof(float4) * BLOCK * MAXB + sizeof(int) * BLOCK * MAXB + (tq ? sizeof(int) * (BLOCK / 64) * TQ_WORDS : 0);
}

struct SOut {  // one ray's answer
    v3 col;
    int hit0;
    float t0;
};

__device__ __forceinline__ void shade_store(const SArgs& A, long long i, const SOut& r) {
    store_px(A.rgb, A.bgra, (size_t)i, A.unclamped ? r.col : clamp01(r.col));
    if (A.hit) A.hit[i] = r.hit0;
    if (A.t) A.t[i] = r.t0;
}

// the reference recursion on the reference tree, levels in registers (PB = false) or in the lane's path-buffer slots
template <int MAXB, bool PB>
__device__ __forceinline__ SOut shade_strict(const SArgs& A, long long i, v3 o, v3 d, int* __restrict__ stk, Ctr& c,
                                             float4* pb = nullptr) {
    v3 cols[MAXB];
    int mats[MAXB];
    if constexpr (!PB) {
#pragma unroll
        for (int k = 0; k < MAXB; k++) {
            cols[k] = mk(0.0f, 0.0f, 0.0f);
            mats[k] = 0;
        }
    }
    SOut r = {mk(0.0f, 0.0f, 0.0f), -1, FMAX};
    int L = 0;
    bool tail = false;
    for (int it = 0; it < A.bounces; ++it)
        if (path_step<MAXB, true, false, true, 1, PB>(A.s, A.bounces, it, o, d, cols, mats, L, tail, r.hit0, r.t0,
                                                      A.bounce_hit, (int)i, stk, c, 0u, pb))
            break;
    if constexpr (PB) r.col = fold_pb<MAXB>(A.s, pb, L, tail);
    else r.col = fold_path<MAXB>(A.s, cols, mats, L, tail);
    return r;
}

// One ray per lane (see above). c counts per lane: prim, refl, shad, skip, hits, err (path_step's CTR_INC).
template <int MAXB, bool STRICT, bool TQ>
__device__ __forceinline__ void shade_lockstep(const SArgs& A, long long i, int* __restrict__ stk, int* tq, Ctr& c,
                                               unsigned& nstrict, unsigned& nties) {
    v3 o = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
    v3 d = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
    if (A.bounce_hit)
        for (int k = 0; k < A.bounces; k++) A.bounce_hit[(size_t)i * A.bounces + k] = -2;
    if constexpr (STRICT) {
        shade_store(A, i, shade_strict<MAXB, false>(A, i, o, d, stk, c));
    } else {
        const DScene& s = A.s;
        const bool sp = !query_domain(o, d, A.o_max);  // the whole path on the reference tree
        nstrict += sp ? 1u : 0u;
        v3 cols[MAXB];
        int mats[MAXB];
#pragma unroll
        for (int k = 0; k < MAXB; k++) {
            cols[k] = mk(0.0f, 0.0f, 0.0f);
            mats[k] = 0;
        }
        SOut r = {mk(0.0f, 0.0f, 0.0f), -1, FMAX};
        int L = 0;
        bool tail = false;
        for (int it = 0; it < A.bounces; ++it) {
            float best;
            int nd, orig;
            if (it == 0) {
                unsigned ev = 0;
                c.prim++;
                orig = closest_q<TQ>(s, o, d, A.o_max, best, nd, stk, c, ev, tq);
                nties += (ev & QE_TIE) >> 4;
                r.hit0 = orig;
                r.t0 = best;
            } else {  // a unit-length ray from a point of the scene: the frame kernels' situation
                c.refl++;
                if (sp) orig = closest<true, false>(s, o, d, best, nd, stk, c);
                else orig = closest<false, false, true, false, false, TQ>(s, o, d, best, nd, stk, c, nullptr, WSTACK, true, tq);
            }
            if (A.bounce_hit) A.bounce_hit[(size_t)i * A.bounces + it] = orig;
            bool end;
            if (sp) end = path_shade<MAXB, true, false, true>(s, A.bounces, it, orig, best, nd, o, d, cols, mats, L, tail, stk, c);
            else end = path_shade<MAXB, false, false, true, 1, false, false, TQ>(s, A.bounces, it, orig, best, nd, o, d, cols,
                                                                              mats, L, tail, stk, c, 0u, nullptr, nullptr,
                                                                              WSTACK, tq);
            if (end) break;
        }
        r.col = fold_path<MAXB>(s, cols, mats, L, tail);
        shade_store(A, i, r);
    }
}

// trace_path_dfr's Q for a caller-supplied ray (rt_shpool.hpp): the lane's LDS slots, its levels' closest hits, its
// outputs
template <bool TQ_, class CL, class OUT>
struct ShadePath {
    static constexpr bool TQ = TQ_;
    float4* pb;
    int* hid;
    int* tq;
    CL closest_at;
    OUT out;
};
template <bool TQ, class CL, class OUT>
__device__ __forceinline__ ShadePath<TQ, CL, OUT> shade_path(float4* pb, int* hid, int* tq, CL cl, OUT out) {
    return ShadePath<TQ, CL, OUT>{pb, hid, tq, cl, out};
}

// A pass of up to 64 rays (ray base + lane, lane < cnt) through trace_path_dfr; called by every lane of the wave.
// pb / hid: the lane's level-0 slots of the wave's path buffer and hit-triangle array; tq: the wave's queue (TQ).
template <int MAXB, bool TQ>
__device__ __forceinline__ void shade_pool(const SArgs& A, long long base, int cnt, int* __restrict__ stk, float4* pb,
                                           int* hid, int* tq, Ctr& c, UCtr& u, unsigned& nstrict, unsigned& nties) {
    const DScene& s = A.s;
    const int lane = (int)(threadIdx.x & 63u);
    const bool valid = lane < cnt;
    const long long i = base + (valid ? lane : 0);
    v3 o = mk(0.0f, 0.0f, 0.0f), d = o;
    if (valid) {
        o = mk(A.origin[3 * i], A.origin[3 * i + 1], A.origin[3 * i + 2]);
        d = mk(A.dir[3 * i], A.dir[3 * i + 1], A.dir[3 * i + 2]);
        if (A.bounce_hit)
            for (int k = 0; k < A.bounces; k++) A.bounce_hit[(size_t)i * A.bounces + k] = -2;
    }
    const bool sp = valid && !query_domain(o, d, A.o_max);
    nstrict += sp ? 1u : 0u;
    SOut r = {mk(0.0f, 0.0f, 0.0f), -1, FMAX};
    const auto q = shade_path<TQ>(
        pb, hid, tq,
        [&](int it, v3 ro, v3 rd, float& best, int& nd) {
            if (it == 0) {
                unsigned ev = 0;
                const int orig = closest_q<TQ>(s, ro, rd, A.o_max, best, nd, stk, c, ev, tq);
                nties += (ev & QE_TIE) >> 4;
                return orig;
            }
            return closest<false, false, true, false, false, TQ>(s, ro, rd, best, nd, stk, c, nullptr, WSTACK, true, tq);
        },
        [&](int it, int orig, float best) {
            if (it == 0) {
                r.hit0 = orig;
                r.t0 = best;
            }
            if (A.bounce_hit) A.bounce_hit[(size_t)i * A.bounces + it] = orig;
        });
    r.col = trace_path_dfr<MAXB, false>(A, valid && !sp, o, d, stk, c, u, -1, nullptr, WSTACK, q);
    if (sp) r = shade_strict<MAXB, true>(A, i, o, d, stk, c, pb);
    if (valid) shade_store(A, i, r);
}

// MAXB: the levels a path keeps (4 / 8, FOR_MAXB). STRICT: every walk on the reference tree (RT_KERNEL_STRICT).
// TQ: packed triangle tests through the wave's LDS queue (ctx->tq_ok). POOL: the pool form (fast kernel, wide views;
// launched with shade_pool_lds<MAXB>(TQ) bytes of dynamic LDS).
template <int MAXB, bool STRICT, bool TQ, bool POOL>
__global__ __attribute__((amdgpu_flat_work_group_size(1, BLOCK), amdgpu_waves_per_eu(POOL ? 2 : 3)))
void k_shade(SArgs A) {
    static_assert(!(POOL && STRICT), "the pool form serves the fast kernel");
    __shared__ int lds[STACK * BLOCK];
    int* stk = lds + threadIdx.x;
    int* tq = nullptr;
    float4* pb = nullptr;
    int* hid = nullptr;
    if constexpr (POOL) {
        extern __shared__ int lds_dyn[];
        float4* pb0 = (float4*)lds_dyn;
        const size_t wl = (size_t)((threadIdx.x >> 6) * MAXB) * 64 + (threadIdx.x & 63);
        pb = pb0 + wl;
        hid = (int*)(pb0 + (size_t)BLOCK * MAXB) + wl;
        if constexpr (TQ) tq = (int*)(pb0 + (size_t)BLOCK * MAXB) + BLOCK * MAXB + (threadIdx.x >> 6) * TQ_WORDS;
    } else if constexpr (TQ && !STRICT) {
        tq = tq_static();
    }
    if constexpr (TQ && !STRICT) tq_clear(tq);
    const int lane = threadIdx.x & 63;
    const unsigned n_chunks = ((unsigned)A.n + QUERY_CHUNK - 1) / QUERY_CHUNK;
    Ctr c = {};
    UCtr u = {};
    unsigned strict = 0, ties = 0;
    for (;;) {
        unsigned ch = 0;
        if (lane == 0) ch = atomicAdd(A.work, 1u);
        ch = __builtin_amdgcn_readfirstlane(__shfl(ch, 0, 64));
        if (ch >= n_chunks) break;
        for (int pass = 0; pass < QUERY_CHUNK / 64; pass++) {
            const long long base = (long long)ch * QUERY_CHUNK + pass * 64;
            if (base >= A.n) break;
            if constexpr (POOL) {
                const int cnt = (int)(A.n - base < 64 ? A.n - base : 64);
                shade_pool<MAXB, TQ>(A, base, cnt, stk, pb, hid, tq, c, u, strict, ties);
            } else {
                const long long i = base + (int)lane_now();
                if (i < A.n) shade_lockstep<MAXB, STRICT, TQ>(A, i, stk, tq, c, strict, ties);
            }
        }
    }
    // (the pool form's wave-uniform counts, u, are lane 0's share)
    const bool l0 = lane == 0;
    const unsigned v[S_NCOUNT] = {c.prim + (l0 ? u.prim : 0u), c.hits + (l0 ? u.hits : 0u), c.refl + (l0 ? u.refl : 0u),
                                  c.shad + (l0 ? u.shad : 0u), c.skip + (l0 ? u.skip : 0u), strict, ties + c.fb, c.err};
#pragma unroll
    for (int k = 0; k < S_NCOUNT; k++) {
        const unsigned sum = wave_sum(v[k]);
        if (l0 && sum) atomicAdd(A.counters + k, (unsigned long long)sum);
    }
}

}  // namespace rtd
