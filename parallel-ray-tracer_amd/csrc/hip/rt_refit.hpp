// rt_refit.hpp — vertex updates (rt_update_vertices): every view of the uploaded scene refitted on the device to new
// triangle coordinates, topology kept.
//
//   1. k_plan          read-only pass over the new coordinates: their magnitude (the inflation's and the query domain's),
//                      a non-finite flag, and per subset view (unit, primary) the triangles that became hittable but
//                      are not in the view (k_member's bitmap of its tri_orig) -- those force that view's rebuild
//   2. k_tri_records   the 48-B triangle records of a view in its own order (rt_hip.hip tri_records' roundings);
//      k_shade_normals the two shading normals per triangle (triangle_init's, cpu/src/triangle.c:14-19)
//   3. k_bin_level     a binary view's child-pair records, one launch per tree level, deepest first: a leaf child's
//                      box is the reference's fold (fminf / fmaxf from +-1e10, bvh.c:61-71) over its triangles, an
//                      interior child's comes from the scratch array of exact record boxes written one launch earlier;
//      k_faces         the records' face coordinates per axis, then sorted (hipcub, rt_hip.hip)
//   4. k_wide_level    an 8-wide view's nodes, one launch per level (levels are contiguous ranges of the breadth-first
//                      layout): each slot's exact box, the node's own into the scratch array, then the shared
//                      re-quantisation (rt_quant.hpp requantise: the code rth_wbvh_refit runs on the host)
// The launch boundary is the only synchronisation between levels. Every index read here was written by this library's
// own builders (rt_hip.hip build_view, rt_wide.cpp), which bound them at upload.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_device.hpp"
#include "rt_quant.hpp"

namespace rtr {

enum { P_MX = 0, P_BAD = 1, P_JOIN_UNIT = 2, P_JOIN_PRIM = 3, P_WORDS = 4 };  // k_plan's output words

__global__ __launch_bounds__(256) void k_member(const int* __restrict__ orig, int n, unsigned* __restrict__ bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicOr(bits + (orig[i] >> 5), 1u << (orig[i] & 31));
}

// |n|^2 of the triangle's record normal in double, as rt_hip.hip hittable() forms it before its square root
__device__ __forceinline__ double normal_len2(const float* __restrict__ p) {
    const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
    const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    return (double)nx * nx + (double)ny * ny + (double)nz * nz;
}

// x_unit / x_prim: the smallest double whose (correctly rounded) square root reaches hittable()'s threshold for that
// view, so that len2 >= x is hittable()'s own comparison without a device square root; ubits / pbits nullable (no
// such view: nothing can join it). plan[P_MX] starts at the bits of 16.0f (scene_magnitude's floor).
__global__ __launch_bounds__(256) void k_plan(const float* __restrict__ coords, int n, const unsigned* __restrict__ ubits,
                                              const unsigned* __restrict__ pbits, double x_unit, double x_prim,
                                              unsigned* __restrict__ plan) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float mx = 0.0f;
    if (i < n) {
        const float* p = coords + 9 * (size_t)i;
        bool bad = false;
        for (int k = 0; k < 9; k++) {
            const float a = __builtin_fabsf(p[k]);
            if (!(a <= rtd::FMAX)) bad = true;
            else mx = fmaxf(mx, a);
        }
        if (bad) atomicOr(plan + P_BAD, 1u);
        const double l2 = normal_len2(p);
        const unsigned bit = 1u << (i & 31);
        if (ubits && l2 >= x_unit && !(ubits[i >> 5] & bit)) atomicAdd(plan + P_JOIN_UNIT, 1u);
        if (pbits && l2 >= x_prim && !(pbits[i >> 5] & bit)) atomicAdd(plan + P_JOIN_PRIM, 1u);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(plan + P_MX, (unsigned)__float_as_int(mx));  // (non-negative floats)
}

__global__ __launch_bounds__(256) void k_tri_records(const float* __restrict__ coords, const int* __restrict__ orig,
                                                     int n, float4* __restrict__ tris) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = coords + 9 * (size_t)orig[i];
    const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
    const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    tris[3 * (size_t)i + 0] = make_float4(p[0], p[1], p[2], e1x);
    tris[3 * (size_t)i + 1] = make_float4(e1y, e1z, e2x, e2y);
    tris[3 * (size_t)i + 2] = make_float4(e2z, nx, ny, nz);
}

__global__ __launch_bounds__(256) void k_shade_normals(const float* __restrict__ coords, int n, float4* __restrict__ shade) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = coords + 9 * (size_t)i;
    const rtd::v3 a = rtd::mk(p[0], p[1], p[2]), b = rtd::mk(p[3], p[4], p[5]), c = rtd::mk(p[6], p[7], p[8]);
    const rtd::v3 e1 = rtd::sub(b, a), e2 = rtd::sub(c, a);
    const rtd::v3 n0 = rtd::normalize(rtd::cross(e1, e2)), n1 = rtd::normalize(rtd::cross(e2, e1));
    const float mat = shade[2 * (size_t)i].w;
    shade[2 * (size_t)i + 0] = make_float4(n0.x, n0.y, n0.z, mat);
    shade[2 * (size_t)i + 1] = make_float4(n1.x, n1.y, n1.z, 0.0f);
}

struct B3 {
    float lx, ly, lz, hx, hy, hz;
};
__device__ __forceinline__ void fold(B3& b, const float* __restrict__ v) {  // aabb_grow_pt, bvh.c:61-64
    b.lx = fminf(b.lx, v[0]);
    b.ly = fminf(b.ly, v[1]);
    b.lz = fminf(b.lz, v[2]);
    b.hx = fmaxf(b.hx, v[0]);
    b.hy = fmaxf(b.hy, v[1]);
    b.hz = fmaxf(b.hz, v[2]);
}

// One level of a binary view (rt_device.hpp DBvh): record list[i] gets both child boxes (grown by inflate > 0 as
// build_view grows them) and leaves its own exact box in exact[2 r], exact[2 r + 1]. The refs in its 4th float4 stay.
__global__ __launch_bounds__(256) void k_bin_level(const int* __restrict__ list, int count, float4* __restrict__ nodes,
                                                   const int2* __restrict__ leaves, const int* __restrict__ orig,
                                                   const float* __restrict__ coords, float4* __restrict__ exact,
                                                   float inflate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int r = list[i];
    const float4 q = nodes[4 * (size_t)r + 3];
    const int ref[2] = {__float_as_int(q.x), __float_as_int(q.y)};
    B3 c[2];
    for (int k = 0; k < 2; k++) {
        c[k] = B3{1e10f, 1e10f, 1e10f, -1e10f, -1e10f, -1e10f};  // bvh.c:104-108; an empty child keeps it
        if (ref[k] == rtd::EMPTY_REF) continue;
        if (ref[k] < 0) {
            const int2 lf = leaves[~ref[k]];
            for (int j = 0; j < lf.y; j++) {
                const float* p = coords + 9 * (size_t)orig[lf.x + j];
                fold(c[k], p);
                fold(c[k], p + 3);
                fold(c[k], p + 6);
            }
        } else {
            const float4 lo = exact[2 * (size_t)ref[k]], hi = exact[2 * (size_t)ref[k] + 1];
            c[k] = B3{lo.x, lo.y, lo.z, hi.x, hi.y, hi.z};
        }
    }
    exact[2 * (size_t)r] = make_float4(fminf(c[0].lx, c[1].lx), fminf(c[0].ly, c[1].ly), fminf(c[0].lz, c[1].lz), 0.0f);
    exact[2 * (size_t)r + 1] = make_float4(fmaxf(c[0].hx, c[1].hx), fmaxf(c[0].hy, c[1].hy), fmaxf(c[0].hz, c[1].hz), 0.0f);
    if (inflate > 0.0f)
        for (int k = 0; k < 2; k++) {
            c[k].lx -= inflate;
            c[k].ly -= inflate;
            c[k].lz -= inflate;
            c[k].hx += inflate;
            c[k].hy += inflate;
            c[k].hz += inflate;
        }
    nodes[4 * (size_t)r + 0] = make_float4(c[0].lx, c[0].ly, c[0].lz, c[0].hx);
    nodes[4 * (size_t)r + 1] = make_float4(c[0].hy, c[0].hz, c[1].lx, c[1].ly);
    nodes[4 * (size_t)r + 2] = make_float4(c[1].lz, c[1].hx, c[1].hy, c[1].hz);
}

// the four face coordinates per record and axis (rt_upload_scene's order): out[a * 4 n + 4 r + k]
__global__ __launch_bounds__(256) void k_faces(const float4* __restrict__ nodes, int n, float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float4 p = nodes[4 * (size_t)r], q = nodes[4 * (size_t)r + 1], e = nodes[4 * (size_t)r + 2];
    const float f[3][4] = {{p.x, p.w, q.z, e.y}, {p.y, q.x, q.w, e.z}, {p.z, q.y, e.x, e.w}};
    for (int a = 0; a < 3; a++)
        for (int k = 0; k < 4; k++) out[(size_t)a * 4 * n + 4 * (size_t)r + k] = f[a][k];
}

__device__ __forceinline__ void load_words(const float4* __restrict__ nodes, int k, uint32_t* W) {
    for (int j = 0; j < 5; j++) {
        const float4 f = nodes[5 * (size_t)k + j];
        W[4 * j + 0] = (uint32_t)__float_as_int(f.x);
        W[4 * j + 1] = (uint32_t)__float_as_int(f.y);
        W[4 * j + 2] = (uint32_t)__float_as_int(f.z);
        W[4 * j + 3] = (uint32_t)__float_as_int(f.w);
    }
}

__device__ __forceinline__ void wave_add(double v, double* __restrict__ dst) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v != 0.0) atomicAdd(dst, v);
}

// One level of a wide view (rt_device.hpp DWide): nodes first .. first + count - 1. area (nullable): += the summed
// surface area of the nodes' decoded child boxes.
__global__ __launch_bounds__(64) void k_wide_level(int first, int count, float4* __restrict__ nodes,
                                                   const int* __restrict__ orig, const float* __restrict__ coords,
                                                   float4* __restrict__ exact, float inflate, double* __restrict__ area) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double A = 0.0;
    if (i < count) {
        const int k = first + i;
        uint32_t W[20];
        load_words(nodes, k, W);
        rtq::Box box[rtq::WIDTH];
        rtq::Box own = rtq::empty_box();
        for (int s = 0; s < rtq::WIDTH; s++) {
            if (!rtq::occupied(W, s)) continue;
            if ((rtq::imask_of(W) >> s) & 1u) {
                const size_t c = rtq::child_of(W, s);
                const float4 lo = exact[2 * c], hi = exact[2 * c + 1];
                box[s] = rtq::Box{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
            } else {
                const uint32_t m = rtq::meta_of(W, s), cnt = m >> 5, off = m & 31u;
                box[s] = rtq::empty_box();
                for (uint32_t j = 0; j < cnt; j++) {
                    const float* p = coords + 9 * (size_t)orig[W[5] + off + j];
                    rtq::grow(box[s], p);
                    rtq::grow(box[s], p + 3);
                    rtq::grow(box[s], p + 6);
                }
            }
            rtq::grow(own, box[s]);
        }
        exact[2 * (size_t)k] = make_float4(own.lo[0], own.lo[1], own.lo[2], 0.0f);
        exact[2 * (size_t)k + 1] = make_float4(own.hi[0], own.hi[1], own.hi[2], 0.0f);
        (void)rtq::requantise(W, box, inflate);  // (never false: rt_update_vertices refuses coordinates beyond RT_COORD_MAX)
        // (the topology words are written back as read)
        for (int j = 0; j < 5; j++)
            nodes[5 * (size_t)k + j] = make_float4(__int_as_float((int)W[4 * j]), __int_as_float((int)W[4 * j + 1]),
                                                   __int_as_float((int)W[4 * j + 2]), __int_as_float((int)W[4 * j + 3]));
        if (area) A = rtq::decoded_area(W);
    }
    if (area) wave_add(A, area);
}

// area += the summed surface area of every node's decoded child boxes (the view as it stands)
__global__ __launch_bounds__(256) void k_wide_area(const float4* __restrict__ nodes, int n, double* __restrict__ area) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    double A = 0.0;
    if (k < n) {
        uint32_t W[20];
        load_words(nodes, k, W);
        A = rtq::decoded_area(W);
    }
    wave_add(A, area);
}

}  // namespace rtr
