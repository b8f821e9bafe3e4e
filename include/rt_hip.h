/*
 * rt_hip.h — C-ABI of librt_hip.so, the device half of the drop-in (HIP, gfx950 / MI355X).
 *
 * It replaces the reference's render seam:
 *   GPU  gpu/include/gpu.cuh:23-26   void load_to_gpu(void); float render_frame(bool,int,int);
 *                                     void load_from_gpu(void);
 *   CPU  cpu/src/main.c:214-264       void render_frame(void) over the globals cam, triangles,
 *                                     lights, amb_light, bvh, tri_idx -> vec_t pixels[W*H]
 * with explicit, reentrant calls: state lives in an rt_ctx (one per device), inputs are the
 * reference's own data (triangle_t / bvh_t / light_t layouts, rt_types.h), every call returns an
 * int status (0 = ok, < 0 = RT_E_*), nothing calls exit(). A context is not thread-safe; distinct
 * contexts may be driven from distinct host threads.
 *
 * The per-pixel hot path (ray generation, BVH traversal, ray-triangle intersection, Lambert/Blinn
 * shading with shadow rays, the BOUNCES reflection loop, clamp) runs in ONE HIP kernel per frame
 * (or per batch of frames, rt_render_frames). Every launch configuration is chosen through the
 * arguments below (rt_frame.variant / waves_cap / dealing / regroup / hot_pct); the library reads no
 * environment variable on the render path except two diagnostics (PRT_TILE_TRACE, PRT_TUNE_LOG).
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

/* rt_opts.flags */
enum {
    RT_FLAG_COUNTERS = 1,       /* also count traversal work (node visits, triangle tests): slower */
    /* The kernels' packed builds have field bounds: 5-byte stack entries hold a 24-bit child base (at most 2^24 wide
     * nodes per view), packed triangle-test jobs a 26-bit triangle index (fewer than 2^26 triangles). Scenes past them
     * run the unpacked builds. These two flags select those builds for any scene, so that they can be checked on
     * scenes of test size (tests/test_gpu_unpacked.py). The result is bit-identical either way. */
    RT_FLAG_UNPACKED_STACK = 2, /* as for a scene of more than 2^24 wide nodes: no packed stack entries (no pool
                                   kernels, PERSIST4 with two-word entries) */
    RT_FLAG_UNPACKED_TRIS = 4,  /* as for a scene of 2^26 or more triangles: no packed triangle tests */
    /* The pool kernels hand their shadow rays out from a per-wave job list in LDS where it fits 4 workgroups per CU,
     * and with a cursor where it does not (many lights, 5-8 bounces, deep trees). This flag selects the cursor for any
     * scene, so that it can be checked on scenes of test size (tests/test_gpu_pool_handout.py). Same bits, same walks. */
    RT_FLAG_POOL_CURSOR = 8     /* as for a launch whose LDS has no room for the job lists */
};

typedef struct rt_opts {
    int device;      /* HIP device ordinal */
    unsigned flags;  /* RT_FLAG_* */
    void* stream;    /* hipStream_t to launch on; NULL = the context creates its own */
} rt_opts;

/* Scene = the globals load_to_gpu() reads (gpu/src/gpu.cu:16-29, 129-201). Deep-copied by
 * rt_upload_scene; the caller keeps ownership. bvh/tri_idx are bvh_build()'s output
 * (cpu/src/bvh.c:360-388) for ANY builder that keeps the reference layout. */
typedef struct rt_scene {
    const rt_triangle* triangles;
    int n_triangles;
    const rt_bvh_node* bvh;
    int n_nodes;
    const int* tri_idx;
    const rt_light* lights;
    int n_lights;
    rt_vec3 amb; /* amb_light (cpu/src/main.c:37): 0.5, 0.5, 0.5 */
    int accel;   /* RT_ACCEL_*: acceleration structure of the fast kernel */
    int ploc_radius; /* RT_ACCEL_GPU / AUTO: the GPU build's nearest-neighbour radius (0 = 32, at most 64) */
    float collapse_node_cost; /* the 8-wide collapse's price of a wide-node visit in triangle tests (0 = 2) */
} rt_scene;

/* rt_scene.accel */
enum {
    RT_ACCEL_AUTO = 0,      /* the library builds the fast walk's BVH: RT_ACCEL_GPU, falling back to RT_ACCEL_HOST;
                               `bvh` serves the strict walk */
    RT_ACCEL_REFERENCE = 1, /* traverse the given `bvh` in both walks */
    RT_ACCEL_GPU = 2,       /* build the fast walk's BVH on the GPU (PLOC over Morton-sorted triangles, rt_build.hpp),
                               then collapse it to the 8-wide quantised layout; falls back to RT_ACCEL_HOST when the
                               tree is too deep for the wide walk (rt_scene_info.accel_built says which) */
    RT_ACCEL_HOST = 3       /* build it on the host: binned SAH (librt_host.so), then the same collapse */
};

/* what rt_upload_scene built (rt_get_scene_info) */
typedef struct rt_scene_info {
    int n_triangles, n_lights;
    int wide_nodes, wide_depth; /* the fast walk's 8-wide BVH (0: none, the binary fast walk) */
    int accel_built;            /* RT_ACCEL_* of the fast walk's BVH as built (RT_ACCEL_HOST = host binned SAH, RT_ACCEL_GPU = PLOC on the device) */
    float build_ms;             /* host wall time of the acceleration build (binary tree + wide collapse) */
    float gpu_build_ms;         /* of which the GPU tree build (RT_ACCEL_GPU; incl. transfers) */
    int unit_triangles;         /* triangles a unit-length ray can hit (|e1 x e2| >= EPSILON: hit_triangle's det cull,
                                   cpu/src/raytracer.c:41-45), indexed by the view reflection and shadow rays walk;
                                   0: that view is the full one */
    int unit_nodes, unit_depth; /* its 8-wide BVH */
    int primary_triangles;      /* triangles a direction of length <= 3 can hit, indexed by the view primary rays walk
                                   when every primary direction of a launch is that short (the reference camera's are
                                   1.87-2.77); 0: no such view (it would leave out < 2 % of the triangles) */
    int primary_nodes;
    /* build_ms by stage, summed over the views: */
    float ploc_ms;     /* the GPU tree builds (PLOC, incl. transfers) */
    float treelet_ms;  /* the treelet restructuring of the GPU-built trees (host threads, rt_treelet.hpp) */
    float collapse_ms; /* the layout and the 8-wide collapse with its quantisation (host threads, rt_wide.cpp) */
} rt_scene_info;

/* rt_frame.kernel */
enum {
    RT_KERNEL_AUTO = 0,   /* RT_KERNEL_FAST */
    RT_KERNEL_STRICT = 1, /* reference-order traversal, exact slab divisions: bit-exact by construction */
    RT_KERNEL_FAST = 2    /* the fast walk (8-wide quantised BVH) in the launch configuration rt_frame.variant
                             names; every variant renders the same bits as RT_KERNEL_STRICT */
};

/* rt_frame.variant: launch configuration of RT_KERNEL_FAST */
enum {
    RT_VARIANT_DEFAULT = 0,  /* the library's rule, measured per frame shape: frame batches and spp > 1 try
                                RT_VARIANT_PERSIST4 and the pool kernel -- RT_VARIANT_SHDEFER where its LDS path buffer
                                fits, else RT_VARIANT_SHPOOL -- three times each on their first launches and keep the
                                faster, by the minimum of each candidate's trials, or by their medians when a
                                candidate's median exceeds 50 ms (RT_VARIANT_PERSIST4 alone where no pool fits); single 1-spp frames
                                run RT_VARIANT_HYBRID (RT_VARIANT_PERSIST where it cannot run); rt_get_launch_info */
    RT_VARIANT_PERSIST = 1,  /* k_persist: one lane per pixel path, walks in lockstep, 3 waves per SIMD */
    RT_VARIANT_PERSIST4 = 2, /* k_persist at 4 waves per SIMD (path levels in LDS) */
    /* 3: the split pipeline (closest chains / shadow batches / resolve), measured slower, removed in round 4: refused */
    RT_VARIANT_COOP2 = 4,    /* k_coop: 2 lanes per ray (shorter chains for small row sets) */
    RT_VARIANT_COOP4 = 5,    /* k_coop: 4 lanes per ray */
    /* 6: k_coop with 8 lanes per ray, 3x slower, removed in round 4: refused */
    /* 7: k_fan (1 + lights lanes per pixel, shadow fan-out), never chosen by a rule nor won a trial, removed in
       round 5: refused */
    /* 8, 9: k_chain (each lane's walks back to back), measured slower and removed in round 2: refused */
    /* 10: k_pool (tile-local LDS ray queues behind workgroup barriers), measured slower, removed in round 4: refused */
    RT_VARIANT_HYBRID = 11,  /* single 1-spp frames: the tiles a measuring frame of the same SHAPE found costliest through
                                k_coop (2 or 4 lanes per ray) on a second stream while k_persist or the shadow pool renders
                                the rest. The first frame of a shape measures (k_persist with per-tile times), the next
                                ones try the candidates -- including the whole-frame kernels -- four frames each, back
                                to back, and the best median of the last three renders from then on, each frame's tile lists built on the device from the
                                previous frame's per-tile times (RT_BUILD_FEEDBACK: a moving camera's lists stay one
                                frame old). Nothing waits on the host: measurements and trials are read by event queries
                                (rt_frame.hot_pct > 0: that threshold and rt_frame.hot_kernel, no trials) */
    /* 12: k_relay (1 + lights waves per tile, LDS hand-off), measured slower, removed in round 4: refused */
    RT_VARIANT_SHPOOL = 13,  /* k_persist at 4 waves per SIMD with each bounce level's shadow rays (every pixel's, every
                                light's) walked as ONE per-wave pool: a lane whose walk ends takes the next unassigned ray,
                                lanes of ended paths included (rt_frame.regroup = idle lanes per refill; 1..32 lights; the
                                LDS path buffer must fit 4 workgroups per CU, else RT_VARIANT_PERSIST4 runs) */
    /* 14: k_stream (a lane whose path ends takes its tile's next pixel; paths at mixed levels), measured slower in
       round 4 (dragon 0.781 vs 0.654 ms per frame in 20-frame batches) and removed: refused */
    RT_VARIANT_SHDEFER = 15  /* RT_VARIANT_SHPOOL with ONE pool for all bounce levels: a wave's paths find their closest
                                hits level by level first, then the shadow rays of every level, pixel and light are walked
                                as one pool and the levels are shaded after it (RT_VARIANT_PERSIST4 where the larger LDS
                                path buffer does not fit) */
};

/* rt_frame.hot_kernel: the kernel RT_VARIANT_HYBRID sends the hot tiles to when rt_frame.hot_pct > 0 */
enum {
    RT_HOT_COOP4 = 0, /* k_coop, 4 lanes per ray */
    RT_HOT_COOP2 = 1  /* k_coop, 2 lanes per ray */
    /* 2: k_fan, removed in round 5; 3: k_relay, removed in round 4: refused */
};

/* rt_frame.dealing: order in which persistent waves take their tiles (k_persist 8x8, k_pool 16x16) */
enum {
    RT_DEAL_DEFAULT = 0,  /* XCD-aware: 4 x 2 regions for batches of full frames, 8 row bands otherwise */
    RT_DEAL_GLOBAL = 1,   /* one counter over the centre-out order */
    RT_DEAL_ROWS = 2,     /* 8 bands of tile rows, band r drained first by the workgroups of XCD r */
    RT_DEAL_COLUMNS = 3,  /* 8 bands of tile columns */
    RT_DEAL_BLOCKS = 4,   /* 4 x 2 blocks */
    RT_DEAL_ROW_MAJOR = 5 /* one counter, row-major tile order */
};

/* Rows rendered: y = row_offset + (k / B) * row_stride + k % B for k in [0, n_rows), B = max(1, row_block)
 * (B = 1: y = row_offset + k * row_stride). Output rows are compact: row k of the output holds image
 * row y. A full frame is {W, H, 0, 1, H, ...}. Rank q of N, cyclic rows: {.., q, N, ..}; block-cyclic
 * rows (blocks of B rows dealt cyclically, so a rank's 8x8 pixel tiles stay 8x8 in the image):
 * {.., q * B, N * B, .., row_block = B}. */
typedef struct rt_frame {
    int width, height;
    int row_offset, row_stride, n_rows;
    int bounces; /* BOUNCES (cpu/include/options.h:52), 1..8; the reference uses 4 */
    int spp;     /* 1 = the reference's pixel-corner ray; s*s = s x s stratified grid, mean of clamped samples */
    int kernel;  /* RT_KERNEL_* */
    int row_block; /* 0 or 1: single rows; B > 1: rows in blocks of B (row_stride >= B) */
    int frame_shift; /* 0: every frame of a batch renders the rows above. S > 0 (RT_KERNEL_FAST only): frame f
                      * of rt_render_frames starts at (row_offset + f * S) % row_stride, so that ranks dealt
                      * block-cyclic rows rotate through every block residue over a batch and their costs
                      * even out; compact rows whose image row falls at or past height are skipped. */
    /* launch configuration (RT_KERNEL_FAST; all zero = the library's defaults) */
    int variant;   /* RT_VARIANT_* */
    int tune;      /* 0 or 1, both the default rule (which measures its candidates itself). Until round 4, 1 selected
                      a separate autotuner whose candidates left out the hybrid launch; it was slower than the default
                      rule on every BASELINE scene and was removed. Other values are refused. */
    int waves_cap; /* persistent grids: at most this many workgroups (4 waves each) per CU; 0 = occupancy limit */
    int dealing;   /* RT_DEAL_* */
    int regroup;   /* RT_VARIANT_SHPOOL: idle lanes of a wave that trigger a refill from the pool; 0 = 16 */
    int hot_pct;   /* RT_VARIANT_HYBRID: tiles whose measured time exceeds hot_pct % of the costliest tile's go to the
                      kernel hot_kernel names; 0 = try several thresholds and hot kernels and keep the fastest */
    int hot_kernel; /* RT_HOT_* (with hot_pct > 0) */
} rt_frame;

/* Device output pointers (all nullable). rgb: [n_rows][width][3] f32 in [0,1] = vec_t pixels
 * (main.c:39); NULL -> a buffer owned by the context (read it with rt_download).
 * hit: [n_rows][width] int32 primary closest-hit triangle index (-1 = miss); t: its distance.
 * bounce_hit: [n_rows][width][bounces] int32 closest-hit triangle index of every recursion level
 * (raytrace(.., iter), raytracer.c:101-135): -1 = miss, -2 = level not reached (first sample when spp > 1).
 * bgra: [n_rows][width] uint32, the pixel quantised as the BMP writer does (vec_to_bgra,
 * cpu/src/bmp_writer.c:88-95: B | G << 8 | R << 16 | 255 << 24, little-endian bytes B,G,R,A) in the frame's
 * top-down row order (the BMP file stores rows bottom-up); written by the kernel itself, so a frame bound for
 * a gather or a file moves 4 bytes per pixel instead of 12. With bgra set and rgb NULL no f32 pixels are
 * written (rt_download of rgb, rt_gather and rt_download_bmp then refuse the frame). */
typedef struct rt_outputs {
    float* rgb;
    int* hit;
    float* t;
    int* bounce_hit;
    unsigned int* bgra;
} rt_outputs;

typedef struct rt_stats {
    unsigned long long primary;        /* primary rays                                     */
    unsigned long long reflection;     /* traced reflection rays                           */
    unsigned long long shadow;         /* traced shadow rays (past the back-face test)     */
    unsigned long long shadow_skipped; /* light_v early-outs (raytracer.c:66-67)           */
    unsigned long long hits;           /* closest-hit rays that hit a triangle             */
    unsigned long long ch_inner, ch_leaf, ch_tri; /* closest-hit interior visits / leaf visits / tri tests (RT_FLAG_COUNTERS) */
    unsigned long long sh_inner, sh_leaf, sh_tri; /* same for shadow rays (RT_FLAG_COUNTERS)             */
    unsigned long long pixels;         /* pixels written                                    */
    unsigned long long fallbacks;      /* fast-kernel rays re-walked strictly (zero direction component or exact tie) */
    unsigned long long stack_overflows; /* must be 0 (rt_get_stats fails otherwise)          */
    unsigned long long node_bytes;     /* BVH node / leaf record bytes read (RT_FLAG_COUNTERS; fused kernels) */
    unsigned long long wave_steps;     /* wave-level wide-node steps (RT_FLAG_COUNTERS): SIMD efficiency =
                                          (ch_inner + sh_inner of the wide walk) / (64 * wave_steps) */
    unsigned long long shadow_wave_steps; /* of which shadow walks' (k_persist's walks; RT_FLAG_COUNTERS)     */
    unsigned long long steps_lanes_16, steps_lanes_32, steps_lanes_48, steps_lanes_64; /* k_persist's wave steps
                                          with 1-16 / 17-32 / 33-48 / 49-64 active lanes (RT_FLAG_COUNTERS)  */
    unsigned long long steps_hist[2][4][4]; /* k_persist's wave steps by walk kind (0 closest: primary + reflection,
                                          1 shadow) x bounce level (0, 1, 2, 3 and deeper) x active lanes (1-16,
                                          17-32, 33-48, 49-64) (RT_FLAG_COUNTERS)                               */
} rt_stats;

int rt_device_count(void);
const char* rt_version(void);

int rt_create(const rt_opts* opts, rt_ctx** out);
/* The largest |coordinate| of a scene, at an upload and at every update: 2^123 (1.06e37). A wide view's planes lie on a
 * per-node grid whose origin is 1,024 steps below the node's boxes (rt_quant.hpp); up to here that origin, the step
 * 2^e (e <= 117) and every decoded plane are finite floats, beyond it they need not be. rt_upload_scene and
 * rt_update_vertices (rt_rebuild_views with it) answer RT_E_ARG for a larger coordinate and change nothing; the host
 * builders (rth_wbvh_build, rth_wbvh_build_greedy, rth_wbvh_refit) answer RT_E_ARG where a grid does not fit. */
#define RT_COORD_MAX 0x1p123f
/* load_to_gpu(): converts the reference layouts into the device layout and uploads. Where the fast view's
 * collapse fails or its product does not pass rth_wbvh_check, the scene has no wide view (rt_scene_info.wide_nodes = 0)
 * and the fast kernels answer from the other trees or the exhaustive loops: never from a view that misses triangles. */
int rt_upload_scene(rt_ctx* ctx, const rt_scene* scene);
int rt_get_scene_info(rt_ctx* ctx, rt_scene_info* info);
/* render_frame(): enqueues ONE kernel on the context stream (asynchronous) */
int rt_render(rt_ctx* ctx, const rt_camera* cam, const rt_frame* frame, const rt_outputs* out);
/* A batch of n_frames frames of the same shape (a camera sequence; main.c:141-160's ITERATIONS loop when
 * the cameras are equal): frame i uses cams[i] and writes its outputs at frame offset i, i.e. rgb
 * [n_frames][n_rows][width][3], hit / t [n_frames][n_rows][width], bounce_hit [n_frames][n_rows][width]
 * [bounces]. RT_KERNEL_FAST traces the whole batch in ONE persistent launch whose tile dealing interleaves
 * the frames (the long reflection chains of every frame start first, so one frame's tail overlaps the
 * others' work); other kernels launch once per frame. Each frame equals its rt_render bit for bit; the
 * stats of the call are the batch's sums. rt_gather / rt_download_bmp need a single-frame render. */
int rt_render_frames(rt_ctx* ctx, const rt_camera* cams, int n_frames, const rt_frame* frame,
                     const rt_outputs* out);
/* What the last rt_render / rt_render_frames ran (no synchronisation): the default rule resolves RT_VARIANT_DEFAULT per
 * shape, trying candidates on the first frames of a shape. A caller timing the drop-in seam skips frames until
 * `settled` (the reference's own loop needs no such thing: every frame is bit-exact either way). */
typedef struct rt_launch_info {
    int variant;      /* RT_VARIANT_* the last render ran (0 for RT_KERNEL_STRICT) */
    int hot_pct;      /* RT_VARIANT_HYBRID with hot tiles: the threshold, else 0 */
    int hot_lanes;    /* its lanes per ray (k_coop) or per pixel (k_fan) */
    int cold_variant; /* its kernel of the cold tiles (RT_VARIANT_PERSIST or RT_VARIANT_SHPOOL) */
    int trial;        /* 1: a measuring or trial frame of the default rule */
    int settled;      /* 1: the configuration of this shape is decided: no trial frames follow */
    int refresh;      /* 1: a decided hybrid shape's measuring frame that renews its tile lists (k_persist with per-tile
                         times; settled = 1) -- only where the per-frame feedback is off (PRT_FEEDBACK=0 at build time:
                         a measuring frame every 64 frames of a shape); 0 with it */
    unsigned build;   /* the k_persist instantiation that ran (of the cold tiles, for a hybrid launch): RT_BUILD_* bits;
                         0 for the other kernels (strict, k_coop alone) */
} rt_launch_info;
/* rt_launch_info.build */
enum {
    RT_BUILD_WAVES4 = 1,       /* 4 waves per SIMD (<= 128 VGPRs); else 3 */
    RT_BUILD_PACKED_STACK = 2, /* 5-byte wide-stack entries */
    RT_BUILD_PACKED_TRIS = 4,  /* packed triangle tests through the wave's LDS queue */
    RT_BUILD_LDS_PATHS = 8,    /* the path levels in LDS (else a global slab, or registers at 3 waves) */
    RT_BUILD_POOL_LEVEL = 16,  /* the per-level shadow pool (RT_VARIANT_SHPOOL) */
    RT_BUILD_POOL_ALL = 32,    /* one shadow pool for all levels (RT_VARIANT_SHDEFER) */
    RT_BUILD_TRACE = 64,       /* the measuring build with per-tile times */
    RT_BUILD_FEEDBACK = 128,   /* a decided single-frame shape's frame dealt by the previous frame's per-tile times, its
                                  tile lists built on the device (no measuring frames, no host round trip) */
    RT_BUILD_POOL_LIST = 256   /* a pool kernel handing its rays out from the per-wave job list (else its cursor) */
};
int rt_get_launch_info(rt_ctx* ctx, rt_launch_info* info);

/* Ray queries: the reference's two traversals for the caller's own rays (device arrays), on the uploaded scene.
 *   RT_QUERY_CLOSEST   (hit, t) = what bvh_traverse(0, &o, &d, &nd, &t, &index) leaves in index and t on the scene's
 *                      reference BVH (cpu/src/bvh.c:317-358), the first-found rule at exact ties included; hit is the
 *                      original triangle index
 *   RT_QUERY_OCCLUDED  occluded = !bvh_light_traverse(0, &o, &d, &t, max_dist2) (bvh.c:269-315; no back-face
 *                      early-out: that is light_v's and needs a normal)
 * RT_KERNEL_FAST answers with the same bits as RT_KERNEL_STRICT: a ray the fast walks' assumptions do not cover
 * (checked per ray: the direction's length for the view, its magnitude, the origin's distance from the scene, unit
 * length and a finite positive max_dist2 for the occlusion walk, non-finite input, an all-zero direction; DESIGN.md
 * §3k) walks the reference tree; whatever that walk returns is the answer, and no input is an error.
 * A query touches nothing a render call owns: rt_download, rt_download_bmp, rt_gather, rt_get_stats,
 * rt_get_launch_info, rt_kernel_times, rt_sync's kernel_ms and the default rule's per-shape state are what they were. */
enum { RT_QUERY_CLOSEST = 0, RT_QUERY_OCCLUDED = 1 };
typedef struct rt_rays {
    const float* origin;    /* device, [n][3] f32 */
    const float* dir;       /* device, [n][3] f32, NOT normalised by the library */
    const float* max_dist2; /* device, [n] f32; RT_QUERY_OCCLUDED only (light_dist2 of bvh_light_traverse) */
    int n;                  /* >= 0; 0 is RT_OK and launches nothing */
    int kind;               /* RT_QUERY_* */
    int kernel;             /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
    int regroup;            /* RT_QUERY_OCCLUDED with RT_KERNEL_FAST (its pool kernel): idle lanes of a wave that trigger
                               a refill, 1..63; 0 = the library's default (16); 64 = the lockstep kernel instead. Same
                               bits either way. RT_QUERY_CLOSEST has the lockstep kernel only: 0..64
                               accepted, no effect */
} rt_rays;
typedef struct rt_ray_results { /* device pointers */
    int* hit;      /* CLOSEST: [n] original triangle index, -1 = miss (nullable) */
    float* t;      /* CLOSEST: [n] ray parameter, exactly what rt_outputs.t holds for a primary ray (FLT_MAX on a
                      miss) (nullable; not both) */
    int* occluded; /* OCCLUDED: [n] 1 = blocked, 0 = clear */
} rt_ray_results;
/* asynchronous on the context stream; elements at index n and beyond are not written */
int rt_trace_rays(rt_ctx* ctx, const rt_rays* rays, const rt_ray_results* out);
typedef struct rt_query_info {
    long long rays, hits;                       /* hits: CLOSEST rays that hit / OCCLUDED rays blocked */
    long long unit_rays, short_rays, full_rays; /* rays the fast walk served from the unit / primary / full view */
    long long strict_rays;     /* RT_KERNEL_FAST: rays outside the fast walk's domain, walked on the reference tree from
                                  the start (RT_KERNEL_STRICT: 0, it has no such domain) */
    long long tie_rewalks;     /* fast walks re-walked for an exact tie or a failed reference-path check */
    long long stack_overflows; /* must be 0 */
    float kernel_ms;           /* HIP events around the query's launch */
} rt_query_info;
/* counters of the last query (synchronises); RT_E_KERNEL when it overflowed a traversal stack (its results are not
 * valid), RT_E_STATE before the first query */
int rt_get_query_info(rt_ctx* ctx, rt_query_info* info);

/* Radiance queries: the reference's raytrace() (cpu/src/raytracer.c:101-177) for the caller's own rays -- Lambert/Blinn
 * shading with one shadow ray per light, the reflection chain of `bounces` levels, folded deepest level first -- so a
 * ray no pinhole camera on a pixel grid expresses (a panorama, an orthographic view, jittered samples, a probe) gets
 * the colour, bit for bit, that a frame's pixel with that primary ray would get. RT_KERNEL_FAST answers with the same
 * bits as RT_KERNEL_STRICT: the caller's ray is tested as rt_trace_rays tests it, and a path whose first ray is outside
 * the fast walks' domain walks the reference tree at every level. No ray value is an error.
 * A shade query touches nothing a render call owns (as rt_trace_rays) and leaves rt_get_query_info's answer alone. */
typedef struct rt_shade {
    const float* origin;   /* device, [n][3] f32 */
    const float* dir;      /* device, [n][3] f32, NOT normalised by the library */
    int n;                 /* >= 0; 0 is RT_OK and launches nothing */
    int bounces;           /* 1..8, as rt_frame.bounces */
    int kernel;            /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
    int regroup;           /* fast kernel's shadow-pool form: 1..63 idle lanes per refill; 0 = library default;
                              64 = the lockstep form. Same bits either way. */
    int unclamped;         /* 0: rgb = vec_constrain(raytrace(o, d, 0), 0, 1), a frame's pixel;
                              1: raytrace()'s return value as is (rgb only; refused together with bgra) */
} rt_shade;
typedef struct rt_shade_results {   /* device pointers, all nullable, at least one non-null when n > 0 */
    float* rgb;            /* [n][3] */
    unsigned int* bgra;    /* [n], vec_to_bgra's quantisation as rt_outputs.bgra */
    int* hit; float* t;    /* [n] the level-0 closest hit, exactly rt_trace_rays' CLOSEST answer */
    int* bounce_hit;       /* [n][bounces], -1 miss, -2 level not reached, as rt_outputs.bounce_hit */
} rt_shade_results;
/* asynchronous on the context stream; elements at index n and beyond are not written */
int rt_shade_rays(rt_ctx* ctx, const rt_shade* rays, const rt_shade_results* out);
typedef struct rt_shade_info {
    long long rays, hits, reflection, shadow, shadow_skipped; /* rt_stats' primary / hits / reflection / shadow /
                                  shadow_skipped, for this query: rays = the caller's (level-0) rays */
    long long strict_paths;    /* fast kernel: paths whose level-0 ray is outside the fast walks' domain */
    long long tie_rewalks;     /* fast walks re-walked on the reference tree (an exact tie, a failed reference-path
                                  check, a degenerate ray on a box face), at any level */
    long long stack_overflows; /* must be 0 */
    float kernel_ms;           /* HIP events around the query's launch */
} rt_shade_info;
/* counters of the last shade query (synchronises); RT_E_KERNEL when it overflowed a traversal stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_shade_info(rt_ctx* ctx, rt_shade_info* info);

/* Multi-hit queries: the k nearest hits and the hit count of the caller's own rays -- what lies behind the first
 * surface (transmission, thickness, later lidar returns, point-in-mesh parity, closest hits limited to a segment).
 * For ray i the hit set is
 *   S_i = { j : hit_triangle(o, d, triangles[j]) = t_j < FLT_MAX and t_j <= t_max[i] }
 * (hit_triangle: cpu/src/raytracer.c:35-59 with its |det| < EPSILON and t > EPSILON culls), ordered by (t ascending,
 * original triangle index ascending): a total order, so the answer depends on no BVH. It is what the reference's
 * brute-force path sees (USE_BVH 0, raytracer.c:115-129), not what bvh_traverse sees: for a direction with a zero
 * component from an origin on a box face the reference's BVH walk misses geometry that brute force finds (DESIGN.md §2
 * item 2); here it is found.
 * tri[i][0..max_hits) and t[i][0..max_hits) receive the first max_hits entries of S_i (unused slots: -1 / FLT_MAX);
 * count[i] = min(|S_i|, max_hits), or |S_i| itself with count_all (the walk then prunes at t_max only). max_hits = 0
 * with count_all is a pure counting query. t_max NULL or t_max[i] = +inf: no bound; a NaN or non-positive t_max[i]: the
 * empty set. No ray value is an error.
 * RT_KERNEL_STRICT tests every ray against every triangle (the checker: rays x triangles tests, as slow as that
 * sounds); RT_KERNEL_FAST walks the wide views and answers with the same bits.
 * A hits query touches nothing a render, a ray query or a shade query owns. */
#define RT_HITS_MAX 16
typedef struct rt_hits {
    const float* origin;   /* device, [n][3] f32 */
    const float* dir;      /* device, [n][3] f32, NOT normalised by the library */
    const float* t_max;    /* device, [n] f32, nullable */
    int n;                 /* >= 0; 0 is RT_OK and launches nothing */
    int max_hits;          /* 0..RT_HITS_MAX */
    int count_all;         /* 0 / 1 */
    int kernel;            /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_hits;
typedef struct rt_hit_results { /* device pointers: [n][max_hits], [n][max_hits], [n] */
    int* tri;     /* nullable (with max_hits > 0 not both tri and t) */
    float* t;     /* nullable */
    int* count;   /* nullable, except for max_hits = 0 */
} rt_hit_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, null origin / dir with n > 0, max_hits outside 0..RT_HITS_MAX, max_hits > 0 with tri and
 * t both NULL, max_hits = 0 without count_all and a count pointer, count_all not 0 / 1, an unknown kernel. */
int rt_trace_hits(rt_ctx* ctx, const rt_hits* rays, const rt_hit_results* out);
typedef struct rt_hits_info {
    long long rays, rays_hit;                   /* rays_hit: rays with a non-empty S_i */
    long long hits_stored, hits_counted;        /* sums of min(|S_i|, max_hits) and of count[i] */
    long long unit_rays, short_rays, full_rays; /* rays the fast walk served from the unit / primary / full view */
    long long exhaustive_rays;  /* rays tested against every triangle: all with a valid bound under RT_KERNEL_STRICT,
                                   those outside the fast walk's domain under RT_KERNEL_FAST (a ray whose t_max makes
                                   S_i empty walks nothing and is in none of the four) */
    long long stack_overflows;  /* must be 0 */
    float kernel_ms;            /* HIP events around the query's launch */
} rt_hits_info;
/* counters of the last hits query (synchronises); RT_E_KERNEL when it overflowed a traversal stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_hits_info(rt_ctx* ctx, rt_hits_info* info);

/* Nearest-surface queries: per caller-supplied point the nearest triangle, the closest point on it and the squared
 * distance (distance fields, clearance tests, snapping samples to a surface, closest-point correspondences).
 * Query i is a point q with an optional bound max_dist2[i]. Its candidate set is
 *   S_i = { j : D(q, triangle j) <= min(max_dist2[i], FLT_MAX) }, ordered by (D ascending, original index ascending),
 * and the answer is its first element: a total order, so the answer depends on no BVH, and triangles that share the
 * nearest vertex or edge (an exact tie, common on ordinary meshes) answer with the lowest index.
 * D and the closest point P are defined on a triangle's record a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0) by Ericson's
 * region algorithm (Real-Time Collision Detection 5.1.5), every operation one float32 operation, dot(u, v) evaluated as
 * u.x*v.x + u.y*v.y + u.z*v.z left to right, nothing contracted into an FMA:
 *   ap = q - a;   d1 = dot(e1, ap);  d2 = dot(e2, ap)
 *   bp = ap - e1; d3 = dot(e1, bp);  d4 = dot(e2, bp)
 *   cp = ap - e2; d5 = dot(e1, cp);  d6 = dot(e2, cp)
 *   vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4
 *   the first condition that holds, in this order:
 *     d1 <= 0 && d2 <= 0                   p = a
 *     d3 >= 0 && d4 <= d3                  p = a + e1
 *     vc <= 0 && d1 >= 0 && d3 <= 0        p = a + e1 * (d1 / (d1 - d3))
 *     d6 >= 0 && d5 <= d6                  p = a + e2
 *     vb <= 0 && d2 >= 0 && d6 <= 0        p = a + e2 * (d2 / (d2 - d6))
 *     va <= 0 && x >= 0 && y >= 0          p = (a + e1) + (e2 - e1) * (x / (x + y)),  x = d4 - d3, y = d5 - d6
 *     otherwise  den = 1 / ((va + vb) + vc); p = (a + e1 * (vb * den)) + e2 * (vc * den)
 *   lo = fminf(fminf(a, a + e1), a + e2); hi = fmaxf(fmaxf(a, a + e1), a + e2)     per component
 *   P = fminf(fmaxf(p, lo), hi)                                  per component, C semantics: a NaN operand loses
 *   df = q - P;  D = dot(df, df)
 * The clamp into the triangle's own box is part of the definition: P is finite for every finite triangle (a degenerate
 * triangle's 0 / 0 becomes a corner of its box -- such a P need not lie on the triangle), and the walk prunes with no
 * tuned margin. P at the second or third vertex is fl(a + e1) or fl(a + e2): the vertex itself or a
 * neighbouring float.
 * Results: tri[i] = the original triangle index, d2[i] = D, point[i] = P. The empty set gives -1, FLT_MAX and q's own
 * bits; it is empty when nothing lies within the bound, when max_dist2[i] is NaN or negative (0 is a valid bound: points
 * on the surface), and for a non-finite q (decided before any walk). max_dist2 NULL or +inf: no bound. A finite q so
 * far away that D overflows has the empty set. No input value is an error.
 * RT_KERNEL_STRICT tests every point against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * boxes ordered and pruned by their distance to the point, and answers with the same bits; a scene without a wide view
 * (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
 * A nearest query touches nothing a render, a ray query, a shade query or a hits query owns. */
typedef struct rt_points {
    const float* point;     /* device, [n][3] f32 */
    const float* max_dist2; /* device, [n] f32, nullable */
    int n;                  /* >= 0; 0 is RT_OK and launches nothing */
    int kernel;             /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_points;
typedef struct rt_nearest_results { /* device pointers, all nullable, at least one non-null when n > 0 */
    int* tri;     /* [n] */
    float* d2;    /* [n] */
    float* point; /* [n][3] */
} rt_nearest_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, a null point with n > 0, all three outputs NULL with n > 0, an unknown kernel. */
int rt_nearest_points(rt_ctx* ctx, const rt_points* points, const rt_nearest_results* out);
typedef struct rt_nearest_info {
    long long points, found;      /* found: points with a non-empty S_i */
    long long walked_points;      /* points that walked the wide view */
    long long exhaustive_points;  /* points tested against every triangle: all valid ones under RT_KERNEL_STRICT or
                                     without a wide view (a non-finite point or a NaN / negative bound is in neither) */
    long long empty_points;       /* points - found */
    long long nodes_visited;      /* wide nodes decoded, summed over the points (a level popped again counts again) */
    long long tris_tested;        /* triangle tests, summed over the points (exhaustive: points x triangles) */
    long long stack_overflows;    /* must be 0 */
    float kernel_ms;              /* HIP events around the query's launch */
} rt_nearest_info;
/* counters of the last nearest query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_nearest_info(rt_ctx* ctx, rt_nearest_info* info);

/* Neighbour queries: per caller-supplied point the k nearest triangles and the number of triangles within a radius --
 * rt_nearest_points' plural form (contacts of a particle against every triangle within its radius, several candidates
 * of a correspondence search, blending over the nearest few faces, density and clearance estimates, and the whole fan
 * of triangles that tie exactly at a shared vertex, of which rt_nearest_points answers one).
 * Query i is a point q with an optional bound max_dist2[i]. Its candidate set is rt_nearest_points' own, in its order:
 *   S_i = { j : D(q, triangle j) <= min(max_dist2[i], FLT_MAX) }, ordered by (D ascending, original index ascending),
 * D and P exactly as the block above states them.
 * tri[i][0..max_tris) receives the first max_tris entries of S_i (unused slots: -1), d2[i][0..max_tris) their D (unused
 * slots: FLT_MAX), point[i][0..max_tris)[3] their P (unused slots: q's own bits). count[i] = min(|S_i|, max_tris), or
 * |S_i| itself with count_all; max_tris = 0 with count_all is a pure radius count.
 * S_i is empty when nothing lies within the bound, when max_dist2[i] is NaN or negative (0 is a valid bound) and for a
 * non-finite q (decided before any walk). max_dist2 NULL or +inf: no bound; with count_all the query then counts every
 * triangle whose D does not overflow, which costs a full traversal of the scene. No input value is an error.
 * With max_tris = 1 and no count_all, tri, d2 and point are rt_nearest_points' answer bit for bit.
 * RT_KERNEL_STRICT tests every point against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * pruning at min(the bound, the max_tris-th D found so far) -- at the bound alone with count_all -- and answers with
 * the same bits; a scene without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under
 * either kernel.
 * A neighbours query touches nothing a render or any other query owns. */
#define RT_NEIGHBOURS_MAX 16
typedef struct rt_neighbours {
    const float* point;     /* device, [n][3] f32 */
    const float* max_dist2; /* device, [n] f32, nullable */
    int n;                  /* >= 0; 0 is RT_OK and launches nothing */
    int max_tris;           /* 0..RT_NEIGHBOURS_MAX */
    int count_all;          /* 0 / 1 */
    int kernel;             /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_neighbours;
typedef struct rt_neighbour_results { /* device pointers, all nullable: [n][max_tris], [n][max_tris],
                                         [n][max_tris][3], [n] */
    int* tri;
    float* d2;
    float* point;
    int* count;   /* required for max_tris = 0 */
} rt_neighbour_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, a null point with n > 0, max_tris outside 0..RT_NEIGHBOURS_MAX, max_tris > 0 with tri, d2
 * and point all NULL, max_tris = 0 without count_all and a count pointer, count_all not 0 / 1, an unknown kernel, a
 * negative n. */
int rt_nearest_tris(rt_ctx* ctx, const rt_neighbours* points, const rt_neighbour_results* out);
typedef struct rt_neighbours_info {
    long long points, found;              /* found: points with a non-empty S_i */
    long long tris_stored, tris_counted;  /* sums of min(|S_i|, max_tris) and of count[i] */
    long long walked_points;              /* points that walked the wide view */
    long long exhaustive_points;  /* points tested against every triangle: all valid ones under RT_KERNEL_STRICT or
                                     without a wide view (a non-finite point or a NaN / negative bound is in neither) */
    long long empty_points;       /* points - found */
    long long nodes_visited;      /* wide nodes decoded, summed over the points (a level popped again counts again) */
    long long tris_tested;        /* triangle tests, summed over the points (exhaustive: points x triangles) */
    long long stack_overflows;    /* must be 0 */
    float kernel_ms;              /* HIP events around the query's launch */
} rt_neighbours_info;
/* counters of the last neighbours query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results
 * are not valid), RT_E_STATE before the first */
int rt_get_neighbours_info(rt_ctx* ctx, rt_neighbours_info* info);

/* Overlap queries: per caller-supplied axis-aligned box the triangles that touch it, and how many -- the query for a
 * volume (filling a voxel grid, the faces under a moving body's bounds, what a culling cell holds, the cells of a
 * distance field that lie near the surface).
 * Query i is the closed box [lo, hi] (a box with lo == hi on one, two or three axes -- a plane, a line, a point -- is
 * valid). Its answer is
 *   S_i = { j : T(lo, hi, triangle j) }, ordered by original triangle index ascending,
 * and S_i is empty when any of the six numbers is non-finite or lo > hi on an axis (decided before any walk). No input
 * value is an error. T is computed in float32 exactly as follows, on a = v0, e1 = v1 - v0, e2 = v2 - v0 (rounded once,
 * as the uploaded or updated triangle records hold them), every operation rounded to float32, no FMA. With
 * b = a + e1 and c = a + e2:
 *   1. tlo = fminf(fminf(a, b), c); thi = fmaxf(fmaxf(a, b), c)                                   per component
 *      T is false unless tlo.k <= hi.k && thi.k >= lo.k on all three axes k
 *   2. T is true if tlo.k >= lo.k && thi.k <= hi.k on all three axes
 *   3. ctr = 0.5*lo + 0.5*hi;  h = 0.5*hi - 0.5*lo;  v0 = a - ctr; v1 = b - ctr; v2 = c - ctr
 *      for each edge f of f0 = e1, f1 = e2 - e1, f2 = e2 and each axis k, with i = (k+1)%3, j = (k+2)%3:
 *        p_m = v_m.j * f.i - v_m.i * f.j   (m = 0, 1, 2);   rad = h.i * |f.j| + h.j * |f.i|
 *        the axis separates when fminf(fminf(p_0, p_1), p_2) > rad or fmaxf(fmaxf(p_0, p_1), p_2) < -rad
 *      nrm = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x)
 *      d = (nrm.x*v0.x + nrm.y*v0.y) + nrm.z*v0.z;   r = (h.x*|nrm.x| + h.y*|nrm.y|) + h.z*|nrm.z|
 *      the plane separates when |d| > r
 *      T is true when none of the ten separates (a comparison with a NaN operand separates nothing)
 * This is Akenine-Moller's triangle-box test behind two exact steps: 1 lets the walk drop a subtree by comparisons
 * alone, with no margin; 2 reports every triangle inside the box whatever 3 would round to.
 * Results: tri[i][0..max_tris) receives the first max_tris members of S_i by index (unused slots: -1);
 * count[i] = min(|S_i|, max_tris), or |S_i| itself with count_all; max_tris = 0 with count_all is a pure count.
 * The list form (offsets and list given): list[offsets[i] .. offsets[i+1]) receives members of S_i until it is full.
 * When the segment holds at least |S_i| entries its first |S_i| entries are S_i as a set, in no stated order; the rest
 * of the segment is not written, and nothing outside it is. count and tri are what they are without a list. A segment
 * whose end lies below its start, or whose start is negative, has no length. It may be combined with max_tris = 0.
 * RT_KERNEL_STRICT tests every box against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view and
 * answers with the same bits; a scene without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either.
 * An overlap query touches nothing a render or any other query owns. */
#define RT_OVERLAPS_MAX 16
typedef struct rt_boxes {
    const float* lo;     /* device, [n][3] f32 */
    const float* hi;     /* device, [n][3] f32 */
    const int* offsets;  /* device, [n + 1] i32, non-decreasing; nullable: given exactly when rt_overlap_results.list is */
    int n;               /* >= 0; 0 is RT_OK and launches nothing */
    int max_tris;        /* 0..RT_OVERLAPS_MAX */
    int count_all;       /* 0 / 1 */
    int kernel;          /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_boxes;
typedef struct rt_overlap_results { /* device pointers */
    int* tri;   /* [n][max_tris]; required for max_tris > 0 */
    int* count; /* [n]; nullable for max_tris > 0, required for max_tris = 0 */
    int* list;  /* [offsets[n]]; nullable: given exactly when rt_boxes.offsets is */
} rt_overlap_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, a null lo or hi with n > 0, max_tris outside 0..RT_OVERLAPS_MAX, max_tris > 0 without tri,
 * max_tris = 0 without count_all and a count pointer, count_all not 0 / 1, offsets without list or list without
 * offsets, an unknown kernel, a negative n. */
int rt_overlap_boxes(rt_ctx* ctx, const rt_boxes* boxes, const rt_overlap_results* out);
typedef struct rt_overlaps_info {
    long long boxes, found;               /* found: boxes with a non-empty S_i */
    long long tris_stored, tris_counted;  /* sums of min(|S_i|, max_tris) and of count[i] */
    long long tris_listed;                /* entries written to list: the sum of min(|S_i|, the segment's length) */
    long long walked_boxes;               /* boxes that walked the wide view */
    long long exhaustive_boxes;  /* boxes tested against every triangle: all valid ones under RT_KERNEL_STRICT or without
                                    a wide view (an invalid box is in neither) */
    long long empty_boxes;       /* boxes - found */
    long long nodes_visited;     /* wide nodes decoded, summed over the boxes */
    long long tris_tested;       /* evaluations of T, summed over the boxes (exhaustive: boxes x triangles; the walk
                                    takes the triangles of a leaf slot that lies inside the box without one) */
    long long stack_overflows;   /* must be 0 */
    float kernel_ms;             /* HIP events around the query's launch */
} rt_overlaps_info;
/* counters of the last overlap query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_overlaps_info(rt_ctx* ctx, rt_overlaps_info* info);

/* Sweep queries: per caller-supplied moving sphere the first contact with the mesh -- the query for a body of finite
 * size that moves (continuous collision of particles, camera and character probes, thick rays, path clearance): raycast,
 * overlap, sweep.
 * Query i is a sphere of radius r whose centre at time t is c + t d, d not normalised, over 0 <= t <= T with
 * T = fminf(t_max[i], FLT_MAX) (t_max NULL or +inf: no bound). Its answer is the first element of
 *   S_i = { j : toi(i, triangle j) exists }, ordered by (toi ascending, original index ascending):
 * a total order, so the answer depends on no BVH, and triangles that share the touched edge or vertex (an exact tie)
 * answer with the lowest index. S_i is empty, decided before any walk, when any of c, d, r is non-finite, when r < 0,
 * and when t_max[i] is NaN or negative. 0 is a valid bound ("does it touch now"), d = 0 a valid motion with the same
 * meaning, r = 0 a valid thin sweep. No input value is an error.
 * toi is computed in float32 exactly as follows on a triangle's record a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0), every
 * operation rounded to float32, dot(u, v) = u.x*v.x + u.y*v.y + u.z*v.z left to right, no FMA, IEEE division and sqrtf,
 * fminf / fmaxf with C semantics. With b = a + e1, cc = a + e2, r2 = r*r, dd = dot(d, d):
 *   1. The gate. tlo = fminf(fminf(a, b), cc); thi = fmaxf(fmaxf(a, b), cc)   (rt_overlap_boxes' step 1)
 *      glo = tlo - r; ghi = thi + r; t0 = 0; t1 = T; then for each axis k:
 *        d.k == 0: the triangle is out unless glo.k <= c.k && c.k <= ghi.k
 *        else      inv = 1 / d.k; ta = (glo.k - c.k) * inv; tb = (ghi.k - c.k) * inv
 *                  t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb))
 *      the triangle is out unless t0 <= t1
 *   2. Recentre. c0 = c + d*t0. If D(c0, triangle) <= r2 (rt_nearest_points' D) then toi = t0; with t0 = 0 this is a
 *      sphere that touches at the start.
 *   3. Candidates u >= 0 measured from t0; the least valid one counts.
 *      face:     n = rt_overlap_boxes' nrm; nn = dot(n, n); ln = sqrtf(nn); so = dot(n, c - a); dn = dot(n, d)
 *                sg = so < 0 ? -1 : 1; tf = (sg*(r*ln) - so) / dn
 *                valid when nn > 0 && dn*sg < 0 && tf >= 0 and rt_nearest_points' region algorithm at c + d*tf reaches
 *                its last case (the interior); u = fmaxf(tf - t0, 0). (The face uses the ORIGINAL centre: the plane's
 *                side is not decided at c0, which lies within rounding of a flat triangle's plane when r is small.)
 *      edges (p, f) = (a, e1), (a, e2), (b, e2 - e1):
 *                m = c0 - p; md = dot(m, f); nd = dot(d, f); ff = dot(f, f); A = ff*dd - nd*nd; K = dot(m, m) - r2
 *                Cq = ff*K - md*md; Bq = ff*dot(m, d) - nd*md; disc = Bq*Bq - A*Cq; u = (-Bq - sqrtf(disc)) / A
 *                s = md + u*nd; valid when A > 0 && disc >= 0 && u >= 0 && 0 <= s && s <= ff
 *      vertices v = a, b, cc:
 *                m = c0 - v; Bv = dot(m, d); Cv = dot(m, m) - r2; disc = Bv*Bv - dd*Cv; u = (-Bv - sqrtf(disc)) / dd
 *                valid when dd > 0 && disc >= 0 && u >= 0
 *      No valid candidate: the triangle is out. Otherwise toi = t0 + u, and the triangle is in S_i iff toi <= T.
 * This is the ray c + t d against the Minkowski sum of the triangle and the sphere: the prism's side walls lie inside the
 * edge cylinders and the cylinders' caps inside the vertex spheres, so the least valid candidate is the first entry.
 * The set differs from the real-number one only within rounding of a grazing contact. toi >= t0 holds by construction,
 * and the gate is monotone in the box planes: the walk drops a subtree whose gate interval is empty or starts strictly
 * after the best toi so far, with no margin. r = 0 is a thin sweep whose bits are NOT rt_trace_hits': it
 * is another formula, with none of the ray tests' EPSILON culls.
 * Results: tri[i] = the original triangle index, t[i] = toi, point[i] = rt_nearest_points' P of the centre
 * C = c + d*toi on that triangle: the contact point (the caller's normal is C - P). The empty set gives -1, FLT_MAX and
 * c's own bits.
 * RT_KERNEL_STRICT runs every sweep against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * slots in order of their gate t0 and pruned by the best toi, and answers with the same bits. A scene without a wide view
 * (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel, and so does, under RT_KERNEL_FAST, a sweep outside
 * the walk's domain: max|c.k| <= 2^20 mx, r <= 2^20 mx (mx: rt_update_info.scene_magnitude's quantity) and every nonzero
 * |d.k| within [2^-64, 2^64], where the gate makes no NaN.
 * A sweep query touches nothing a render or any other query owns. */
typedef struct rt_spheres {
    const float* centre;  /* device, [n][3] f32: c */
    const float* motion;  /* device, [n][3] f32: d, not normalised; the centre at time t is c + t d */
    const float* radius;  /* device, [n] f32: r >= 0 */
    const float* t_max;   /* device, [n] f32, nullable (NULL or +inf: no bound) */
    int n;                /* >= 0; 0 is RT_OK and launches nothing */
    int kernel;           /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_spheres;
typedef struct rt_sweep_results {   /* device pointers, all nullable, at least one non-null when n > 0 */
    int* tri;     /* [n] */
    float* t;     /* [n] */
    float* point; /* [n][3] */
} rt_sweep_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, a null centre, motion or radius with n > 0, all three outputs NULL with n > 0, an unknown
 * kernel, a negative n. */
int rt_sweep_spheres(rt_ctx* ctx, const rt_spheres* spheres, const rt_sweep_results* out);
typedef struct rt_sweep_info {
    long long spheres, found;     /* found: sweeps with a non-empty S_i */
    long long empty_spheres;      /* spheres - found */
    long long walked_spheres;     /* sweeps that walked the wide view */
    long long exhaustive_spheres; /* sweeps run against every triangle: all valid ones under RT_KERNEL_STRICT or without
                                     a wide view, and those outside the walk's domain (an invalid sweep is in neither) */
    long long nodes_visited;      /* wide nodes decoded, summed over the sweeps (a level popped again counts again) */
    long long tris_tested;        /* evaluations of toi, summed over the sweeps (exhaustive: sweeps x triangles) */
    long long stack_overflows;    /* must be 0 */
    float kernel_ms;              /* HIP events around the query's launch */
} rt_sweep_info;
/* counters of the last sweep query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are not
 * valid), RT_E_STATE before the first */
int rt_get_sweep_info(rt_ctx* ctx, rt_sweep_info* info);

/* Contact queries: per caller-supplied moving sphere the k earliest contacts with the mesh, and how many there are --
 * rt_sweep_spheres' plural form (every triangle a sphere touches where it starts, every triangle that shares the touched
 * edge or vertex, the sheets behind the first one, the triangles a capsule overlaps).
 * Query i is rt_sweep_spheres' own: centre c + t d, radius r, 0 <= t <= T = fminf(t_max[i], FLT_MAX). Its candidate set
 * is the sweep's own, in its order:
 *   S_i = { j : toi(i, triangle j) exists and toi <= T }, ordered by (toi ascending, original index ascending),
 * with toi exactly the sequence stated for rt_sweep_spheres above (gate, recentre, seven candidates). toi of a pair does
 * NOT depend on the bound: T enters step 1 only as the first value of t1, t0 is made of 0 and the plane times, and steps 2
 * and 3 read t0 alone. The bound only decides rejection (t0 <= t1, toi <= T), so a pair has one toi whatever limit a walk
 * holds when it meets it; the plural form relies on that.
 * S_i is empty, decided before any walk, under the sweep's rules: a non-finite c, d or r, r < 0, a NaN or negative
 * t_max[i]. No input value is an error.
 * Results, for max_tris in 0..RT_CONTACTS_MAX:
 *   tri[i][0..max_tris)       the first max_tris entries of S_i (unused slots: -1)
 *   t[i][0..max_tris)         their toi (unused slots: FLT_MAX)
 *   point[i][0..max_tris)[3]  rt_nearest_points' P of the centre c + d*toi_j on triangle j: each contact's own contact
 *                             point; the caller's normal is (c + d*toi_j) - P (unused slots: c's own bits)
 *   count[i]                  min(|S_i|, max_tris), or |S_i| itself with count_all
 * max_tris = 0 needs count_all and a count pointer: the pure count. With t_max = 1 it is the number of triangles that
 * the capsule from c to c + d of radius r touches.
 * With max_tris = 1 and no count_all, tri, t and point are rt_sweep_spheres' answer bit for bit. A d = 0 count is NOT
 * promised to equal rt_nearest_tris' radius count bit for bit: the gate's rounded tlo - r can differ from D <= r*r by
 * an ulp.
 * RT_KERNEL_STRICT runs every sweep against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * slots in order of their gate t0, pruned at fminf(T, the max_tris-th toi found so far) -- at T alone with count_all --
 * and answers with the same bits. A scene without a wide view (RT_ACCEL_REFERENCE) and a sweep outside
 * rt_sweep_spheres' walk domain run the exhaustive loop under either kernel.
 * A contacts query touches nothing a render or any other query owns. */
#define RT_CONTACTS_MAX 16
typedef struct rt_sphere_contacts {
    const float* centre;  /* device, [n][3] f32: c */
    const float* motion;  /* device, [n][3] f32: d, not normalised */
    const float* radius;  /* device, [n] f32: r >= 0 */
    const float* t_max;   /* device, [n] f32, nullable (NULL or +inf: no bound) */
    int n;                /* >= 0; 0 is RT_OK and launches nothing */
    int max_tris;         /* 0..RT_CONTACTS_MAX */
    int count_all;        /* 0 / 1 */
    int kernel;           /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_sphere_contacts;
typedef struct rt_contact_results { /* device pointers, all nullable: [n][max_tris], [n][max_tris],
                                       [n][max_tris][3], [n] */
    int* tri;
    float* t;
    float* point;
    int* count;   /* required for max_tris = 0 */
} rt_contact_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, a null centre, motion or radius with n > 0, max_tris outside 0..RT_CONTACTS_MAX,
 * max_tris > 0 with tri, t and point all NULL, max_tris = 0 without count_all and a count pointer, count_all not 0 / 1,
 * an unknown kernel, a negative n. */
int rt_sweep_contacts(rt_ctx* ctx, const rt_sphere_contacts* spheres, const rt_contact_results* out);
typedef struct rt_contacts_info {
    long long spheres, found;             /* found: sweeps with a non-empty S_i */
    long long tris_stored, tris_counted;  /* sums of min(|S_i|, max_tris) and of count[i] */
    long long walked_spheres;             /* sweeps that walked the wide view */
    long long exhaustive_spheres; /* sweeps run against every triangle: all valid ones under RT_KERNEL_STRICT or without
                                     a wide view, and those outside the walk's domain (an invalid sweep is in neither) */
    long long empty_spheres;      /* spheres - found */
    long long nodes_visited;      /* wide nodes decoded, summed over the sweeps (a level popped again counts again) */
    long long tris_tested;        /* evaluations of toi, summed over the sweeps (exhaustive: sweeps x triangles) */
    long long stack_overflows;    /* must be 0 */
    float kernel_ms;              /* HIP events around the query's launch */
} rt_contacts_info;
/* counters of the last contacts query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_contacts_info(rt_ctx* ctx, rt_contacts_info* info);

/* Cut queries: per caller-supplied triangle the mesh triangles it crosses, how many, and the segment along which each
 * pair crosses -- the query for the shape the scene itself is made of (mesh against mesh: the faces of a part, a tool
 * or a cloth that cross the uploaded mesh; cutting: where a sheet crosses the surface, as segments that chain into
 * cross-section polylines; clash checks of a placed component).
 * Query i is a triangle with corners q0, q1, q2 (float32, as given). Its answer is
 *   S_i = { j : X(q, triangle j) }, ordered by original triangle index ascending,
 * and S_i is empty, decided before any walk, when any of the nine numbers is non-finite. No input value is an error.
 * X is computed in float32 exactly as follows, on a triangle's record a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0), every
 * operation rounded once, no FMA, dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z, u x v by the formula of rt_overlap_boxes'
 * nrm, IEEE division, fminf / fmaxf with C semantics, a comparison with a NaN operand false. With b = a + e1,
 * c = a + e2, f1 = q1 - q0, f2 = q2 - q0:
 *   1. The gate. qlo = fminf(fminf(q0, q1), q2); qhi = fmaxf(fmaxf(q0, q1), q2)                  per component
 *      tlo, thi: rt_overlap_boxes' step 1
 *      X is false unless tlo.k <= qhi.k && thi.k >= qlo.k on all three axes k
 *   2. The mesh triangle against the query's plane. nq = f1 x f2; dm_m = dot(nq, m - q0) for m = a, b, c
 *      X is false when all three are > 0, all three are < 0, or all three are == 0 (a coplanar pair, a query of zero
 *      area: neither is a member)
 *   3. The query against the mesh triangle's plane. nm = e1 x e2; dq_m = dot(nm, q_m - a) for m = 0, 1, 2
 *      the same three rejections
 *   4. The line. D = nq x nm; k = 0; k = 1 if |D.y| > |D.x|; then k = 2 if |D.z| > |D.k|
 *   5. Each triangle's interval on the line (Moller's interval test), from its corners v0..v2 (a, b, c; q0, q1, q2)
 *      and their distances d0..d2 (dm; dq), with s_m = (d_m > 0) - (d_m < 0). The lone corner al is the first of
 *        s0 == s1 && s0 != 0: 2;  s0 == s2 && s0 != 0: 1;  (s1 == s2 && s1 != 0) || s0 != 0: 0;  s1 != 0: 1;  else 2
 *      and for the other two corners x = (al+1)%3, y = (al+2)%3:
 *        lam_x = d_al / (d_al - d_x);  P_x = v_al + (v_x - v_al) * lam_x  per component;  t_x = P_x.k;  the same for y
 *      The triangle's start point is P_x if t_x <= t_y, else P_y; its end point the other.
 *      lo = fminf(t_x, t_y); hi = fmaxf(t_x, t_y)
 *   6. Overlap. With [mlo, mhi] the mesh triangle's interval and [qlo_t, qhi_t] the query's:
 *      X is true iff mlo <= qhi_t && qlo_t <= mhi (closed)
 * The cut segment of a member: s0 = the query's start point if qlo_t > mlo, else the mesh triangle's start point;
 * s1 = the query's end point if qhi_t < mhi, else the mesh triangle's end point. So s0.k <= s1.k up to NaN.
 * Step 1 lets the walk drop a subtree by comparisons alone, with no margin. The set differs from the
 * real-number one only within rounding of a grazing contact.
 * Results: tri[i][0..max_tris) receives the first max_tris members of S_i by index (unused slots: -1);
 * count[i] = min(|S_i|, max_tris), or |S_i| itself with count_all; max_tris = 0 with count_all is a pure count.
 * The list form (offsets and list given) follows rt_overlap_boxes' rules: list[offsets[i] .. offsets[i+1]) receives
 * members of S_i until it is full, in no stated order; the rest of the segment is not written, and nothing outside it
 * is. With list_seg, a member written to list[p] has its s0 and s1 written to list_seg[p][0] and list_seg[p][1].
 * Segments exist only in the list form; tri holds indices only.
 * RT_KERNEL_STRICT tests every query against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view
 * against the query's corner box and answers with the same bits; a scene without a wide view (RT_ACCEL_REFERENCE) runs
 * the exhaustive loop under either.
 * A cut query touches nothing a render or any other query owns. */
#define RT_CUTS_MAX 16
typedef struct rt_tris {
    const float* tris;   /* device, [n][3][3] f32: q0, q1, q2 of every query */
    const int* offsets;  /* device, [n + 1] i32, non-decreasing; nullable: given exactly when rt_cut_results.list is */
    int n;               /* >= 0; 0 is RT_OK and launches nothing */
    int max_tris;        /* 0..RT_CUTS_MAX */
    int count_all;       /* 0 / 1 */
    int kernel;          /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_tris;
typedef struct rt_cut_results { /* device pointers */
    int* tri;        /* [n][max_tris]; required for max_tris > 0 */
    int* count;      /* [n]; nullable for max_tris > 0, required for max_tris = 0 */
    int* list;       /* [offsets[n]]; nullable: given exactly when rt_tris.offsets is */
    float* list_seg; /* [offsets[n]][2][3] f32; nullable; only with list */
} rt_cut_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, null tris with n > 0, max_tris outside 0..RT_CUTS_MAX, max_tris > 0 without tri,
 * max_tris = 0 without count_all and a count pointer, count_all not 0 / 1, offsets without list or list without
 * offsets, list_seg without list, an unknown kernel, a negative n. */
int rt_cut_triangles(rt_ctx* ctx, const rt_tris* tris, const rt_cut_results* out);
typedef struct rt_cuts_info {
    long long triangles, found; /* found: query triangles with a non-empty S_i */
    long long stored, counted;  /* sums of min(|S_i|, max_tris) and of count[i] */
    long long listed;           /* entries written to list: the sum of min(|S_i|, the segment's length) */
    long long walked;           /* query triangles that walked the wide view */
    long long exhaustive;       /* query triangles tested against every triangle: all valid ones under RT_KERNEL_STRICT
                                   or without a wide view (an invalid one is in neither) */
    long long empty;            /* triangles - found */
    long long nodes_visited;    /* wide nodes decoded, summed over the queries */
    long long pairs_tested;     /* evaluations of X, summed over the queries (exhaustive: queries x triangles) */
    long long stack_overflows;  /* must be 0 */
    float kernel_ms;            /* HIP events around the query's launch */
} rt_cuts_info;
/* counters of the last cut query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are not
 * valid), RT_E_STATE before the first */
int rt_get_cuts_info(rt_ctx* ctx, rt_cuts_info* info);

/* Clearance queries: per caller-supplied triangle the nearest mesh triangle, the squared distance to it and the pair of
 * points where the two come closest -- rt_cut_triangles' distance form, as rt_nearest_points is a point's (the clearance
 * of a placed part against the scene, tolerance and clash margins, proximity pairs for cloth and contact solvers, the
 * gap between a tool and a surface: what is asked as soon as rt_cut_triangles answers "nothing").
 * Query i is a triangle q0, q1, q2 with an optional bound max_dist2[i]. Its candidate set is
 *   S_i = { j : D(q, triangle j) <= min(max_dist2[i], FLT_MAX) }, ordered by (D ascending, original index ascending),
 * and the answer is its first element: a total order, so the answer depends on no BVH.
 * Every operation is one float32 operation and nothing is contracted into an FMA. dot(u, v) = u.x*v.x + u.y*v.y + u.z*v.z
 * left to right; clamp01(x) = fminf(fmaxf(x, 0), 1); fminf / fmaxf with C semantics (a NaN operand loses); IEEE
 * division; a comparison with a NaN operand is false.
 * Records and boxes. The mesh triangle is its record a = v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0), with corners a,
 * b = fl(a + e1), c = fl(a + e2) and corner box [tlo, thi] (rt_overlap_boxes' step 1). The query is made a record the
 * same way: f1 = fl(q1 - q0), f2 = fl(q2 - q0), qb = fl(q0 + f1), qc = fl(q0 + f2). The query box [qlo, qhi] is the
 * componentwise fminf / fmaxf over the FIVE points q0, q1, q2, qb, qc (folded in that order): it holds the raw corners
 * that rt_cut_triangles' X gates on and the record corners that the candidates use.
 * D of a pair is the least of fifteen candidates, offered in this order; a candidate replaces the pair's best only when
 * its D is strictly smaller:
 *   0..2    the query corners q0, qb, qc against the mesh record, by rt_nearest_points' own D and P: the pair of points
 *           is (corner, P);
 *   3..5    the mesh corners a, b, c against the query record (q0, f1, f2), by the same function: the pair is
 *           (P, corner);
 *   6..14   the nine edge pairs, query edge major: candidate 6 + 3*i + j is query edge i of (q0, f1), (q0, f2),
 *           (qb, fl(f2 - f1)) against mesh edge j of (a, e1), (a, e2), (b, fl(e2 - e1)). An edge pair (p1, d1), (p2, d2):
 *             r = p1 - p2;  A = dot(d1, d1);  E = dot(d2, d2);  f = dot(d2, r);  c = dot(d1, r);  B = dot(d1, d2)
 *             den = A*E - B*B
 *             s = den > 0 ? clamp01((B*f - c*E) / den) : 0
 *             t = (B*s + f) / E
 *             if (t < 0) s = clamp01(-c / A); else if (t > 1) s = clamp01((B - c) / A)
 *             t = clamp01(t)
 *             c1 = p1 + d1*s;  c2 = p2 + d2*t
 *             c1 = fminf(fmaxf(c1, qlo), qhi);  c2 = fminf(fmaxf(c2, tlo), thi)                       per component
 *             df = c1 - c2;  D = dot(df, df);  the pair is (c1, c2)
 * The crossing. After the fifteen, if rt_cut_triangles' X(q0, q1, q2; triangle) holds -- that test unchanged, on the
 * raw corners --, then D = 0 and both points are the cut segment's first end s0.
 * Every candidate's two points lie in [qlo, qhi] and [tlo, thi], which is what lets the walk prune with no tuned margin
 * (DESIGN.md §3y); every D is >= +0, and the fifteen candidates' points are finite for finite triangles.
 * Results: tri[i] = the original triangle index, d2[i] = D, on_query[i] and on_mesh[i] = the pair of points, kind[i] =
 * 0..14 for the winning candidate and 15 for a crossing. The empty set gives -1, FLT_MAX, q0's own bits twice and -1;
 * it is empty when any of the nine numbers is non-finite (decided before any walk), when max_dist2[i] is NaN or
 * negative, or when nothing lies within the bound (0 is a valid bound: what touches). max_dist2 NULL or +inf: no bound.
 * No input value is an error.
 * Documented, not fixed:
 *   - A query of zero area is valid and is answered by the fifteen candidates alone: X excludes it, as
 *     rt_cut_triangles does. One with q1 == q2 is a segment, one with all three corners equal a point. A needle that
 *     pierces a triangle's interior therefore reports the distance to that triangle's boundary, not 0. Segments belong
 *     to rt_sweep_spheres with r = 0 and t_max = 1, points to rt_nearest_points.
 *   - For a point query D is not promised to equal rt_nearest_points' bit for bit: an edge candidate may round an ulp
 *     lower.
 * RT_KERNEL_STRICT tests every query against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * boxes ordered and pruned by their distance to the query box, and answers with the same bits; a scene without a wide
 * view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel.
 * A clearance query touches nothing a render or any other query owns. */
typedef struct rt_clear_tris {
    const float* tris;      /* device, [n][3][3] f32: q0, q1, q2 of every query */
    const float* max_dist2; /* device, [n] f32, nullable */
    int n;                  /* >= 0; 0 is RT_OK and launches nothing */
    int kernel;             /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_clear_tris;
typedef struct rt_clearance_results { /* device pointers, all nullable, at least one non-null when n > 0 */
    int* tri;        /* [n] */
    float* d2;       /* [n] */
    float* on_query; /* [n][3] */
    float* on_mesh;  /* [n][3] */
    int* kind;       /* [n] */
} rt_clearance_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, null tris with n > 0, all five outputs NULL with n > 0, an unknown kernel, a negative n. */
int rt_clearance_triangles(rt_ctx* ctx, const rt_clear_tris* tris, const rt_clearance_results* out);
typedef struct rt_clearance_info {
    long long triangles, found; /* found: query triangles with a non-empty S_i */
    long long walked;           /* query triangles that walked the wide view */
    long long exhaustive;       /* query triangles tested against every triangle: all valid ones under RT_KERNEL_STRICT
                                   or without a wide view (an invalid one is in neither) */
    long long empty;            /* triangles - found */
    long long nodes_visited;    /* wide nodes decoded, summed over the queries (a level popped again counts again) */
    long long pairs_gated;      /* the walk: triangles of a kept leaf slot skipped because the bound of their own corner
                                   box exceeded the limit, or equalled the best D at a higher index (pure pruning; 0 in
                                   the exhaustive loop) */
    long long pairs_tested;     /* evaluations of D, summed over the queries (exhaustive: queries x triangles) */
    long long stack_overflows;  /* must be 0 */
    float kernel_ms;            /* HIP events around the query's launch */
} rt_clearance_info;
/* counters of the last clearance query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_clearance_info(rt_ctx* ctx, rt_clearance_info* info);

/* Proximity queries: per caller-supplied triangle the k nearest mesh triangles, their squared distances and pairs of
 * closest points, and the number of mesh triangles within a margin -- rt_clearance_triangles' plural form, as
 * rt_nearest_tris is rt_nearest_points' (every mesh face within a cloth or contact solver's collision margin with the
 * closest points of each pair, the number of faces closer than a tolerance, the few closest faces of a clash report).
 * Query i is a triangle q0, q1, q2 with an optional bound max_dist2[i]. Its candidate set is clearance's own, in
 * clearance's order:
 *   S_i = { j : D(q, triangle j) <= fminf(max_dist2[i], FLT_MAX) }, ordered by (D ascending, original index ascending).
 * D, the pair of points and kind are exactly rt_clearance_triangles' sequence above: the fifteen candidates, then the
 * crossing (kind 15, D = 0, both points the cut segment's first end). D of a pair is a function of the query and the
 * mesh triangle alone: it depends on no limit a walk holds and on nothing found before it, so a pair has the same bits
 * in every list, count and segment, under every kernel and view. The plural form relies on that.
 * S_i is empty, decided before any walk, under clearance's rules: any of the nine numbers non-finite, or max_dist2[i]
 * NaN or negative. 0 is a valid bound (what touches); max_dist2 NULL or +inf: no bound. No input value is an error.
 * Results, for max_tris (k) in 0..RT_PROXIMITY_MAX; the slots past |S_i| of query i are its unused slots:
 *   tri[i][0..k)       the first k entries of S_i                       unused slots: -1
 *   d2[i][0..k)        their D                                          unused slots: FLT_MAX
 *   on_query[i][0..k)  each pair's point on the query                   unused slots: q0's own bits
 *   on_mesh[i][0..k)   each pair's point on the mesh triangle           unused slots: q0's own bits
 *   kind[i][0..k)      each entry's winning candidate, 0..15            unused slots: -1
 *   count[i]           min(|S_i|, k), or |S_i| itself with count_all
 * max_tris = 0 with count_all is the pure count: how many mesh triangles lie within the margin. With count_all the
 * walk prunes at the query's bound alone; without a bound that is a full traversal.
 * With max_tris = 1 and no count_all, tri, d2, on_query, on_mesh and kind equal rt_clearance_triangles' bit for bit.
 * With a bound of 0, S_i contains rt_cut_triangles' S_i for the same triangle. It may hold more -- touching pairs whose
 * fifteen candidates give exactly 0 -- so the two are not promised equal.
 * The list form (offsets and list given) follows rt_cut_triangles' rules: list[offsets[i] .. offsets[i+1]) receives
 * members of S_i until it is full, in no stated order; the rest of the segment is not written, and nothing outside it
 * is. A member written to list[p] has its D in list_d2[p], its points in list_points[p][0] (on the query) and
 * list_points[p][1] (on the mesh triangle) and its kind in list_kind[p], where those are given. In the list form the
 * walk prunes at the query's bound alone, as with count_all, whatever max_tris is.
 * RT_KERNEL_STRICT tests every query against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * boxes ordered and pruned by their distance to the query box against min(the bound, the k-th D found so far), and
 * answers with the same bits; a scene without a wide view (RT_ACCEL_REFERENCE) runs the exhaustive loop under either.
 * A proximity query touches nothing a render or any other query owns. */
#define RT_PROXIMITY_MAX 16
typedef struct rt_prox_tris {
    const float* tris;      /* device, [n][3][3] f32: q0, q1, q2 of every query */
    const float* max_dist2; /* device, [n] f32, nullable */
    const int* offsets;     /* device, [n + 1] i32, non-decreasing; nullable: given exactly when
                               rt_proximity_results.list is */
    int n;                  /* >= 0; 0 is RT_OK and launches nothing */
    int max_tris;           /* 0..RT_PROXIMITY_MAX */
    int count_all;          /* 0 / 1 */
    int kernel;             /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_prox_tris;
typedef struct rt_proximity_results { /* device pointers, all nullable within the rules below */
    int* tri;           /* [n][max_tris] */
    float* d2;          /* [n][max_tris] */
    float* on_query;    /* [n][max_tris][3] */
    float* on_mesh;     /* [n][max_tris][3] */
    int* kind;          /* [n][max_tris] */
    int* count;         /* [n]; required for max_tris = 0 */
    int* list;          /* [offsets[n]]; given exactly when rt_prox_tris.offsets is */
    float* list_d2;     /* [offsets[n]]; only with list */
    float* list_points; /* [offsets[n]][2][3] f32; only with list */
    int* list_kind;     /* [offsets[n]]; only with list */
} rt_proximity_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, null tris with n > 0, max_tris outside 0..RT_PROXIMITY_MAX, max_tris > 0 with tri, d2,
 * on_query, on_mesh and kind all NULL, max_tris = 0 without count_all and a count pointer, count_all not 0 / 1, offsets
 * without list or list without offsets, list_d2, list_points or list_kind without list, an unknown kernel, a negative
 * n. */
int rt_proximity_triangles(rt_ctx* ctx, const rt_prox_tris* tris, const rt_proximity_results* out);
typedef struct rt_proximity_info {
    long long triangles, found; /* found: query triangles with a non-empty S_i */
    long long stored, counted;  /* sums of min(|S_i|, max_tris) and of count[i] */
    long long listed;           /* entries written to list: the sum of min(|S_i|, the segment's length) */
    long long walked;           /* query triangles that walked the wide view */
    long long exhaustive;       /* query triangles tested against every triangle: all valid ones under RT_KERNEL_STRICT
                                   or without a wide view (an invalid one is in neither) */
    long long empty;            /* triangles - found */
    long long nodes_visited;    /* wide nodes decoded, summed over the queries (a level popped again counts again) */
    long long pairs_gated;      /* the walk: triangles of a kept leaf slot skipped because the bound of their own corner
                                   box exceeded the limit, or because the list was full and their least possible key
                                   lay beyond its last (pure pruning; 0 in the exhaustive loop) */
    long long pairs_tested;     /* evaluations of D, summed over the queries (exhaustive: queries x triangles); the
                                   second evaluation that fills on_query, on_mesh and kind is not counted */
    long long stack_overflows;  /* must be 0 */
    float kernel_ms;            /* HIP events around the query's launch */
} rt_proximity_info;
/* counters of the last proximity query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results are
 * not valid), RT_E_STATE before the first */
int rt_get_proximity_info(rt_ctx* ctx, rt_proximity_info* info);

/* Triangle sweep queries: per caller-supplied moving triangle the first contact with the mesh -- rt_clearance_triangles'
 * motion form, as rt_sweep_spheres is a point query's (continuous collision of a part, a tool or a cloth face against the
 * mesh, how far a placed component can travel along a direction before it clashes, the time of impact a contact solver
 * needs so that a face does not tunnel through a thin sheet between two samples).
 * Query i is a triangle q0, q1, q2 that translates without rotating: its corners at time t are q + t d, d not
 * normalised, over 0 <= t <= T with T = fminf(t_max[i], FLT_MAX) (t_max NULL or +inf: no bound). Its answer is the first
 * element of
 *   S_i = { j : toi(i, triangle j) exists and <= T }, ordered by (toi ascending, original index ascending):
 * a total order, so the answer depends on no BVH, and an exact tie (triangles that share the touched edge or corner)
 * goes to the lower index. S_i is empty, decided before any walk, when one of the twelve numbers of q0, q1, q2, d is
 * non-finite, and when t_max[i] is NaN or negative (the sign read from the bits: a negative subnormal is negative, -0 is
 * the bound 0). t_max = 0 and d = 0 both ask "does it touch now". No input value is an error.
 * Every operation is one float32 operation and nothing is contracted into an FMA. dot(u, v) = u.x*v.x + u.y*v.y + u.z*v.z
 * left to right; cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x); fminf / fmaxf with C semantics
 * (a NaN operand loses); IEEE division; a comparison with a NaN operand is false.
 *   1. Records and boxes are rt_clearance_triangles' own. The mesh triangle is its record a = v0, e1 = fl(v1 - v0),
 *      e2 = fl(v2 - v0) with corners a, b = fl(a + e1), c = fl(a + e2) and corner box [tlo, thi]. The query is made a
 *      record the same way: f1 = fl(q1 - q0), f2 = fl(q2 - q0), qb = fl(q0 + f1), qc = fl(q0 + f2); [qlo, qhi] is the
 *      componentwise fminf / fmaxf over the FIVE points q0, q1, q2, qb, qc (folded in that order).
 *   2. The gate. t0 = 0; t1 = T; then for each axis k:
 *        d.k == 0: the triangle is out unless qlo.k <= thi.k && tlo.k <= qhi.k
 *        else      inv = 1 / d.k; ta = (tlo.k - qhi.k) * inv; tb = (thi.k - qlo.k) * inv
 *                  t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb))
 *      the triangle is out unless t0 <= t1. (rt_sweep_spheres' slab gate with the query's box in the sphere's place.)
 *   3. Recentre. sh = d*t0; r0 = q0 + sh, r1 = q1 + sh, r2 = q2 + sh, rb = qb + sh, rc = qc + sh. f1 and f2 keep their
 *      bits.
 *   4. A start in contact. If rt_cut_triangles' X(r0, r1, r2; triangle) holds -- that test unchanged, on the recentred
 *      raw corners --, then toi = t0, kind = 15 and the point is the cut segment's first end s0. (With t0 > 0 this is a
 *      query whose box and the triangle's first meet where the triangles do, as on an axis-aligned wall.)
 *   5. Otherwise fifteen candidates u >= 0 measured from t0, offered in rt_clearance_triangles' order; a candidate
 *      replaces the best only when it is valid and strictly smaller.
 *      ray(o, dr; p, g1, g2), the one ray-triangle function, with no EPSILON culls:
 *                h = cross(dr, g2); det = dot(g1, h); inv = 1 / det; s = o - p; bu = dot(s, h) * inv
 *                qv = cross(s, g1); bv = dot(dr, qv) * inv; u = dot(g2, qv) * inv
 *                valid when det != 0 && bu >= 0 && bv >= 0 && bu + bv <= 1 && u >= 0
 *      0..2      o = r0, rb, rc: ray(o, d; a, e1, e2); the point is o + d*u
 *      3..5      v = a, b, c: ray(v, -d; r0, f1, f2); the point is v
 *      6..14     candidate 6 + 3*i + j is query edge i of (r0, f1), (r0, f2), (rb, fl(f2 - f1)) against mesh edge j of
 *                (a, e1), (a, e2), (b, fl(e2 - e1)). An edge pair (p, f), (m, e):
 *                n = cross(f, e); nn = dot(n, n); dn = dot(d, n); w0 = m - p; u = dot(w0, n) / dn
 *                rn = 1 / nn; w = w0 - d*u; s = dot(cross(w, e), n) * rn; t = dot(cross(w, f), n) * rn
 *                valid when nn > 0 && dn != 0 && u >= 0 && 0 <= s && s <= 1 && 0 <= t && t <= 1; the point is m + e*t
 *      No valid candidate: the triangle is out. Otherwise toi = t0 + u (so toi >= t0 by construction), and the triangle
 *      is in S_i iff toi <= T.
 *   6. Results: tri[i] = the original triangle index, t[i] = toi, point[i] = the contact point on the mesh triangle
 *      stated above, each component clamped fminf(fmaxf(., tlo), thi), kind[i] = 0..14 for the winning candidate and 15
 *      for a start in contact. The empty set gives -1, FLT_MAX, q0's own bits and -1.
 * The gate is monotone in the mesh-side box planes, so the walk drops a subtree whose gate interval is empty or starts
 * strictly after the best toi so far, with no margin.
 * Documented, not fixed:
 *   - Motion inside the common plane of a coplanar pair gives no contact (X excludes the pair, every det and dn is 0 up
 *     to rounding), and contacts of exactly parallel edges give none (nn = 0): a face that lands flat on a coplanar
 *     face is reported through its corners, when they lie within the other's closed bounds.
 *   - A query of zero area (a segment, a point) is valid and is answered by the candidates alone: X excludes it, as
 *     rt_cut_triangles does.
 *   - toi at a grazing contact, as with rt_sweep_spheres at r = 0, is exact only to rounding: the set differs from the
 *     real-number one only within rounding of a contact at a boundary.
 *   - Coordinates whose triple products overflow float32 (beyond about 2^42) make every det, dn and plane distance
 *     infinite or NaN: no candidate is valid and the answer is the empty set.
 * RT_KERNEL_STRICT runs every query against every triangle (the checker); RT_KERNEL_FAST walks the full 8-wide view,
 * slots in order of their gate t0 and pruned by the best toi, and answers with the same bits. A scene without a wide view
 * (RT_ACCEL_REFERENCE) runs the exhaustive loop under either kernel, and so does, under RT_KERNEL_FAST, a query outside
 * the walk's domain: every |q.k| <= 2^20 mx (mx: rt_update_info.scene_magnitude's quantity) and every nonzero |d.k|
 * within [2^-64, 2^64], where the gate makes no NaN.
 * A triangle sweep query touches nothing a render or any other query owns. */
typedef struct rt_sweep_tris {
    const float* tris;   /* device, [n][3][3] f32: q0, q1, q2 of every query */
    const float* motion; /* device, [n][3] f32: d, not normalised; a corner at time t is q + t d */
    const float* t_max;  /* device, [n] f32, nullable (NULL or +inf: no bound) */
    int n;               /* >= 0; 0 is RT_OK and launches nothing */
    int kernel;          /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_sweep_tris;
typedef struct rt_trisweep_results { /* device pointers, all nullable, at least one non-null when n > 0 */
    int* tri;     /* [n] */
    float* t;     /* [n] */
    float* point; /* [n][3] */
    int* kind;    /* [n] */
} rt_trisweep_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, null tris or motion with n > 0, all four outputs NULL with n > 0, an unknown kernel, a
 * negative n. */
int rt_sweep_triangles(rt_ctx* ctx, const rt_sweep_tris* tris, const rt_trisweep_results* out);
typedef struct rt_trisweep_info {
    long long triangles, found; /* found: query triangles with a non-empty S_i */
    long long empty;            /* triangles - found */
    long long walked;           /* query triangles that walked the wide view */
    long long exhaustive;       /* query triangles run against every triangle: all valid ones under RT_KERNEL_STRICT or
                                   without a wide view, and those outside the walk's domain (an invalid one is in neither) */
    long long nodes_visited;    /* wide nodes decoded, summed over the queries (a level popped again counts again) */
    long long pairs_gated;      /* the walk: triangles of a visited leaf slot turned away by their own gate (0 in the
                                   exhaustive loop) */
    long long pairs_tested;     /* the walk: triangles past their own gate; exhaustive: queries x triangles */
    long long stack_overflows;  /* must be 0 */
    float kernel_ms;            /* HIP events around the query's launch */
} rt_trisweep_info;
/* counters of the last triangle sweep query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its results
 * are not valid), RT_E_STATE before the first */
int rt_get_trisweep_info(rt_ctx* ctx, rt_trisweep_info* info);

/* Triangle contact queries: per caller-supplied moving triangle the k earliest contacts with the mesh and the number of
 * contacts -- rt_sweep_triangles' plural form, as rt_sweep_contacts is rt_sweep_spheres' (every mesh triangle that
 * shares the touched edge or corner: they tie at one time of impact; every triangle a face already touches where it
 * starts, to be pushed out of; the sheets behind the first one; the number of mesh triangles that the swept volume of
 * the face touches).
 * Query i is rt_sweep_triangles' own: corners q + t d over 0 <= t <= T = fminf(t_max[i], FLT_MAX). Its candidate set is
 * the sweep's own, in the sweep's order:
 *   S_i = { j : toi(i, triangle j) exists and toi <= T }, ordered by (toi ascending, original index ascending),
 * and it is empty under the sweep's rules, decided before any walk: a non-finite one among the twelve numbers of q0,
 * q1, q2, d, or a NaN or negative t_max[i], the sign read from the bits. toi, the contact point and the kind of a pair
 * are steps 1-6 of rt_sweep_triangles above, not restated here.
 * A pair's toi, point and kind depend on the query and the triangle alone: not on the bound (T enters the gate as the
 * first value of the interval's end t1 and the last comparison toi <= T, and nothing else reads either), and not on any
 * other member of S_i. The form rests on this: a member has the same bits at every max_tris, with and without
 * count_all, under every bound that keeps it, and in rt_sweep_triangles' own answer.
 * Results, for max_tris (k) in 0..RT_TRICONTACTS_MAX; the slots past |S_i| of query i are its unused slots:
 *   tri   [n][k]     the first k entries of S_i; -1 in unused slots
 *   t     [n][k]     their toi; FLT_MAX in unused slots
 *   point [n][k][3]  each pair's own contact point (step 6); q0's own bits in unused slots
 *   kind  [n][k]     each pair's own kind, 0..15; -1 in unused slots
 *   count [n]        min(|S_i|, k), or |S_i| itself with count_all
 * max_tris = 0 needs count_all and a count pointer and is the pure count; with t_max = 1 it is the number of mesh
 * triangles that the prism swept from q to q + d touches. With max_tris = 1 and no count_all, tri, t, point and kind
 * are rt_sweep_triangles' answer bit for bit.
 * Not promised: a t_max = 0 or d = 0 set is not rt_cut_triangles' set, nor rt_proximity_triangles' set at bound 0 -- the
 * gate and the touching candidates differ from those queries' tests by rounding.
 * Documented, not fixed, as for rt_sweep_triangles: motion inside the common plane of a coplanar pair and contacts of
 * exactly parallel edges give no member; a query of zero area is answered by the candidates alone; membership at a
 * grazing contact is exact only to rounding; coordinates whose triple products overflow float32 (beyond about 2^42)
 * give the empty set.
 * RT_KERNEL_STRICT runs every query against every triangle under T (the checker); RT_KERNEL_FAST walks the full 8-wide
 * view, slots in order of their gate t0, pruned by lim = fminf(T, the k-th stored toi once the list is full) -- T alone
 * with count_all -- and answers with the same bits. A scene without a wide view and, under
 * RT_KERNEL_FAST, a query outside rt_sweep_triangles' walk domain run the exhaustive loop.
 * A triangle contact query touches nothing a render or any other query owns. */
#define RT_TRICONTACTS_MAX 16
typedef struct rt_tri_contacts {
    const float* tris;   /* device, [n][3][3] f32: q0, q1, q2 of every query */
    const float* motion; /* device, [n][3] f32: d, not normalised */
    const float* t_max;  /* device, [n] f32, nullable (NULL or +inf: no bound) */
    int n;               /* >= 0; 0 is RT_OK and launches nothing */
    int max_tris;        /* 0..RT_TRICONTACTS_MAX */
    int count_all;       /* 0 / 1: count holds |S_i| itself */
    int kernel;          /* RT_KERNEL_AUTO (= FAST) / STRICT / FAST */
} rt_tri_contacts;
typedef struct rt_tricontact_results { /* device pointers, all nullable */
    int* tri;     /* [n][max_tris] */
    float* t;     /* [n][max_tris] */
    float* point; /* [n][max_tris][3] */
    int* kind;    /* [n][max_tris] */
    int* count;   /* [n] */
} rt_tricontact_results;
/* asynchronous on the context stream; elements at index n and beyond are not written. RT_E_STATE before an upload;
 * RT_E_ARG for a null struct, null tris or motion with n > 0, max_tris outside 0..RT_TRICONTACTS_MAX, max_tris > 0 with
 * tri, t, point and kind all NULL (whatever count is), max_tris = 0 without count_all and a count pointer, count_all not
 * 0 or 1, an unknown kernel, a negative n. */
int rt_sweep_tri_contacts(rt_ctx* ctx, const rt_tri_contacts* tris, const rt_tricontact_results* out);
typedef struct rt_tricontacts_info {
    long long triangles, found; /* found: query triangles with a non-empty S_i */
    long long stored;           /* list entries written (sum of min(|S_i|, max_tris)) */
    long long counted;          /* sum of the count output (whether or not it was asked for) */
    long long walked;           /* query triangles that walked the wide view */
    long long exhaustive;       /* query triangles run against every triangle: all valid ones under RT_KERNEL_STRICT or
                                   without a wide view, and those outside the walk's domain (an invalid one is in neither) */
    long long empty;            /* triangles - found */
    long long nodes_visited;    /* wide nodes decoded, summed over the queries (a level popped again counts again) */
    long long pairs_gated;      /* the walk: triangles of a visited leaf slot turned away by their own gate (0 in the
                                   exhaustive loop) */
    long long pairs_tested;     /* the walk: triangles past their own gate; exhaustive: queries x triangles; the second
                                   evaluation that fills point and kind is not counted */
    long long stack_overflows;  /* must be 0 */
    float kernel_ms;            /* HIP events around the query's launch */
} rt_tricontacts_info;
/* counters of the last triangle contact query (synchronises); RT_E_KERNEL when it overflowed the walk's stack (its
 * results are not valid), RT_E_STATE before the first */
int rt_get_tricontacts_info(rt_ctx* ctx, rt_tricontacts_info* info);

/* Vertex updates: moving geometry without a new upload. Every view of the uploaded scene -- the reference tree of the
 * strict walk, the binary acceleration view where one exists, the 8-wide full / unit / primary views, the triangle
 * records, the shading normals, the box-face lists -- is refitted on the device to the new coordinates; topology stays.
 *
 * The contract: after rt_update_vertices every render, ray query and radiance query, strict kernel and every fast
 * variant, gives the bits a fresh rt_upload_scene of the scene S' gives, where
 *   triangles[i] = triangle_init(coords'[i], ks_i, kd_i, kr_i): materials kept, centroid and norm[0], norm[1]
 *                  recomputed exactly as cpu/src/triangle.c:14-19 computes them;
 *   bvh          = the uploaded reference tree with the same child, tr_len and tri_idx, every node's min / max regrown
 *                  as cpu/src/bvh.c grows it: aabb_grow over the node's triangles' vertices starting from +-1e10 (an
 *                  empty node keeps +-1e10);
 *   lights, ambient and accel mode unchanged.
 * What an update is not: a new bvh_build of the moved triangles, whose topology can differ from the kept one. That
 * difference shows only at exact ties (the first-found rule follows the tree's order).
 * The fast views keep their topology too, which can only cost speed (rt_update_info.area_ratio says how loose the
 * full view's boxes have become); a subset view (unit, primary) that newly hittable triangles must join cannot be
 * refitted and is rebuilt through the upload's own path, on the host (views_rebuilt; a triangle that stops being
 * hittable simply stays in its view). rt_scene_info's view fields follow what the update did.
 * The default rule's per-shape launch decisions survive an update (an animation does not re-trial every frame); the
 * query and shade state is untouched; the inflation 2^-16 x magnitude and the queries' origin bound follow the new
 * coordinates.
 * Errors: RT_E_STATE before an upload; RT_E_ARG for a null pointer, a count mismatch, a non-finite coordinate or one
 * beyond RT_COORD_MAX -- found by a read-only first pass, so a refused update leaves the scene exactly as it was.
 * coords is read in stream order on the context stream. The call waits on the host once, for that first pass's few
 * words (and, the first time after an upload or a rebuild, before that pass, for the trees' level lists and the face
 * lists' buffers); everything after is asynchronous, except a view's rebuild. */
typedef struct rt_vertex_update {
    const float* coords;  /* device, [n_triangles][3][3] f32: the new triangle_t.coords of every triangle, original order */
    int n_triangles;      /* must equal the uploaded scene's */
} rt_vertex_update;
int rt_update_vertices(rt_ctx* ctx, const rt_vertex_update* u);

typedef struct rt_update_info {
    int views_refit, views_rebuilt;   /* wide views (full / unit / primary) refitted in place / rebuilt because membership changed */
    int joined_unit, joined_primary;  /* triangles that became hittable for a view they were absent from (what forces a rebuild) */
    float scene_magnitude;            /* the new scene's, as the boxes' inflation uses it */
    float area_ratio;                 /* full view: summed surface area of all decoded child boxes now / when the view was last built (1 without a wide view) */
    float update_ms;                  /* HIP events around the whole update on the context stream */
} rt_update_info;
/* of the last update (synchronises); RT_E_STATE before the first update */
int rt_get_update_info(rt_ctx* ctx, rt_update_info* info);

/* New light positions and colours: a stream-ordered copy (host array; n_lights must equal the scene's) */
int rt_update_lights(rt_ctx* ctx, const rt_light* lights, int n_lights);

/* Test-only read-back of a wide view as it stands on the device (synchronises): view 0 = full, 1 = unit, 2 = primary.
 * Returns the view's node count (0: no such view) or < 0; copies min(count, cap_nodes) nodes of 20 words into nodes and
 * min(triangles, cap_tris) entries of the view's position -> original triangle map into tri_orig (both nullable).
 * tests/test_gpu_refit.py compares the words with rth_wbvh_refit's. Not part of the supported interface. */
int rt_debug_read_wide(rt_ctx* ctx, int view, unsigned int* nodes, int cap_nodes, int* tri_orig, int cap_tris);

/* ---- view rebuilds: new topologies for the fast walk's wide views after large motion.
 * rt_update_vertices keeps every tree's topology; after large motion the wide views' boxes overlap and frames slow down
 * (rt_update_info.area_ratio). rt_rebuild_views does everything rt_update_vertices does for the same coords -- the plan
 * pass with its refusals, records, normals, reference tree, binary acceleration view, faces, a refit of the wide views
 * -- and then gives the wide views (full, unit, primary) a new topology built from those device-resident coordinates.
 * The reference tree is kept, so every render, ray query and radiance query, strict kernel and every fast variant,
 * returns exactly the bits it returns after rt_update_vertices of the same coords: the fast walk gives the reference's
 * bits on any conservative BVH, the views only change speed.
 * The subset views follow the upload's rule over the new coordinates (hittable triangles, and only when there are some
 * and fewer than the upload's limits): a view may appear, disappear or change size exactly as in a fresh upload.
 * The new views are built into fresh buffers and swapped in in stream order; the old ones and their refit data are
 * freed; rt_update_info.area_ratio is measured against the rebuilt view from then on; rt_scene_info's view fields follow.
 * The default rule's per-shape launch decisions survive, query / shade / update-info state is untouched.
 * Modes:
 *   RT_REBUILD_HOST    the upload's own path over downloaded coordinates (PLOC or binned SAH as the scene was built,
 *                      the host treelet pass, the cost-optimal collapse): the quality of a fresh upload.
 *   RT_REBUILD_DEVICE  no tree leaves the device: subset compaction, PLOC from the device vertices, the greedy collapse
 *                      (rt_collapse.hpp; no treelet pass, no cost model), then the refit's own fill of boxes and records.
 *                      The host reads back a few counts per PLOC round and per wide level. Only for a scene whose
 *                      accel_built is RT_ACCEL_GPU (RT_E_ARG otherwise); RT_E_STATE, with the refitted scene left in
 *                      place, when a device tree is deeper than the wide walk's stack.
 *   RT_REBUILD_AUTO    DEVICE where it is allowed, falling back to HOST when a device tree is too deep or larger than
 *                      the packed layouts' node bound; HOST for a host-built scene.
 * Errors: RT_E_STATE before an upload and for a scene without a wide view (RT_ACCEL_REFERENCE); the update's own errors
 * and refusals unchanged (a non-finite coordinate changes nothing). A failure after the update step returns its error
 * and leaves the refitted scene, which is valid. The call waits on the host (counts, and in HOST mode the whole build). */
enum { RT_REBUILD_AUTO = 0, RT_REBUILD_DEVICE = 1, RT_REBUILD_HOST = 2 };
typedef struct rt_view_rebuild {
    const float* coords;  /* device, [n_triangles][3][3] f32, as rt_vertex_update.coords */
    int n_triangles;      /* must equal the uploaded scene's */
    int mode;             /* RT_REBUILD_* */
} rt_view_rebuild;
int rt_rebuild_views(rt_ctx* ctx, const rt_view_rebuild* r);

typedef struct rt_rebuild_info {
    int mode_used;            /* RT_REBUILD_DEVICE or RT_REBUILD_HOST */
    int fell_back;            /* RT_REBUILD_AUTO on a GPU-built scene used HOST: 1 too deep, 2 too many nodes; else 0 */
    int views_built;          /* wide views built (1..3) */
    int nodes[3], depth[3];   /* per view (full, unit, primary): wide nodes and levels; 0: no such view now */
    int launches;             /* DEVICE: kernel launches and copies issued by the build (PLOC, collapse, fill) */
    double area_before;       /* full view: summed decoded child-box area just after the refit ... */
    double area_after;        /* ... and just after the rebuild (rt_refit.hpp k_wide_area) */
    float rebuild_ms;         /* HIP events on the context stream around the whole call's device work */
    float host_ms;            /* the call's wall time */
    float ploc_ms, collapse_ms, fill_ms; /* wall time of the stages, summed over the views (HOST: ploc includes the
                                            treelet pass, fill the upload of the views) */
} rt_rebuild_info;
/* of the last rebuild (synchronises); RT_E_STATE before the first rebuild */
int rt_get_rebuild_info(rt_ctx* ctx, rt_rebuild_info* info);

/* Test-only read-back of the binary tree the last RT_REBUILD_DEVICE rebuild collapsed for a view (0 = full, 1 = unit,
 * 2 = primary), so that the CPU mirror (rth_wbvh_build_greedy) can be given the same input. Layout: a view of n
 * triangles has nodes 0 .. n - 1 = leaves, leaf k holding scene triangle leaf_tri[k], and nodes n .. 2 n - 2 = merges
 * whose children are left[id - n] and right[id - n]; *root is the root's id. Returns n (0: no such view or no device
 * rebuild) or < 0; copies min(n, cap) leaf_tri entries and min(n - 1, cap) left / right entries (all nullable).
 * Not part of the supported interface. */
int rt_debug_read_build_tree(rt_ctx* ctx, int view, int* left, int* right, int* leaf_tri, int cap, int* root);

/* load_from_gpu(): copies the last frame's compact rows to host (synchronous); nullable args. RT_E_KERNEL when the
 * render reported a traversal-stack overflow (its frame is not valid). */
int rt_download(rt_ctx* ctx, float* h_rgb, int* h_hit);
/* waits for the stream; kernel_ms (nullable) = the last render's kernel time from HIP events; RT_E_KERNEL when the
 * last render reported a traversal-stack overflow */
int rt_sync(rt_ctx* ctx, float* kernel_ms);
/* per-launch kernel times (HIP events recorded on the context stream around each kernel) of the last
 * n launches (n <= 64), oldest first; synchronises; returns the number written or < 0. A launch's time is one value:
 * rt_sync and rt_kernel_times read its event pair once and return that figure on every later call. */
int rt_kernel_times(rt_ctx* ctx, float* ms, int n);
/* Multi-GPU in one process without RCCL (the fallback of the CLI's --gpus N; also several contexts on ONE
 * device): gathers the last render of n contexts -- a frame or a frame batch, f32 rgb or BGRA8 (rt_outputs.bgra),
 * the same kind on every context -- into ctxs[root]'s full frames [frames][height][width]. Every context must
 * have rendered the same shape, and their row sets must partition each frame (rank g of n: cyclic rows
 * {g, n}, block-cyclic rows {g*B, n*B, .., row_block = B}, rotated residues with frame_shift).
 * Each source's xGMI peer copies are issued on ITS stream after its render (the sources' copy engines run at
 * once), the root waits for them (events) and un-interleaves the rows. Afterwards the root's last render is
 * the full frame(s) (rgb or bgra, and hit when every context wrote one): rt_download / rt_download_bmp read a
 * single frame. Asynchronous like rt_render. */
int rt_gather(rt_ctx* const* ctxs, int n, int root);
/* rt_gather into a caller's device buffer d_dst on the root's device ([frames][height][width] x 3 floats or
 * x 1 uint32, the last renders' kind), e.g. to keep a gathered frame batch; d_dst NULL = rt_gather */
int rt_gather_to(rt_ctx* const* ctxs, int n, int root, void* d_dst);

/* RCCL communicator over contexts (the framebuffer gather over xGMI). Two ways to build one:
 *   rt_comm_init      -- one process driving n devices (the CLI's --gpus N): ncclCommInitAll over the contexts'
 *                        devices, rank i = ctxs[i] (one context per device);
 *   rt_comm_init_rank -- one rank per process (N processes, one GPU each): ncclCommInitRank with an id that
 *                        rank 0 made with rt_comm_get_id and handed to every rank (any channel: MPI, a file,
 *                        torch.distributed). One communicator per rank serves every context of that rank on its
 *                        device (rt_comm_gather_from).
 * rt_comm_gather(comm, root, d_dst): every rank's last render (a frame or frame batch, rgb or BGRA8; the row
 * sets must partition each frame, as for rt_gather) is sent to `root` with ncclSend / ncclRecv in one group,
 * on each context's stream (so after its render), and un-interleaved there into d_dst ([frames][height][width]
 * x 3 floats or x 1 uint32; a device pointer on the root's device) or, with d_dst NULL, into the root
 * context's own buffer, which then is its last render (rt_download / rt_download_bmp). Collective: every rank
 * calls it. Asynchronous on the streams. Hit indices are not gathered (rt_gather does).
 * Across processes the ranks exchange their 64-B row-set descriptors (one ncclAllGather, a host wait) only on what
 * every rank sees the same way: the first gather, a new frame size, frame count or pixel kind (fields every rank of
 * a valid layout shares), or rt_comm_relayout called by every rank. A rank whose own rows change without one of
 * those is refused (RT_E_ARG) before any collective call. The root checks each exchanged layout partitions every
 * frame and, on the layout's first gather, that every pixel of the gathered frames arrived (one host wait per
 * layout); later gathers of the same layout neither exchange nor wait. Every host wait on a collective is bounded
 * (rt_comm_set_timeout, default 120 s): a peer that never joins turns into RT_E_TIMEOUT and an aborted communicator
 * (ncclCommAbort), never a hang. */
typedef struct rt_comm rt_comm;
#define RT_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct rt_comm_info {
    long long gathers;   /* rt_comm_gather / rt_comm_gather_from calls */
    long long exchanges; /* row-set descriptor exchanges (multi-process): one per layout */
    long long checked;   /* layouts whose first gather the root checked pixel by pixel */
    int nranks, rank;    /* the job's ranks; this communicator's (first local) rank */
} rt_comm_info;
int rt_comm_get_id(unsigned char* id /* RT_COMM_ID_BYTES */);
int rt_comm_init(rt_ctx* const* ctxs, int n, rt_comm** out);
int rt_comm_init_rank(rt_ctx* ctx, int nranks, int rank, const unsigned char* id, rt_comm** out);
int rt_comm_gather(rt_comm* comm, int root, void* d_dst);
/* rt_comm_gather of the last render of `src`, a context of this rank on the communicator's device (NULL: the
 * context the communicator was built with); multi-process communicators only. Successive gathers of one
 * communicator run in their call order, whatever streams their contexts use. */
int rt_comm_gather_from(rt_comm* comm, rt_ctx* src, int root, void* d_dst);
/* Collective: every rank calls it before the same gather, which then exchanges the row sets again (a rank's rows
 * may change there). */
int rt_comm_relayout(rt_comm* comm);
/* The deadline of every host wait on a collective of this communicator (seconds > 0; default 120). */
int rt_comm_set_timeout(rt_comm* comm, double seconds);
/* Waits, bounded by that deadline, until the communicator's last gather has run on the device: RT_OK, or
 * RT_E_TIMEOUT with the communicator aborted (a peer never joined). For a caller that would otherwise block in a
 * device synchronisation behind a collective that cannot complete. */
int rt_comm_wait(rt_comm* comm);
int rt_comm_get_info(rt_comm* comm, rt_comm_info* info);
const char* rt_comm_last_error(rt_comm* comm);
void rt_comm_destroy(rt_comm* comm);
/* bmp_write_file's bytes of the last frame (cpu/src/bmp_writer.c:88-211): 54-B header + BGRA8 rows
 * bottom-up, (uint8_t)(c * 255.0f) per channel (vec_to_bgra), quantised on the device. Needs a full
 * frame (all rows; after rt_gather for multi-GPU). cap >= 54 + 4 * width * height; synchronous. */
int rt_download_bmp(rt_ctx* ctx, unsigned char* h_bmp, size_t cap);
/* counters of the last rendered frame (synchronises) */
int rt_get_stats(rt_ctx* ctx, rt_stats* stats);
const char* rt_last_error(rt_ctx* ctx);
void rt_destroy(rt_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
