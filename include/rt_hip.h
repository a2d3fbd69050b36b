/*
 * rt_hip.h — C-ABI of the MI355X render path (librt_hip.so).
 *
 * This is the drop-in boundary that replaces the reference's device entry
 *   void launch_compute_image_device(vec4* d_pixels, vec4* d_tmpPixels,
 *        vec4* d_image, const int& width, const int& height,
 *        const Camera& camera, const vec4* d_lightsPos,
 *        const vec4* d_lightsColor, const int& nLights,
 *        const vec4& background, const vec4& ambience, const int& max_depth,
 *        const Data* data, const BVH::BVHNodes_SoA* bvhNodes);
 *   (declared mytracer_gpu.h:43-56, defined mytracer_gpu.cu:44-113)
 * together with the managed-memory scene it reads (struct Data, mydata.h:28-72;
 * BVH::BVHNodes_SoA, mybvh.h:49-55; allocated by Raytracer::build_Data,
 * mytracer.cpp:166-296, and BVH::initSoA, mybvh.cpp:375-406).
 *
 * Differences by design:
 *  - the scene is uploaded once with explicit hipMalloc/hipMemcpy into an
 *    MI355X layout (fp32 4-wide BVH nodes collapsed from the reference's
 *    binary tree, child boxes in the parent; the 2-wide form for the canonical
 *    counters; fp64 triangle records in leaf order); no managed memory;
 *  - the caller passes host SoA arrays (the reference's Data/BVHNodes_SoA
 *    content, same meaning, packed xyz instead of vec4) and owns the output;
 *  - errors are returned as status codes with the message in rt_last_error()
 *    (the reference's CHECK prints and continues, common/common.h:6-15);
 *  - rows can be restricted / interleaved so one process per GPU renders its
 *    share of the image (the reference only uses device 0, mytracer_gpu.cu:34).
 * All pointers are plain; no torch or HIP types appear in the signatures
 * (streams are passed as void*).
 * Current device: a call that takes a scene makes the scene's device current on the calling
 * thread and leaves it so (rt_scene_upload*: `device`; rt_ipc_open: `device`), as the
 * reference's single-device code assumes; a caller driving several GPUs from one thread sets
 * its own device again after a call (rt_multi.h does).
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include "rt_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_INVALID (-1)     /* bad argument / inconsistent scene */
#define RT_ERR_HIP (-2)         /* HIP runtime failure */
#define RT_ERR_UNSUPPORTED (-3) /* scene exceeds a compiled limit (e.g. BVH depth, RT_MAX_COORDINATE) */

/* Lights held inline in rt_render_params (and staged in LDS by the kernel).  Scenes with
 * more lights pass them through rt_render_params.lights_ext (any count up to
 * RT_LIGHTS_LIMIT); the reference shades any nLights (mytracer_gpu.cu:632).  Every launch copies
 * its light table with its control block (as the reference's copyLights per call,
 * mytracer.cpp:105-118), so lights may change from call to call, on any stream, without a
 * device synchronisation. */
#define RT_MAX_LIGHTS 16
#define RT_LIGHTS_LIMIT (1 << 20)

/* Host SoA scene: the content of struct Data (mydata.h:28-72) after
 * BVH::initSoA has permuted the per-triangle arrays into leaf order
 * (mybvh.cpp:497-503).  Vectors are packed xyz (3 doubles). */
typedef struct rt_scene_soa {
  int n_meshes;          /* tMeshCount_ */
  int n_vertices;        /* tVertexCount_ */
  int n_vertex_idx;      /* tVertexIdxCount_ = 3 * n_triangles */
  int n_tex_coords;      /* tTextCoordCount_ */
  long long n_texels;    /* tTexelCount_ */
  const int* vertex_mesh_id;     /* [n_vertices]          vertexMeshId_ */
  const double* vertex_pos;      /* [3*n_vertices]        vertexPos_ */
  const double* vertex_normals;  /* [3*n_vertices]        vertexNormals_ */
  const double* face_normals;    /* [3*n_triangles]       normals_ (leaf order) */
  const int* vertex_idx;         /* [n_vertex_idx]        vertexIdx_ (leaf order, global ids) */
  const int* texture_idx;        /* [n_vertex_idx]        textureIdx_ (leaf order, global ids) */
  const double* tex_u;           /* [n_tex_coords]        textureCoordinatesU_ */
  const double* tex_v;           /* [n_tex_coords]        textureCoordinatesV_ */
  const unsigned char* texels;   /* [3*n_texels] RGB8     meshTexels_ (vec4 in the reference) */
  const int* mesh_tex_width;     /* [n_meshes], -1 = none meshTexWidth_ */
  const int* mesh_tex_height;    /* [n_meshes]            meshTexHeight_ */
  const long long* mesh_tex_offset; /* [n_meshes]         firstMeshTex_ */
  const int* mesh_draw_mode;     /* [n_meshes]            meshDrawMode_ */
  const double* mat_ambient;     /* [3*n_meshes]          materialAmbient_ */
  const double* mat_diffuse;     /* [3*n_meshes]          materialDiffuse_ */
  const double* mat_specular;    /* [3*n_meshes]          materialSpecular_ */
  const double* mat_shininess;   /* [n_meshes]            materialShininess_ */
  const double* mat_mirror;      /* [n_meshes]            materialMirror_ */
  const int* mat_shadowable;     /* [n_meshes]            materialShadowable_ */
} rt_scene_soa;

/* The reference's BVH::BVHNodes_SoA (mybvh.h:49-55), nodes [0, n_nodes). */
typedef struct rt_bvh_soa {
  int n_nodes;                 /* nodesUsed_ */
  const double* bb_min;        /* [3*n_nodes] */
  const double* bb_max;        /* [3*n_nodes] */
  const int* left_child;       /* [n_nodes]; right child = left_child + 1 */
  const int* first_tri;        /* [n_nodes] */
  const int* tri_count;        /* [n_nodes]; 0 = internal */
} rt_bvh_soa;

/* Output formats of rt_launch_compute_image. */
enum {
  RT_OUT_RGB_F32 = 0,  /* 3 floats per pixel (production) */
  RT_OUT_RGB_F64 = 1   /* 3 doubles per pixel (parity tests) */
};

/* Flags of rt_render_params.flags. */
enum {
  RT_FLAG_TRAVERSAL_STATS = 1, /* canonical counters: 2-wide traversal (the one the oracle replicates),
                                  counts node visits / triangle tests / closest hits */
  RT_FLAG_WIDE_STATS = 2,      /* same counters on the production 4-wide traversal (diagnostics) */
  RT_FLAG_TIMELINE = 4,        /* production kernel + per-round timeline (diagnostics, rt_debug_timeline) */
  RT_FLAG_TILE_COST = 8,       /* diagnostics: per-tile cost of the launch (rt_debug_tile_cost): bounces */
  RT_FLAG_TILE_COST_TIME = 16, /* ... the same, as pixel lifetimes (10-ns ticks) */
  RT_FLAG_COST_ORDER = 32,     /* cost-ordered work for one-frame launches (the reference's use): every work head
                                  renders first the tiles that took longest (pixel lifetimes) in the launch before
                                  the previous one of the same image geometry (animation: frame i - 2's costs
                                  order frame i), and this launch's costs are kept; shortens the end-of-launch
                                  drain, pixels unchanged.  The DEFAULT for one-frame launches
                                  on the stream of the scene's last ordered launch (or the first one-frame
                                  launch); launches on another stream keep the natural order unless they set
                                  this flag, which then makes them wait for the last ordered launch.
                                  Launches of several frames and adaptive passes keep the natural order and
                                  record nothing; one-frame launches of more than 32768 tiles (rt_tile_shape) keep
                                  the natural order */
  RT_FLAG_NATURAL_ORDER = 64,  /* one-frame launch in the natural tile order, recording no costs */
  RT_FLAG_GLOBAL_ROWS = 128    /* the output buffer holds the whole frame (camera.height rows): the shard's rows
                                  are written at their global positions (row y at y * width * 3), not packed.
                                  With a peer GPU's frame buffer (rt_ipc_open) every rank writes its stripes
                                  straight into the assembled frame over xGMI; each wave's stores are released
                                  at system scope before it exits.  Not for the adaptive pass nor
                                  rt_render_to_host (RT_ERR_INVALID) */
};

/* One render call.  Rows are rendered as interleaved stripes:
 * row y is rendered iff row_begin <= y < row_end and
 * (y / stripe_height) % stripe_count == stripe_index; rendered rows are
 * packed into the output in increasing y, row-major, pixel (x, y) of local
 * row r at out[(r*width + x)*3 + c] (the reference's pixels[y*W+x],
 * mytracer_gpu.cu:158).  stripe_count == 1 renders every row in range. */
typedef struct rt_render_params {
  rt_camera camera;
  int n_lights;                          /* <= RT_MAX_LIGHTS, or <= RT_LIGHTS_LIMIT with lights_ext */
  int max_depth;                         /* reflection bounces after the primary hit */
  rt_light lights[RT_MAX_LIGHTS];        /* used when lights_ext == NULL */
  double background[3];
  double ambience[3];
  int spp_n;            /* n: n*n stratified samples per pixel (mytracer_gpu.cu:202-221); 1 = one ray through (x,y) */
  int row_begin;
  int row_end;          /* <= 0 means camera.height */
  int stripe_height;    /* >= 1 */
  int stripe_count;     /* >= 1 */
  int stripe_index;     /* [0, stripe_count) */
  int out_format;       /* RT_OUT_* */
  int flags;            /* RT_FLAG_* */
  const rt_light* lights_ext;  /* non-NULL: the n_lights lights (host memory, read during the call) */
} rt_render_params;

/* Light i of a render call (lights_ext when set, else the inline table). */
static inline const rt_light* rt_params_light(const rt_render_params* p, int i) {
  return p->lights_ext ? &p->lights_ext[i] : &p->lights[i];
}

/* Ray counters of one launch (canonical definition: DESIGN.md §5).
 * primary = pixels*spp; shadow = shading points x lights with a shadowable
 * material (mytracer.cpp:589); reflection = shading points with mirror > 0
 * below max_depth (mytracer.cpp:547).  node_visits / tri_tests / hits are
 * filled only with RT_FLAG_TRAVERSAL_STATS (canonical 2-wide walk: exact, equal to the oracle's)
 * or RT_FLAG_WIDE_STATS (the 4-wide production traversal, every wave sorting children: with
 * shadow rays these vary by ~1e-5 between runs, as the postponed-leaf timing and the fan-out of
 * shadow rays to idle lanes depend on which rays share a wave). */
typedef struct rt_stats {
  long long primary_rays;
  long long shadow_rays;
  long long reflection_rays;
  long long node_visits;      /* fp32 2-wide nodes fetched (= internal-node pops) */
  long long tri_tests;        /* triangle records tested */
  long long closest_hits;     /* closest-hit rays that hit (shading fetches) */
  long long pixels;           /* pixels written */
  long long reserved_;
} rt_stats;

typedef struct rt_scene rt_scene;   /* opaque device-resident scene */

/* Largest vertex coordinate magnitude a scene may hold: 2^61, about 2.3e18 (see rt_scene_upload). */
#define RT_MAX_COORDINATE 2305843009213693952.0

/* Uploads the scene to HIP device `device` (hipSetDevice), converting the
 * host SoA + reference BVH into the MI355X layout.  Leaves the device current.
 *
 * Supported coordinate range (derivation: DESIGN.md §4, "Supported coordinate range").  Results do
 * not depend on the scene's scale or position: the fp32 boxes grow by 2^-20 max|vertex|, a relative
 * amount.  The only absolute limit is fp32's range: the 4-wide kernels multiply the ray origin,
 * moved into the root box, by a reciprocal direction clamped at 1e20, which overflows from
 * max|vertex| = 3.4e18 on.  A scene whose max|vertex| exceeds RT_MAX_COORDINATE is refused with
 * RT_ERR_UNSUPPORTED (one infinite coordinate included), whatever else it holds.  NaN coordinates are
 * not looked for: the reference box of their triangles excludes them and those triangles are never
 * hit.  Small scenes need no limit of this kind, but the reference's own absolute constants
 * (|S| < 1e-10 rejects a triangle, t <= 1e-5 a hit) empty a scene shrunk by about 2^-20.
 * Ray origins (camera eyes, lights, rt_ray origins) may lie far outside the scene: each ray enters
 * the root box at a point computed in fp64, whose rounding error, about 6 * 2^-53 times the origin's
 * distance D, stays inside the part of the box growth the fp32 error bound leaves free while
 * D <= 2^28 max|vertex|. */
int rt_scene_upload(const rt_scene_soa* soa, const rt_bvh_soa* bvh, int device, rt_scene** out);

/* Device traversal hierarchy (never changes a pixel or a ray count: the closest hit is
 * the smallest (t, reference slot) over a conservative superset of candidates, DESIGN.md
 * §4; the canonical counters always walk the reference tree given in `bvh`).
 *   RT_TREE_SBVH       binned SAH with spatial splits (straddling triangles referenced from
 *                      both sides, clipped bounds), 4-wide collapsed (default; builds ~5x
 *                      slower than RT_TREE_SAH: 16 s at 10 M triangles on 16 threads)
 *   RT_TREE_SAH        binned-SAH tree over all triangles (object splits only), 4-wide collapsed
 *   RT_TREE_REFERENCE  the reference median-split tree, oversize leaves refined */
enum { RT_TREE_SAH = 0, RT_TREE_REFERENCE = 1, RT_TREE_SBVH = 2 };
/* 4-wide collapse of the device hierarchy: open the child with the largest box, or the
 * SAH-optimal choice of up to 4 slots per node (dynamic programme; the default).
 * RT_COLLAPSE_BY_SIZE (the default before round 5: greedy below 2^18 input triangles) now
 * resolves to RT_COLLAPSE_SAH at every size. */
enum { RT_COLLAPSE_GREEDY = 0, RT_COLLAPSE_SAH = 1, RT_COLLAPSE_BY_SIZE = 2 };

/* Upload options.  The library reads nothing from the environment: its behaviour depends only
 * on these fields and the call's arguments.  Fill with rt_upload_options_init (the defaults),
 * then change fields:
 *     rt_upload_options o; rt_upload_options_init(&o); o.device_tree = RT_TREE_SAH;
 * A zero-initialised struct is valid too: zero in sbvh_bins, sbvh_c_trav, collapse_c_tri and
 * lds_treelet means their defaults; zero in device_tree / collapse / sbvh_alpha / sbvh_budget
 * selects RT_TREE_SAH / RT_COLLAPSE_GREEDY / alpha 0 / budget 0 (valid, but not the defaults).
 * None of them changes a pixel or a ray count: they pick the device hierarchy,
 * its build, and the kernel's LDS / grid layout. */
typedef struct rt_upload_options {
  int device_tree;       /* RT_TREE_* (default RT_TREE_SBVH) */
  int build_threads;     /* host threads of the builders; 0 = the CPUs this process may use (its
                            affinity mask, capped by a cgroup CPU quota), at most 64.
                            The hierarchy does not depend on it */
  int stack_ring;        /* LDS stack-ring entries of the production kernel: 0 = by size (16 from 2^18
                            device records on, else 8; default), 8 or 16 */
  int lds_treelet;       /* 4-wide nodes each block caches in LDS: 0 = as many as fit (default),
                            > 0 = at most this many, -1 = none */
  int collapse;          /* RT_COLLAPSE_* (default RT_COLLAPSE_SAH; RT_COLLAPSE_BY_SIZE resolves to it) */
  int sbvh_leaf_max;     /* SBVH: SAH-terminated leaves of up to this many references, 1..8 (1 = split
                            down to single references); 0 = by size (default): 1 from 2^18 input
                            triangles on, else 2 */
  int sbvh_bins;         /* SBVH: spatial bins per axis (default 32; 0 = default), 2..128 (64: 10 M random
                            triangles +1.7 % per frame for +64 % build time) */
  int blocks_per_cu;     /* persistent blocks per CU: 0 = as many as fit (default), else at most this many */
  int grid_spare;        /* block slots of the persistent grid left free for concurrent kernels (default 0) */
  int verbose;           /* 1: build phase times to stderr (default 0) */
  double sbvh_alpha;     /* SBVH: try spatial splits where the best object split's children overlap by
                            more than alpha x the root's surface area; < 0 = by size (default):
                            0 from 2^18 input triangles on, else 1e-5 */
  double sbvh_budget;    /* SBVH: at most this many extra references per triangle; < 0 = by size
                            (default): 1.5 from 2^18 input triangles on, else 0.75 */
  double sbvh_c_trav;    /* SBVH: node visit cost in triangle tests, for leaf termination (default 1.0;
                            0 = default) */
  double collapse_c_tri; /* RT_COLLAPSE_SAH: cost of a leaf slot per unit area (default 1.0; 0 = default) */
  int reserve_cus;       /* CUs each render launch leaves free for concurrent kernels (an RCCL gather of the
                            previous launch: its 256-VGPR waves fit no single free block slot of the
                            persistent grid): > 0 = the launches run on an internal stream
                            whose CU mask clears the first reserve_cus CUs, the grid sized to the rest
                            (32 = one XCD's worth: the smallest reservation a 256-VGPR kernel was
                            measured to run beside a stand-in of RCCL's kernel shape); 0 = none (default,
                            also in rt_multi_create: the reservation slows the render by ~12 % and
                            its gain at N > 1 is unmeasured; bench.py times both at N > 1); -1 = none */
  int order_window;      /* one-frame cost order (RT_FLAG_COST_ORDER, the default on one stream): a tile sorts by
                            the largest recorded cost within +-order_window tiles of its row; 0 = by size (4,
                            exact costs for hierarchies from 2^18 device records on, whatever stack_ring forces;
                            default), -1 = exact */
  int spp_lanes;         /* n x n > 1 samples per pixel, n^2 a power of two: 1 = a pixel's samples on
                            neighbouring lanes of one wave (groups of G = min(n^2, 32) lanes, summed in sample
                            order on chip), 2..64 (a power of two) = the same with G capped at that many
                            lanes (chunks of G samples in sequence), -1 = one lane per pixel, its samples in
                            sequence; 0 = the default,
                            groups (4K 16 spp +22.6 %, 8K 64 spp +19.3 %).  Launches with
                            other n, the diagnostic flags, tile-cost maps or RT_FLAG_COST_ORDER keep one lane
                            per pixel.  The adaptive pass follows it too (groups: no sample buffer, no
                            reduce kernel).  Pixels and ray counts are identical either way */
  int tree_opt;          /* subtree reinsertion on the finished binary hierarchy, before the wide collapse
                            (DESIGN.md §20): 0 = by size (default): on for RT_TREE_SBVH from 2^10 to below 2^18
                            input triangles (at most RT_TREE_OPT_PASSES passes), off otherwise; -1 = off;
                            1..RT_TREE_OPT_MAX = at most this many passes, whatever the tree and the size */
  int reserved_[4];
} rt_upload_options;

enum { RT_TREE_OPT_PASSES = 3, RT_TREE_OPT_MAX = 64 };

/* Fills *opt with the defaults listed above. */
void rt_upload_options_init(rt_upload_options* opt);

/* rt_scene_upload with options (NULL = defaults). */
int rt_scene_upload_ex(const rt_scene_soa* soa, const rt_bvh_soa* bvh, int device, const rt_upload_options* opt,
                       rt_scene** out);

/* Uploads one scene to several devices: the device layout (hierarchy, records) is built
 * once on the host and copied to devices[0..n_devices), one host thread per device.
 * outs[g] receives the scene on devices[g]; on failure every outs[g] is NULL.  The
 * multi-GPU driver (rt_multi.h) uses it. */
int rt_scene_upload_multi(const rt_scene_soa* soa, const rt_bvh_soa* bvh, const int* devices, int n_devices,
                          const rt_upload_options* opt, rt_scene** outs);

/* Device bytes held by the scene (nodes, triangles, shading data). */
long long rt_scene_device_bytes(const rt_scene* scene);

/* Host seconds of the scene's upload: build_s = the device layout built on the host (the device
 * hierarchy -- SBVH / SAH / refined reference tree --, its wide collapse, the triangle and shading
 * records; once for every device of rt_scene_upload_multi), copy_s = device allocation and the
 * H2D copies of this device.  The reference's own build (BVH::initSoA, mybvh.cpp:375-406) is the
 * caller's rt_host_prepare, timed separately.  Either pointer may be NULL. */
int rt_scene_upload_seconds(const rt_scene* scene, double* build_s, double* copy_s);

/* Opt-in analytic primitives: the spheres and planes of the
 * raw scene (rt_raw_scene.spheres / .planes), tested in fp64 before the BVH in
 * the CPU's order -- spheres, then planes, nearest strictly closer wins, then
 * triangles only if strictly closer (oracle intersect_scene; Sphere/Plane
 * intersect, myplane.cpp:22-49).  The reference GPU path traces meshes only
 * (intersect_scene_device, mytracer_gpu.cu:314-328); a scene without this call
 * matches it.  Replaces
 * any previous set; n = 0 removes them.  Synchronises the device. */
int rt_scene_set_analytic(rt_scene* scene, const rt_sphere* spheres, int n_spheres, const rt_plane* planes,
                          int n_planes);

/* Number of rows rt_launch_compute_image writes for these params. */
int rt_rows_in_shard(const rt_render_params* p);

/* Renders into the caller-owned DEVICE buffer d_out (rows x width x 3 of the
 * chosen format) on `stream` (hipStream_t, NULL = the null stream).
 * Asynchronous unless stats != NULL, in which case it synchronises the stream
 * and fills *stats.  Launches on different streams may run concurrently: the
 * scene keeps a ring of 8 launch contexts (path state, work heads, counters)
 * and a context is reused only after its previous launch completed.  Calls on
 * one scene must come from one host thread at a time.  Replaces launch_compute_image_device's primary pass
 * (mytracer_gpu.cu:66-81); the adaptive pass (:83-109) is SURVEY §8f "next". */
int rt_launch_compute_image(rt_scene* scene, const rt_render_params* p, void* d_out,
                            rt_stats* stats, void* stream);

/* Up to RT_MAX_FRAMES frames in ONE launch of the persistent kernel: frame f renders
 * p[f] into d_outs[f].  The frames share one work queue, so the tail of one frame is
 * filled with the next frame's pixels instead of idling (the per-launch drain is paid
 * once per batch).  p[f] may differ from p[0] only in camera.eye / lower_left / x_dir /
 * y_dir (an animation path); everything else must be identical.  stats (optional,
 * synchronising) sums the frames.  Results equal n_frames rt_launch_compute_image calls. */
#define RT_MAX_FRAMES 128
int rt_launch_frames(rt_scene* scene, const rt_render_params* p, int n_frames, void* const* d_outs,
                     rt_stats* stats, void* stream);

/* Adaptive supersampling pass: replaces adaptive_supersampling_device
 * (mytracer_gpu.cu:162-229, launched at :83-109 with subp = 4, threshold = 0.02).
 * d_primary: the primary pass of the SAME params rendered with
 * RT_OUT_RGB_F64 (H x W x 3 doubles, device).  Every interior pixel whose
 * squared colour differences to its 4 neighbours (x+1, y+1, x-1, y-1, in that
 * order) sum above `threshold` is re-rendered with subp x subp stratified
 * samples (averaged, clamped); all other pixels are copied from d_primary.
 * d_out (H x W x 3, p->out_format) must not alias d_primary.  Full frame only
 * (stripe_count 1, no row range).  stats (optional, synchronising) counts the
 * rays of this pass; *n_selected (optional, synchronising) = re-rendered pixels. */
int rt_launch_adaptive(rt_scene* scene, const rt_render_params* p, const double* d_primary, void* d_out, int subp,
                       double threshold, rt_stats* stats, long long* n_selected, void* stream);

/* Adaptive pass over n_frames full frames at once (animation / batched frames):
 * p[0..n_frames) differ only in their camera vectors (as rt_launch_frames), d_primary[f] is frame
 * f's fp64 primary image, d_out[f] its output.  Every frame's selection goes into one list and
 * one launch traces every sample of every selected pixel of every frame (a pixel's samples on
 * neighbouring lanes, as rt_launch_adaptive), so the per-launch drain is paid once per batch.
 * subp^2 a power of two (sample groups, rt_upload_options.spp_lanes >= 0): the render kernel sums
 * and stores each selected pixel itself and the call does not synchronise; otherwise a sample
 * buffer sized by the selection count, which the call reads back (one host synchronisation per
 * call), and a reduce kernel.  Results equal rt_launch_adaptive on each frame.  W x H < 2^25.
 * *n_selected (optional, synchronising) = pixels re-rendered over all frames. */
int rt_launch_adaptive_frames(rt_scene* scene, const rt_render_params* p, int n_frames, const double* const* d_primary,
                              void* const* d_out, int subp, double threshold, rt_stats* stats, long long* n_selected,
                              void* stream);

/* Adaptive pass over a row shard (the multi-GPU case).  p may use
 * stripes or a row range; d_primary / d_out are the shard's packed rows (as
 * rt_launch_compute_image writes them), d_primary in RT_OUT_RGB_F64.  The
 * neighbour test of a shard's first / last row in each run of consecutive rows
 * (a stripe, or the row range) needs the primary colour of the row just outside
 * it: d_halo holds those rows, [segment][2][W][3] doubles, [s][0] = the row
 * below segment s, [s][1] = the row above it, in the order rt_adaptive_halo_rows
 * lists them (rows outside the frame are never read; d_halo may be NULL when all
 * of them are).  Selection and results equal rt_launch_adaptive on the full frame
 * restricted to the shard's rows. */
int rt_launch_adaptive_shard(rt_scene* scene, const rt_render_params* p, const double* d_primary,
                             const double* d_halo, void* d_out, int subp, double threshold, rt_stats* stats,
                             long long* n_selected, void* stream);

/* Global rows the halo of rt_launch_adaptive_shard must hold: rows_out[2s] = the
 * row below segment s, rows_out[2s+1] = the row above it, -1 outside the frame.
 * Returns the entry count (2 x segments); rows_out may be NULL to query it. */
int rt_adaptive_halo_rows(const rt_render_params* p, int* rows_out, int cap);

/* The reference's whole launch_compute_image_device (mytracer_gpu.cu:44-113) in one synchronous
 * call: the primary pass (fp64, device scratch), the adaptive pass (subp, threshold: the reference
 * uses 4 and 0.02) and the copy of the final image into host_out (H x W x 3 of p->out_format; a
 * page-locked, device-mapped buffer is written directly).  Full frame only.  st_primary /
 * st_adaptive / n_selected optional.  Results equal rt_launch_compute_image (fp64) +
 * rt_launch_adaptive on device buffers. */
int rt_render_adaptive_to_host(rt_scene* scene, const rt_render_params* p, int subp, double threshold, void* host_out,
                               rt_stats* st_primary, rt_stats* st_adaptive, long long* n_selected);

/* Renders into a HOST buffer, synchronously (the reference's call pattern: Raytracer::
 * compute_image_cuda copies every frame back, mytracer.cpp:123-159).  A page-locked, device-mapped
 * buffer (hipHostMalloc, hipHostRegister, torch pin_memory) is written by the kernel directly over
 * PCIe as pixels finish; pageable memory goes through a device staging buffer kept by the scene
 * (allocated on first use, grown as needed, freed by rt_scene_free) and one copy. */
int rt_render_to_host(rt_scene* scene, const rt_render_params* p, void* host_out, rt_stats* stats);

/* Batched ray queries on the device scene: the caller's own rays through the
 * render path's hierarchy and fp64 triangle test -- picking, line of sight, range sampling.
 * The ray is Ray(o, d) of the renderer: d is normalised as its `normalize` does (v / |v| per
 * component, unchanged if |v| = 0) and t is the distance along the normalised direction.  A hit
 * counts iff 1e-5 < t < tmax (tmax = +inf: unbounded; t = DBL_MAX is never a hit, as on the CPU);
 * the closest hit is the smallest (t, reference slot), bit-identical to the CPU oracle's
 * closest_hit.  With rt_scene_set_analytic the spheres and planes are tested first, in the CPU's
 * order; a triangle must be strictly closer to replace them.  A ray with a non-finite component
 * in o or d, a zero-length d, a NaN tmax or tmax <= 1e-5 is a miss (not occluded) and is never
 * traversed. */
typedef struct rt_ray {
  double o[3];
  double d[3];
  double tmax;
  double reserved_;
} rt_ray;   /* 64 B */

/* Triangle hit: slot = the triangle's reference leaf slot (its index in the per-triangle arrays
 * of the uploaded rt_scene_soa: vertex_idx[3*slot..]), mesh = its mesh id, alpha / beta = the CPU's
 * Da/S and Db/S, normal = the face normal (RT_DRAW_FLAT) or alpha*vn0 + beta*vn1 + gamma*vn2,
 * gamma = 1 - alpha - beta, not renormalised (RT_DRAW_PHONG); prim = -1.
 * Analytic hit: slot = mesh = -1, prim = index (spheres, then planes), alpha = beta = 0, normal =
 * (p - c) / r or the plane normal.  Miss: t = +inf, slot = mesh = prim = -1, the rest 0. */
typedef struct rt_hit {
  double t;
  double alpha;
  double beta;
  double normal[3];
  int slot;
  int mesh;
  int prim;
  int reserved_;
} rt_hit;   /* 64 B */

/* Counters of one query: rays traced, rays that hit (closest) or were occluded, traversal-stack
 * entries spilled from the LDS ring to global memory, waves that tripped the kernel watchdog. */
typedef struct rt_query_stats {
  long long rays, hits, stack_spills, watchdog, reserved_[4];
} rt_query_stats;

/* d_hits[i] = the closest hit of d_rays[i], i in [0, n) (device buffers), on `stream`.
 * Asynchronous unless stats != NULL, in which case it synchronises the stream and fills *stats
 * (as rt_launch_compute_image).  n == 0 returns RT_OK without a launch.  Queries take no render
 * launch context: they may be in flight beside renders and beside each other on different streams
 * (a ring of 4 query contexts, allocated by the scene's first query).  RT_ERR_HIP on a scene whose
 * watchdog word is set (rt_scene_status). */
int rt_trace_closest(rt_scene* scene, const rt_ray* d_rays, long long n, rt_hit* d_hits, rt_query_stats* stats,
                     void* stream);

/* d_occluded[i] = 1 iff d_rays[i] has some hit with 1e-5 < t < tmax, else 0: an any-hit query
 * that stops at the first such hit (= "the closest hit has t < tmax").  An analytic primitive
 * that blocks the ray skips the hierarchy.  Otherwise as rt_trace_closest. */
int rt_trace_occluded(rt_scene* scene, const rt_ray* d_rays, long long n, unsigned char* d_occluded,
                      rt_query_stats* stats, void* stream);

/* Radiance of the caller's own rays: panoramas, fisheye or thin-lens cameras,
 * probes, re-shading the hit points of a query, sparse sampling.
 * d_rgb[3*i .. 3*i+2] = the colour trace() returns for ray i (what a pixel whose one primary ray
 * is d_rays[i] would hold), i in [0, n), clamped to 1 per channel, in p->out_format (device
 * buffers, 3 floats or 3 doubles per ray), on `stream`.  The render kernel itself shades them --
 * lights, shadows, mirrors to p->max_depth, textures, analytic primitives -- with the operations of
 * a frame launch: the rays of a camera (pixel (x, y): o = eye, d = lower_left + x x_dir + y y_dir -
 * eye) give that frame's bits.  A wave takes 64 consecutive rays, so the caller's ray order decides
 * their coherence (8x8 pixel tiles are the render's own order); results do not depend on it.
 *   The ray is Ray(o, d) as for the queries above: d is normalised by the renderer.  tmax bounds the
 * primary segment only: the ray hits iff 1e-5 < t < tmax (+inf or DBL_MAX: unbounded), else it
 * takes the background; shadow and reflection rays keep their own limits.  A degenerate ray
 * (non-finite component in o or d, zero-length d, NaN tmax or tmax <= 1e-5) is never traversed,
 * is not counted in primary_rays and gets the background colour.
 *   Read from p: the lights (inline, or lights_ext at any count up to RT_LIGHTS_LIMIT), max_depth,
 * background, ambience, out_format.  p->camera is ignored.  RT_ERR_INVALID, before any HIP call,
 * for: a NULL scene or p; n < 0; n > 0 with a NULL buffer; n > RT_RADIANCE_MAX_RAYS (the ray
 * index travels in 32 bits of path state, its work unit of 64 rays in 31); spp_n != 1; a row range
 * or stripes other than the defaults (row_begin = 0, row_end <= 0 or = camera.height, stripe_count
 * <= 1, stripe_index = 0); an unknown out_format; any flag but RT_FLAG_NATURAL_ORDER, which is accepted and changes
 * nothing.  n == 0 returns RT_OK without a launch and touches nothing.
 *   It is a render launch: it takes one of the scene's 8 launch contexts, copies its light table
 * with its control block, runs beside other launches on other streams under the rules of
 * rt_launch_compute_image, honours reserve_cus / blocks_per_cu / grid_spare (the persistent grid
 * is sized from ceil(n / 64) waves), is reported by rt_last_kernel_ms and rt_debug_last_grid, and
 * returns RT_ERR_HIP on a scene whose watchdog word is set.  It neither reads nor records tile
 * costs or orders: frame launches after it behave as if it had not happened.
 *   Asynchronous unless stats != NULL (then it synchronises the stream): primary_rays = the rays
 * traced (degenerate ones excluded), shadow_rays / reflection_rays as for renders, pixels = n,
 * the counter-variant fields 0. */
#define RT_RADIANCE_MAX_RAYS (1LL << 31)
int rt_trace_radiance(rt_scene* scene, const rt_render_params* p, const rt_ray* d_rays, long long n,
                      void* d_rgb, rt_stats* stats, void* stream);

/* Sorting caller-supplied rays into coherent waves.  rt_trace_closest,
 * rt_trace_occluded and rt_trace_radiance put 64 consecutive rays in a wave, so the caller's ray
 * order decides their speed.  rt_ray_order computes a coherence key per ray and the stable
 * ascending order of the keys as a permutation; rt_permute_rows applies a permutation to rays
 * (gather) and to result rows (scatter).  Results never depend on the order.
 *   The key of a ray, 32 bits, for origin_bits ob in [0, 10] (-1 = 5) and db = min(15, (31 - 3 ob) / 2)
 * direction bits: a degenerate ray (the queries' rule above) has RT_ORDER_KEY_DEGENERATE and sorts
 * last; every other key is morton3(origin cell) << (2 db) | morton2(direction cell) < 2^31, with
 * the origin cell floor((o - lo) / (hi - lo) * 2^ob) per axis, clamped to [0, 2^ob - 1] (0 on a flat
 * axis), in the box of rt_scene_bounds, and the direction cell floor((p * 0.5 + 0.5) * 2^db), clamped to
 * 2^db - 1, of the octahedral map p of d (csrc/device/rt_order_key.hpp is the definition). */
#define RT_ORDER_MAX_RAYS (1LL << 31)
#define RT_ORDER_KEY_DEGENERATE 0x80000000u
/* The sort's tile: a block of rt_ray_order's sort owns a contiguous run of whole tiles of this
 * many keys. */
#define RT_ORDER_TILE 1024

/* The box the keys quantise origins in: the scene's root box (the reference root's bounds
 * widened by the layout's delta, what the kernels' entry test uses); zeros for a scene
 * without triangles. */
int rt_scene_bounds(const rt_scene* scene, double lo[3], double hi[3]);

/* Pure host, no HIP call: bytes of d_workspace rt_ray_order needs for n rays
 * (0 for n <= 0; non-decreasing in n):
 *   3 * roundup(4 n, 256) + 4 * 256 * 1024
 * = two key buffers and one index buffer (the sort's ping-pong; d_perm is the other index buffer)
 * and the [digit][block] count table of at most 1024 blocks. */
size_t rt_ray_order_workspace_bytes(long long n);

/* Pure host, no HIP call, no scene: keys[i] of rays[i] (HOST pointers) in box [lo, hi].
 * The same function text the device runs. */
int rt_ray_keys_host(const double lo[3], const double hi[3], const rt_ray* rays, long long n,
                     int origin_bits, unsigned int* keys);

/* d_perm[j] = index of the ray that belongs at position j:
 * the stable ascending order of the rays' keys.
 * d_keys (optional, may be NULL): d_keys[i] = key of d_rays[i].
 * Asynchronous on `stream`.
 * No allocation, no host synchronisation and no scene state is touched.
 * All scratch is the caller's d_workspace (rt_ray_order_workspace_bytes(n) bytes, 256-B aligned).
 * Calls with different workspaces may therefore be in flight on different streams,
 * beside renders and queries.
 * n == 0: RT_OK, no launch.
 * RT_ERR_INVALID, before any HIP call, for: a NULL scene; n < 0; n > RT_ORDER_MAX_RAYS; n > 0 with
 * a NULL d_rays, d_perm or d_workspace; origin_bits outside [-1, 10]; n > 0 with a misaligned workspace.
 * RT_ERR_HIP on a scene whose watchdog word is set (rt_scene_status). */
int rt_ray_order(rt_scene* scene, const rt_ray* d_rays, long long n, int origin_bits,
                 unsigned int* d_perm, unsigned int* d_keys, void* d_workspace, void* stream);

/* inverse == 0 (gather):  dst row j       = src row perm[j].
 * inverse != 0 (scatter): dst row perm[j] = src row j.
 * j in [0, n); rows of row_bytes bytes, 1..256.
 * An entry perm[j] >= n is skipped: nothing is read or written for it.
 * Asynchronous on `stream` of `device`.
 * d_src / d_dst must not overlap.
 * Both must be aligned to the largest power of two <= 16 that divides row_bytes.
 * RT_ERR_INVALID, before any HIP call, for: n < 0 or n > 2^32; row_bytes outside [1, 256]; a
 * negative device; n > 0 with a NULL, misaligned or overlapping buffer.  n == 0: RT_OK, no launch. */
int rt_permute_rows(const void* d_src, void* d_dst, const unsigned int* d_perm, long long n,
                    int row_bytes, int inverse, int device, void* stream);

/* Test hook in the style of the other rt_debug_* calls: caps the blocks of rt_ray_order's
 * kernels on this scene (0 = default), so that a few thousand rays exercise blocks that own
 * several tiles.  Never changes a result. */
int rt_debug_set_order_grid(rt_scene* scene, int max_blocks);

/* Occlusion fans generated on the device: ambient occlusion, sky-view factor,
 * hemispherical visibility.  rt_trace_ao traces k occlusion rays from each of n surface points and
 * returns, per point, how many of them are NOT occluded; the rays exist only in registers, and no
 * per-ray result is written.
 *   A point is an rt_ray record: o = the surface point p, d = its normal nrm (any length > 0),
 * tmax = the occlusion radius (+inf or DBL_MAX: unbounded).  A point is degenerate by the queries'
 * rule: a non-finite component in o or d, dot(d, d) > 0 false, or tmax > 1e-5 false.
 *   Fan ray s in [0, k) of a non-degenerate point i (csrc/device/rt_ao_fan.hpp is the definition;
 * fp64, + - * / sqrt only, no contraction, so host and device agree bit for bit):
 *     N = nrm / sqrt(dot(nrm, nrm))                    (the renderer's normalize)
 *     sg = N.z >= 0 ? 1 : -1,  a = -1 / (sg + N.z),  b = N.x * N.y * a
 *     T = (1 + sg * N.x * N.x * a, sg * b, -sg * N.x)     (the frame of Duff et al.)
 *     B = (b, sg + N.y * N.y * a, -N.y)
 *     set = hash((uint32_t)i ^ seed) % n_sets,  hash = the 32-bit mixer written out in the header
 *     (lx, ly, lz) = d_dirs[(set * k + s) * 3 ..]      (the caller's local direction, z along N)
 *     w = (lx * T + ly * B) + lz * N,  origin = p + bias * N          (per component)
 * and the ray is Ray(origin, w) with the point's tmax, normalised and traced exactly as
 * rt_trace_occluded would.  A degenerate point's fan rays are Ray(o, (0, 0, 0)): degenerate rays,
 * never traversed and not occluded.  A local direction that makes w zero or non-finite gives such a
 * ray too; nothing is clamped or rejected per direction. */
#define RT_AO_MAX_SAMPLES 1024
#define RT_AO_MAX_SETS 65536
#define RT_AO_MAX_POINTS (1LL << 31)
typedef struct rt_ao_params {
  int k;              /* fan rays per point, 1..RT_AO_MAX_SAMPLES */
  int n_sets;         /* direction sets, 1..RT_AO_MAX_SETS */
  unsigned int seed;  /* picks each point's set */
  int reserved_;
  double bias;        /* finite; origin = p + bias * N */
  const double* d_dirs; /* DEVICE, [n_sets][k][3] local directions, caller-owned */
} rt_ao_params;

/* d_unoccluded[i] = the number of point i's k fan rays that rt_trace_occluded reports as 0, i in
 * [0, n) (device buffers), on `stream`:
 *     d_unoccluded[i] == k - sum over s of occluded(rays[i * k + s]),  rays = rt_ao_rays_host's,
 * for every point; a degenerate one reports k.  Asynchronous unless stats != NULL (then it
 * synchronises the stream): rays = n * k, hits = the occluded fan rays, stack_spills and watchdog
 * as for the queries.  It takes one of the scene's query contexts, so it may be in flight beside
 * renders and queries on other streams; it allocates nothing beyond the contexts' first-use
 * allocation and touches no scene state.  When 64 is not a multiple of k the counts are summed
 * with integer atomics and the call zeroes d_unoccluded[0..n) on the stream first.  n == 0 returns
 * RT_OK without a launch and touches nothing.
 *   RT_ERR_INVALID, before any HIP call, for: a NULL scene or params; n < 0 or n >
 * RT_AO_MAX_POINTS; k or n_sets out of range; a non-finite bias; n > 0 with a NULL d_points,
 * d_dirs or d_unoccluded.  RT_ERR_HIP on a scene whose watchdog word is set (rt_scene_status). */
int rt_trace_ao(rt_scene* scene, const rt_ray* d_points, long long n, const rt_ao_params* params,
                unsigned int* d_unoccluded, rt_query_stats* stats, void* stream);

/* Pure host, no HIP call, no scene: rays_out[i * k + s] = fan ray s of points[i] (HOST pointers,
 * params->d_dirs a HOST pointer here), tmax = the point's, reserved_ = 0.  The same function text
 * the device runs and the same argument checks. */
int rt_ao_rays_host(const rt_ray* points, long long n, const rt_ao_params* params, rt_ray* rays_out);

/* Mean radiance of device-generated fans: light baking, irradiance probes, final
 * gathering.  From each of n surface points the call traces the k fan rays of rt_trace_ao's
 * definition above -- the same point records, the same rt_ao_params (k, n_sets, seed, bias, the
 * device table d_dirs), built in registers by the same header text -- shades each one with the
 * full render path, as rt_trace_radiance shades a caller's ray, and stores one mean colour per
 * point; no ray and no per-ray colour is written.  The definition is compositional:
 *     d_rgb[3*i + c] = (sum over s = 0 .. k-1 of R[i*k + s][c]) / (double)k
 * where R is the RT_OUT_RGB_F64 result of rt_trace_radiance(scene, p, rt_ao_rays_host(points,
 * fan), n * k, ...), the sum is taken in fp64 from +0.0 in increasing s, one addition per sample
 * (no contraction, no pairwise order), followed by one fp64 division per channel; RT_OUT_RGB_F32
 * stores (float) of that quotient.  The result equals that written-out computation bit for bit.
 *   The mean is CLAMPED PER SAMPLE: each fan ray's colour is clamped to 1 per channel before it is
 * added, which is what rt_trace_radiance returns for it.  An unclamped (HDR) sum and per-direction
 * weights are not built.  A degenerate fan ray -- its point is degenerate, or the direction w is
 * zero or non-finite -- contributes min(background, 1) and is not counted in primary_rays.  The
 * point's tmax bounds each fan ray's primary segment only.
 *   Read from p what rt_trace_radiance reads: the lights (inline or lights_ext), max_depth,
 * background, ambience, out_format; p->camera is ignored.  RT_ERR_INVALID, before any HIP call,
 * for everything rt_trace_radiance rejects about p (spp_n != 1, a row range or stripes, an unknown
 * out_format, any flag but RT_FLAG_NATURAL_ORDER) and everything rt_trace_ao rejects about n, fan
 * and the buffers (n < 0, n > RT_AO_MAX_POINTS, k or n_sets out of range, a non-finite bias, n > 0
 * with a NULL d_points, d_dirs or d_rgb).  n == 0 returns RT_OK without a launch and touches
 * nothing.  RT_ERR_HIP on a scene whose watchdog word is set.
 *   It is a render launch, as rt_trace_radiance is: one of the scene's 8 launch contexts, the light
 * table copied with the control block, reserve_cus / blocks_per_cu / grid_spare and the half-grid
 * rule honoured (the persistent grid is sized from the lanes in use: a point's rays run on G =
 * the largest power of two <= min(k, 32) neighbouring lanes, ceil(k / G) chunks of them), reported
 * by rt_last_kernel_ms and rt_debug_last_grid; it neither reads nor records tile costs or orders.
 *   Asynchronous unless stats != NULL (then it synchronises the stream): primary_rays = the fan
 * rays traced (degenerate ones excluded), shadow_rays / reflection_rays as for renders -- all three
 * equal the written-out rt_trace_radiance call's -- pixels = n, the counter-variant fields 0. */
int rt_trace_gather(rt_scene* scene, const rt_render_params* p, const rt_ray* d_points, long long n,
                    const rt_ao_params* fan, void* d_rgb, rt_stats* stats, void* stream);

/* A camera's closest hits and surface points made on the device: the G-buffer of a
 * frame -- depth, normal, mesh id, hit point per pixel -- and the point records rt_trace_ao and
 * rt_trace_gather start from, without a ray or a hit written out in between.  rt_trace_camera
 * builds each pixel's primary ray in registers, finds its closest hit as rt_trace_closest does and
 * stores, per pixel, the rt_hit, the surface-point record, or both; it reads nothing per pixel.
 *   The ray of pixel (x, y) (csrc/device/rt_camera_point.hpp is the definition; fp64, + - * / sqrt
 * only, no contraction, so host and device agree bit for bit):
 *     o = eye,  d = ((lower_left + x * x_dir) + y * y_dir) - eye       (per component, unnormalised)
 * with tmax = +inf and reserved_ = 0: the render kernel's primary ray at spp_n = 1.
 *   The surface point of a ray and its rt_hit; the hit counts iff hit.t < +inf:
 *     rd = d / sqrt(dot(d, d))                                          (the renderer's normalize)
 *     p = o + hit.t * rd,  n = hit.normal, negated if n.x * d.x + n.y * d.y + n.z * d.z > 0
 * (the normal faces the ray's origin), and the record is {o = p, d = n, tmax = point_tmax,
 * reserved_ = 0}.  A miss gives {o = the ray's o, d = (0, 0, 0), tmax = point_tmax, reserved_ = 0}: a
 * degenerate point, which rt_trace_ao reports as fully open and rt_trace_gather as background.
 *   Read from p: camera, row_begin, row_end, stripe_height, stripe_count, stripe_index.  The shard's
 * rows are rt_launch_compute_image's, packed in increasing y (rt_rows_in_shard(p) of them); n = rows
 * x width records.  Lights, depth, colours and out_format are ignored.
 *   Order of the records: RT_CAMERA_ROW_MAJOR puts pixel (x, local row r) at record r * width + x,
 * the frame's own layout.  RT_CAMERA_TILE_MAJOR walks the tiles of rt_tile_shape (8 x 8) over the
 * shard's packed rows, tile rows from the bottom, tiles left to right, a tile's pixels row-major
 * and consecutive; the partial tiles at the right and top edges hold only the pixels they have, so
 * there are still exactly n records and no padding.  Tile order is the coherent order for whatever
 * traces from these points next.
 *   The definition is compositional: with rays = rt_camera_rays_host(p, order), d_hits equals
 * rt_trace_closest(rays) bit for bit (analytic primitives of rt_scene_set_analytic included) and
 * d_points equals rt_surface_points_host(rays, those hits, n, point_tmax) bit for bit. */
enum { RT_CAMERA_ROW_MAJOR = 0, RT_CAMERA_TILE_MAJOR = 1 };
#define RT_CAMERA_MAX_PIXELS (1LL << 31)
typedef struct rt_camera_out {
  rt_hit* d_hits;      /* DEVICE, optional: the closest hit per pixel */
  rt_ray* d_points;    /* DEVICE, optional: the surface-point record per pixel (rt_trace_ao / rt_trace_gather input) */
  int order;           /* RT_CAMERA_* */
  int reserved_;
  double point_tmax;   /* tmax written into every point record (+inf: unbounded fans) */
} rt_camera_out;

/* Fills out->d_hits and / or out->d_points (n records each, device buffers) on `stream`.  It takes
 * one of the scene's query contexts, as rt_trace_ao does -- it is not a render launch -- so it may be
 * in flight beside renders and queries on other streams; it allocates nothing beyond the contexts'
 * first-use allocation and touches no scene or cost-order state.  Asynchronous unless stats != NULL
 * (then it synchronises the stream): rays = n, hits = the pixels that hit, stack_spills and
 * watchdog as for the queries.
 *   RT_ERR_INVALID, before any HIP call, for: a NULL scene, p or out; both output pointers NULL; an
 * unknown order; spp_n != 1; any flag but RT_FLAG_NATURAL_ORDER, which is accepted and changes
 * nothing; whatever rt_launch_compute_image rejects about the camera size, the row range and the
 * stripes (a row range combined with stripe_count > 1 included); n > RT_CAMERA_MAX_PIXELS; d_points
 * != NULL with point_tmax > 1e-5 false (NaN included).  RT_ERR_HIP on a scene whose watchdog word is
 * set (rt_scene_status). */
int rt_trace_camera(rt_scene* scene, const rt_render_params* p, const rt_camera_out* out, rt_query_stats* stats,
                    void* stream);

/* Pure host, no HIP call, no scene: rays_out[0..n) = the shard's primary rays in `order` (a HOST
 * pointer), the same function text the device runs and the same checks of p and order. */
int rt_camera_rays_host(const rt_render_params* p, int order, rt_ray* rays_out);

/* Pure host, no HIP call, no scene: points_out[i] = the surface-point record of rays[i] and hits[i]
 * (HOST pointers), i in [0, n), the same function text the device runs.  n == 0 is accepted;
 * RT_ERR_INVALID for n < 0, n > RT_CAMERA_MAX_PIXELS, point_tmax > 1e-5 false, and a NULL buffer
 * with n > 0. */
int rt_surface_points_host(const rt_ray* rays, const rt_hit* hits, long long n, double point_tmax,
                           rt_ray* points_out);

/* The k nearest hits of each ray, resumable past k: the hits behind the first one
 * -- thickness sampling, counting the surfaces a ray crosses, picking through a pane, depth
 * peeling, every wall between two points -- without re-tracing from pushed origins.
 *   The definition does not depend on the hierarchy.  The ray is normalised and judged degenerate
 * exactly as for rt_trace_closest.  Its hit list H is every reference slot whose triangle the CPU's
 * intersect_triangle accepts with 1e-5 < t < tmax (t = DBL_MAX is never a hit), each slot once,
 * however many device records an SBVH made of it, sorted ascending by (t, slot).  With d_after,
 * only the entries with t > after.t || (t == after.t && slot > after.slot) belong to H: {-inf, -1}
 * is no constraint, a NaN after.t empties the list by that comparison (nothing is special-cased),
 * reserved_ is ignored.
 *   d_count[i] = min(|H|, k).  d_hits[i*k + j], j < d_count[i], is the rt_hit of H[j] with the
 * fields and bits rt_trace_closest would give that triangle (t, alpha, beta, normal by draw mode,
 * slot, mesh, prim = -1); the rows j >= d_count[i] are the miss record: the whole buffer is
 * defined.  d_count[i] == k means the list may go on: resume with d_after[i] = {t, slot} of the
 * last entry; a resumed call on an exhausted list returns count 0.  There is deliberately no
 * "more" flag: an exact one would forbid pruning at the k-th hit.  So k = 1 without d_after equals
 * rt_trace_closest on all 64 bytes of every row, and the concatenation of resumed rounds at any k
 * equals H.
 *   RT_ERR_INVALID, before any HIP call, for: a NULL scene; n < 0; k outside [1, RT_HITS_MAX_K];
 * n * k > RT_HITS_MAX_ROWS; n > 0 with a NULL d_rays, d_hits or d_count.  n == 0 returns RT_OK
 * without a launch and touches nothing.  RT_ERR_UNSUPPORTED on a scene that holds analytic
 * primitives (rt_scene_set_analytic with n > 0): a sphere has a second intersection that neither
 * the reference nor the oracle defines.  RT_ERR_HIP on a scene whose watchdog word is set.
 *   It takes a query context, as rt_trace_closest does: it runs beside renders and other queries
 * on other streams, follows scene updates in stream order and allocates nothing beyond the
 * contexts' first-use allocation.  Asynchronous unless stats != NULL: rays = n, hits = the sum of
 * the counts, stack_spills and watchdog as for the queries. */
#define RT_HITS_MAX_K 8
#define RT_HITS_MAX_ROWS (1LL << 31)             /* n * k */
typedef struct rt_hit_key { double t; int slot; int reserved_; } rt_hit_key;   /* 16 B */
int rt_trace_hits(rt_scene* scene, const rt_ray* d_rays, long long n, int k,
                  const rt_hit_key* d_after,      /* DEVICE [n], optional (NULL: none) */
                  rt_hit* d_hits,                 /* DEVICE [n][k] */
                  unsigned int* d_count,          /* DEVICE [n] */
                  rt_query_stats* stats, void* stream);

/* Moving geometry: new vertex positions and normals on the uploaded topology, the
 * device hierarchy refitted on the GPU -- a door that opens, a character that walks, a mesh that
 * deforms -- without rt_scene_free + rt_scene_upload_ex and their host build.  The three arrays are
 * those of the rt_scene_soa the scene was uploaded from, with new values: rt_host_update_vertices
 * (rt_host.h) makes them.
 *   The definition is compositional: after the call every launch and query on the scene returns,
 * bit for bit, what it returns on a scene freshly uploaded with the same options from the original
 * rt_scene_soa with these three arrays replaced and the same reference tree with refitted boxes
 * (frames, adaptive passes, rt_trace_closest / occluded / radiance / ao / gather / camera, the ray
 * counts of rt_stats).  Indices, uvs, texels, materials, analytic primitives and the slot numbering
 * are unchanged.  The device hierarchy keeps its topology and gets new boxes: a leaf slot the exact
 * bounds of its whole triangles (under RT_TREE_SBVH larger than the clipped pieces of the upload,
 * but conservative), an internal slot the union of its child node's slots, all grown by the new
 * delta = 2^-20 max|vertex| and rounded outward as at upload.  No child reference is written.
 *   Which tree to upload a scene that will move with (measured): RT_TREE_SAH.  Its
 * refitted boxes render as fast as a fresh RT_TREE_SAH upload of the moved scene.  The un-clipped
 * leaves of the default RT_TREE_SBVH cost the office proxy a factor of 29 to 39 per frame at every
 * displacement, 1.4 in a room with few spatial splits; results are correct either way.
 *   An RT_TREE_SBVH scene that is already uploaded, or one that moves little, keeps its clipped
 * leaves with rt_scene_update_vertices_ex and RT_UPDATE_RECLIP below (measured, DESIGN.md §25: the
 * office frame after the update within 1.03 of a fresh upload's at a displacement of 0.01 of the
 * box diagonal and faster than the refitted RT_TREE_SAH tree's, 1.5 to 1.8 at 0.1 and 0.3, where at
 * 0.1 the refitted RT_TREE_SAH tree is the faster of the two; a plain update of an RT_TREE_SBVH
 * scene is never the better choice). */
typedef struct rt_scene_update {
  long long n_vertices;          /* must equal the uploaded scene's */
  long long n_triangles;         /* must equal the uploaded scene's */
  const double* vertex_pos;      /* HOST [3*n_vertices] */
  const double* vertex_normals;  /* HOST [3*n_vertices] */
  const double* face_normals;    /* HOST [3*n_triangles], leaf order of the uploaded rt_scene_soa */
  long long reserved_[3];
} rt_scene_update;

/* Host part, synchronous and before any HIP call: RT_ERR_INVALID for a NULL scene, u or array, or a
 * count that differs from the scene's; RT_ERR_UNSUPPORTED for max|vertex| above RT_MAX_COORDINATE
 * (rt_scene_upload's rule; NaN coordinates are not looked for, their triangles enter no box and are
 * never hit), the scene left exactly as it was; RT_ERR_HIP on a scene whose watchdog word is set.  A
 * scene without triangles returns RT_OK without a launch.  The scene's delta and root box switch at
 * the call: launches copy them by value, so a launch issued after the call returns sees the new
 * ones, and rt_scene_bounds and the keys of rt_ray_order follow the new box (the bounds of the
 * vertices the triangles reference, grown by delta).
 *   Device part, asynchronous, on the stream a render launch given this `stream` would use
 * (rt_upload_options.reserve_cus: the caller's CU-masked stream, joined to `stream` by events): the
 * three arrays are copied -- the host arrays may be reused when the call returns --, one kernel
 * rewrites the triangle and normal records, and one kernel per height of the 4-wide tree refits
 * the boxes, leaf-only nodes first.  Stream order orders the update against launches on the same
 * stream.  Launches issued earlier on OTHER streams must have finished before the call: the caller
 * ensures it, it is not checked.  Calls on one scene must come from one host thread at a time.
 *   The scene's first call allocates device copies of the three arrays and the refit schedule (it
 * reads the node references and the records' vertex ids back once): rt_scene_device_bytes grows
 * then and only then.  A scene that is never updated costs what it did before this call existed.
 *   Not built: RT_FLAG_TRAVERSAL_STATS on a scene that has been updated returns RT_ERR_UNSUPPORTED
 * (the canonical counters are the oracle's walk of the median-split tree of the current geometry;
 * a refitted tree is another tree, so the 2-wide nodes are not refitted; RT_FLAG_WIDE_STATS keeps
 * working); topology changes (triangles added or removed); a rebuild when the refitted boxes'
 * quality decays; an rt_multi wrapper (each rt_scene of rt_scene_upload_multi can be updated on its
 * own). */
int rt_scene_update_vertices(rt_scene* scene, const rt_scene_update* u, void* stream);

/* rt_scene_update_vertices with flags.  flags == 0 is that call exactly; a bit other
 * than RT_UPDATE_RECLIP returns RT_ERR_INVALID before any HIP call.
 *   RT_UPDATE_RECLIP keeps the clipped leaves of an RT_TREE_SBVH scene through the update.  The
 * upload remembers, per device record, the region its spatial splits cut the record to (the regions of
 * one triangle's records together cover all of space).  The refit bounds each cut record by the
 * part of its moved triangle inside that region -- bounds(triangle), intersected per plane of the
 * region with the bounds of the triangle's part on that side, in fp64 -- instead of by the whole
 * triangle; a leaf slot whose triangles all left their regions gets the empty box [+inf, -inf],
 * which no ray enters.  Everything else is rt_scene_update_vertices: the compositional definition
 * above holds bit for bit, plain and re-clipping updates may alternate (every box is recomputed
 * from the positions each time), RT_FLAG_TRAVERSAL_STATS stays refused.  The planes stay where the
 * uploaded geometry put them: nothing is re-split.
 *   On a scene without cut records (RT_TREE_SAH, RT_TREE_REFERENCE, an RT_TREE_SBVH build that
 * duplicated no reference) the flag is accepted and the plain refit runs.  The scene's first
 * re-clipping update copies the table to the device and rt_scene_device_bytes grows by
 * 4 * records + 48 * cut records bytes, then and only then; a scene never re-clipped allocates
 * nothing for it. */
enum { RT_UPDATE_RECLIP = 1 };
int rt_scene_update_vertices_ex(rt_scene* scene, const rt_scene_update* u, unsigned flags, void* stream);

/* Pure host, no HIP call: the clip regions of the device records rt_scene_upload_ex builds from
 * these arguments (opt NULL: the defaults).  Returns the record count, or an RT_ERR_* code; writes
 * the first min(records, cap) rows: clip_out[6 * g ..] = lo xyz, hi xyz of record g (-inf / +inf where
 * uncut), slot_out[g] = the reference slot of the record's triangle. */
long long rt_debug_clip_regions(const rt_scene_soa* soa, const rt_bvh_soa* bvh, const rt_upload_options* opt,
                                double* clip_out, int* slot_out, long long cap);

/* Pure host: the fp64 box the re-clipping refit gives triangle (p0, p1, p2) in region clip (lo xyz,
 * hi xyz), the function text the device runs.  1: non-empty, lo / hi written; 0: empty; RT_ERR_INVALID
 * for a NULL pointer. */
int rt_reclip_box_host(const double p0[3], const double p1[3], const double p2[3], const double clip[6],
                       double lo[3], double hi[3]);

/* Moving a scene by positions alone: the face normals, the angle-weighted vertex
 * normals, max|vertex| and the root box are made by kernels, from a HOST or a DEVICE array.
 *
 * rt_scene_set_triangle_order comes first, once per scene.  A vertex's normal sums its corners in
 * the mesh's original triangle order, corner 0, 1, 2 within a triangle, and the uploaded scene
 * holds its triangles in leaf-slot order: slot_triangle[slot] = the triangle's index in the
 * original order (rt_host_slot_triangles, rt_host.h).  Host part: RT_ERR_INVALID for a NULL
 * pointer, an array that is not a permutation of [0, n_triangles) or a count other than the
 * scene's; RT_ERR_UNSUPPORTED where 3 * n_triangles does not fit a signed 32-bit corner index.  It
 * reads every slot's vertex ids back from the device records and builds, on the device, the
 * per-slot ids (16 B per slot), a CSR of every vertex's corners (slot, corner) sorted by
 * (slot_triangle[slot], corner) -- 4 B per vertex + 4, 4 B per corner; a triangle that names a
 * vertex twice contributes two entries -- and the corner weights (32 B per slot):
 * rt_scene_device_bytes grows by 60 * n_triangles + 4 * (n_vertices + 1) bytes, at this call and
 * only here (by nothing for a scene without triangles); a scene that never calls it costs what it
 * did before.  Calling it again replaces the tables (after a device synchronisation). */
int rt_scene_set_triangle_order(rt_scene* scene, const int* slot_triangle, long long n_triangles);

typedef struct rt_scene_positions {
  long long n_vertices;        /* must equal the uploaded scene's */
  const double* vertex_pos;    /* [3*n_vertices], global vertex order */
  int on_device;               /* 0: HOST pointer; 1: DEVICE pointer on the scene's device */
  int reserved_;
  long long reserved2_[3];
} rt_scene_positions;

/* The definition is compositional: the call has the effect of rt_host_update_vertices (rt_host.h)
 * with these positions on the host scene this scene was uploaded from, followed by
 * rt_scene_update_vertices_ex(scene, that scene's three arrays, flags, stream).  For finite
 * positions this holds bit for bit: the 4-wide nodes, the triangle and the normal records
 * (rt_debug_scene_image), delta, rt_scene_bounds and every frame, query and ray count afterwards.
 * The normals are rt_normals.hpp's text, the one HostMesh::compute_normals runs, in fp64 + - * /
 * sqrt with contraction off.  Positions that hold a NaN are outside the bit-for-bit contract (the
 * payload of a generated NaN differs between host and GPU); they neither fault nor hang and are not
 * looked for, as at upload.  flags: 0 or RT_UPDATE_RECLIP.  The two update calls may alternate in
 * any order on one scene; RT_FLAG_TRAVERSAL_STATS stays refused after either.
 *   Checks, before any HIP call: RT_ERR_INVALID for a NULL scene, struct or pointer, an on_device
 * other than 0 or 1, a count other than the scene's, an unknown flag, or a scene that has had no
 * rt_scene_set_triangle_order call; RT_ERR_HIP on a scene whose watchdog word is set.  A scene
 * without triangles returns RT_OK without a launch (from a device pointer also without reading it:
 * its delta stays).
 *   on_device = 0: max|vertex|, the RT_ERR_UNSUPPORTED check (RT_MAX_COORDINATE) and the root box
 * are taken on the host exactly as rt_scene_update_vertices_ex takes them, the positions are copied
 * with one hipMemcpyAsync, and there is no host synchronisation: the array may be reused when the
 * call returns, and updates and renders can be queued back to back on one stream.
 *   on_device = 1: a reduction kernel reads the caller's buffer in stream order and writes
 * max|vertex| over all 3 * n_vertices values and the box of the referenced vertices to page-locked
 * host memory of the scene.  THE CALL THEN WAITS FOR THAT STREAM, ONCE -- its one synchronisation --,
 * applies the RT_MAX_COORDINATE check (on refusal the scene is exactly as it was: nothing of it has
 * been written by then), switches delta and the root box and issues the rest asynchronously.  The
 * buffer may be overwritten once the work issued on `stream` has finished.  The scene's first such
 * call copies the referenced vertex ids to the device and allocates the block partials:
 * rt_scene_device_bytes grows by 4 * referenced vertices + 14336 bytes, then and only then.
 *   Device part: face_normals_kernel (one thread per slot), vertex_normals_kernel (one per vertex),
 * then the record and refit kernels of rt_scene_update_vertices, unchanged.  The stream rules and the
 * first-use allocations are those of rt_scene_update_vertices, the CU-masked stream of
 * rt_upload_options.reserve_cus included.
 *   Not built: a synchronisation-free device-pointer variant (it needs caller-supplied bounds, or
 * launches that read delta from memory); an rt_multi wrapper; topology changes; keeping the host
 * scene in step -- the rt_host_scene, and an oracle made from it, still see the old positions. */
int rt_scene_update_positions(rt_scene* scene, const rt_scene_positions* positions, unsigned flags, void* stream);

/* Pure host, no HIP call and no scene: the normals rt_scene_update_positions makes, by the same CSR
 * build and the same per-thread bodies.  vertex_idx [3 * n_triangles] in leaf order
 * (rt_scene_soa.vertex_idx), slot_triangle as above, vertex_pos [3 * n_vertices];
 * vertex_normals_out [3 * n_vertices], face_normals_out [3 * n_triangles] in leaf order.
 * RT_ERR_INVALID for a NULL pointer, a negative count, a non-permutation or a vertex id out of
 * range. */
int rt_normals_host(const int* vertex_idx, const int* slot_triangle, long long n_vertices, long long n_triangles,
                    const double* vertex_pos, double* vertex_normals_out, double* face_normals_out);

/* Test hook in the style of rt_debug_counters: copies a device array of the scene's layout into
 * out[0 .. min(bytes, size)) -- RT_IMAGE_NODES4: the 4-wide nodes (128 B each: lo / hi of x, y, z
 * for 4 slots as fp32, 4 refs, 4 pad words), RT_IMAGE_TRIS: the triangle records (80 B each),
 * RT_IMAGE_TNORM: the normal records (12 doubles each) -- and returns the bytes the array holds
 * (out may be NULL with bytes = 0 to ask for it).  Synchronises the device. */
enum { RT_IMAGE_NODES4 = 0, RT_IMAGE_TRIS = 1, RT_IMAGE_TNORM = 2 };
long long rt_debug_scene_image(rt_scene* scene, int what, void* out, long long bytes);

/* Cross-process access to a device buffer, for one process per GPU (the frame-assembly mode
 * RT_FLAG_GLOBAL_ROWS: every rank writes its stripes straight into rank 0's frame buffer).
 * rt_ipc_get_handle exports the device allocation that holds d_ptr (an RT_IPC_HANDLE_BYTES-byte
 * handle, plain bytes to send to the other processes) and d_ptr's byte offset in it.  Another
 * process maps it with rt_ipc_open, with its own `device` current and the exporter's device id as
 * this process numbers it (`owner_device`, -1 = unknown: then the mapping's lazy peer access only):
 * peer access from `device` to `owner_device` is checked and enabled, and the call returns a pointer
 * to the same bytes; rt_ipc_close(ptr, offset) unmaps it.  The
 * exporting process must keep the allocation alive while it is mapped elsewhere. */
#define RT_IPC_HANDLE_BYTES 64
int rt_ipc_get_handle(const void* d_ptr, unsigned char* handle, unsigned long long* offset);
int rt_ipc_open(const unsigned char* handle, unsigned long long offset, int device, int owner_device, void** d_ptr);
int rt_ipc_close(void* d_ptr, unsigned long long offset);

/* Milliseconds of the last launch on this scene, measured with hipEvents
 * recorded around the kernel on its stream (waits for it).  Returns RT_ERR_HIP when a launch on
 * the scene tripped the kernel watchdog (rt_scene_status). */
int rt_last_kernel_ms(rt_scene* scene, float* ms);

/* RT_OK, or RT_ERR_HIP once any finished launch on this scene tripped a kernel watchdog (a
 * traversal loop that ran past its iteration bound: a cyclic or corrupt hierarchy, or a kernel
 * bug).  The kernel mirrors the flag into page-locked host memory, so launches without stats
 * report it too: from then on every launch on the scene, rt_last_kernel_ms and this call return
 * RT_ERR_HIP (sticky; the scene's results are void -- free it and upload again).  Replaces the
 * reference's CHECK-and-continue (common/common.h:6-15).  Does not synchronise. */
int rt_scene_status(const rt_scene* scene);

/* Diagnostics: raw device counter words of the last launch (synchronises the
 * device).  Words [8,16) = rt_stats order (from node_visits on: STATS flags only;
 * the ray counts [8,11) are the kernel's per-wave slots, summed here); with a STATS flag, words [16,30) =
 * node-loop iterations / active lanes, leaf-loop iterations / active lanes,
 * traverse / shade / refill cycles (s_memtime), outer iterations, traversal
 * rounds / active lanes (per wave, summed), traversal-stack entries spilled
 * from the LDS ring to global memory, distinct nodes / triangle lines per
 * wave-level node / leaf iteration (summed), triangle tests in leaves of > 4,
 * node iterations served from the LDS treelet; word 31 = watchdog flag; words
 * [32,35) = global-node iterations with one node for the whole wave, distinct
 * nodes of global-node iterations (summed), leaf iterations with one record;
 * words 35, 36 = any-hit triangle tests and those of the ray's own record (STATS
 * flags); word 37 = shadow_rays_skipped, every launch: the shadow rays (counted
 * in word 9) whose light faces away from a surface of a material with shininess
 * > 0 and finite coefficients, all light colours finite, so that their light term
 * is exactly 0 -- not traced by the production kernels; with a STATS or timeline
 * flag they are traced and only counted; word 39 = internal; words 40, 41 (4-wide STATS flag) =
 * wave-level node iterations in which some active lane's stack ring had fewer than three free
 * entries (the pushes take the path that can spill), and those that popped while some active
 * lane had entries in the spill array.
 * Returns the number of words copied (at most 42). */
int rt_debug_counters(rt_scene* scene, unsigned long long* out, int n);

/* Diagnostics: per-wave timeline of the last launch with a STATS flag: words
 * [4w, 4w+4) of wave w of the persistent grid = {start, last successful work
 * fetch, end} (s_memrealtime, 100 MHz) and pixels fetched; waves that were not
 * launched keep stale words.  Synchronises the device; returns words copied. */
long long rt_debug_wave_log(rt_scene* scene, unsigned long long* out, long long n);

/* Diagnostics: persistent-grid blocks per CU of kernel variant 0 (production), 1 (4-wide
 * STATS), 2 (2-wide canonical STATS), 3 (timeline), 4 (production, 16-entry stack ring), 5 / 6
 * (0 / 4 with sample groups, spp > 1), 7 / 8 (0 / 4 over a ray list, rt_trace_radiance), 9 / 10
 * (7 / 8 over surface points with fans, rt_trace_gather), as the launches use it. */
int rt_debug_blocks_per_cu(rt_scene* scene, int variant);

/* Diagnostics: the persistent grid (blocks) the last launch on the scene used, and the grid a
 * launch of that shape gets when the device is otherwise idle.  They differ for a one-frame launch
 * issued while the scene's previous launch, on another stream, was still running: it takes half
 * the block slots, so the two overlap (pixels and counts do not depend on it).  Either pointer may
 * be NULL. */
int rt_debug_last_grid(rt_scene* scene, long long* blocks, long long* full_blocks);

/* Test hook: replaces the scene's first 4-wide node by a cycle (its one child is itself, with a
 * box that holds every ray), so every production traversal that enters the hierarchy loops until
 * the kernel watchdog ends it.  Synchronises the device.  The scene is unusable afterwards. */
int rt_debug_corrupt_hierarchy(rt_scene* scene);

/* Diagnostics: what the device hierarchy of a scene would be, built on the host only (no HIP call,
 * no device needed): the binary tree of opt->device_tree, optimised as opt->tree_opt says, and its
 * 4-wide collapse.  Costs are relative to the root's surface area: sah_* = sum of the internal
 * nodes' areas + sum of the leaves' areas x their records, dp_* = the collapse's dynamic programme
 * at the root (collapse_c_tri per leaf slot, 1 per wide node), before and after the optimiser
 * (equal when it is off).  invalid = 0, or RT_TREE_BAD_* bits of the final binary tree.  opt NULL =
 * the defaults; opt->verbose also prints the optimiser's passes to stderr.  Returns RT_OK or the
 * RT_ERR_* code rt_scene_upload_ex would return for these arguments. */
enum {
  RT_TREE_BAD_UNION = 1,    /* an internal box is not the union of its children's */
  RT_TREE_BAD_LEAF = 2,     /* a leaf's box or records differ from the builder's */
  RT_TREE_BAD_RECORDS = 4,  /* a device record is referenced by no leaf or by several, or leaf order breaks */
  RT_TREE_BAD_IDS = 8,      /* a child id is not above its parent's, or a node is unreachable */
  RT_TREE_BAD_FIXPOINT = 16 /* the optimiser's last pass moved nothing, yet running it again changed the tree */
};
typedef struct rt_tree_report {
  long long binary_nodes, wide_nodes, records;
  long long moved;          /* subtrees the optimiser moved */
  double sah_before, sah_after, dp_before, dp_after;
  double seconds;           /* the optimiser's time, renumbering included */
  int passes;               /* passes run (0 = optimiser off) */
  int stack4;               /* traversal-stack entries the 4-wide tree needs */
  unsigned int invalid;
  int converged;            /* 1: the last pass moved nothing (a fixed point; checked by a second run) */
} rt_tree_report;
int rt_debug_tree_report(const rt_scene_soa* soa, const rt_bvh_soa* bvh, const rt_upload_options* opt,
                         rt_tree_report* out);

/* Diagnostics: per-round timeline of the last launch with RT_FLAG_TIMELINE: for wave w of the
 * persistent grid and its r-th traversal round (r < 256), words [8(256w + r), +8) = {round start,
 * round end} (s_memrealtime, 100 MHz ticks), busy lanes | owner lanes << 8 | (work queue not yet
 * empty) << 16 | shadow-ray lanes << 24, the most node + leaf iterations of a lane | the wave's
 * round-loop iterations << 32, then the time (ticks) | count << 40 of the wave-level iterations of
 * each kind: global-memory node, LDS-treelet node, leaf; last word: the longest wave-level iteration
 * | the round's setup time << 32.  Unused records are zero.  Synchronises the device; returns
 * words copied. */
long long rt_debug_timeline(rt_scene* scene, unsigned long long* out, long long n);

/* The render kernel's work tile: one wave's 64 pixels, *tile_w x *tile_h (8 x 8).  Tile positions
 * of the diagnostics below are ty * ceil(width / tile_w) + tx over the shard's
 * ceil(rows / tile_h) tile rows. */
int rt_tile_shape(int* tile_w, int* tile_h);

/* Diagnostics (tile-order experiments): the per-tile-position cost map of the last launch with
 * RT_FLAG_TILE_COST / RT_FLAG_TILE_COST_TIME / RT_FLAG_COST_ORDER (index ty * tiles_x + tx over the
 * shard's tiles (rt_tile_shape); per finished sample its bounces + 1, or per pixel its lifetime in 10-ns ticks;
 * summed over the launch's frames) into out[0..n); returns the number of positions, 0 if none. */
long long rt_debug_tile_cost(rt_scene* scene, unsigned int* out, long long n);
/* Diagnostics: launches with exactly n tiles take linear tile order[w / 64] for work item w (a
 * permutation; pixels do not depend on it); n = 0 clears. */
int rt_debug_set_tile_order(rt_scene* scene, const unsigned int* order, long long n);
/* Diagnostics: the tile order the last RT_FLAG_COST_ORDER launch used (order[i] = tile rendered i-th
 * within its work head's range) into out[0..n); returns its length, 0 if none. */
long long rt_debug_last_tile_order(rt_scene* scene, unsigned int* out, long long n);

void rt_scene_free(rt_scene* scene);

/* Thread-local message of the last failing call. */
const char* rt_last_error(void);

/* Build info string (kernel variants, arch) for logs. */
const char* rt_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
