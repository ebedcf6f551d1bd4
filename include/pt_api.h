/*
 * pt_api.h — C ABI of the MI355X path-tracing core (libpt_hip.so).
 *
 * This is the drop-in boundary for the reference's offline render path.  The
 * reference (jayHuggie/PathTracer_CUDA_Interactive) has no plugin/FFI API; the
 * seam is "upload the flattened Scene, seed the RNG, launch `render`, sync":
 *
 *   reference call site                       replaced by
 *   ----------------------------------------  ---------------------------------
 *   GPUScene::copyFrom        scene.h:73-119   pt_scene_create
 *   copyTriangleMeshToDevice  shape.cuh:48-59  pt_scene_create (mesh arrays)
 *   copyBVHNodesToDevice2     bvh.cu:83-97     pt_scene_create (node array)
 *   setup_rand<<<>>>          main.cu:54-62,234  (folded into pt_render: O(1) PCG init)
 *   render<<<>>> + sync       main.cu:30-52,258-260   pt_render / pt_render_async
 *   render_progressive<<<>>>  main.cu:64-89,333       pt_render_accumulate
 *   GPUScene::free            scene.h:144-171  pt_scene_destroy
 *   checkCudaErrors -> exit   bbox.cuh:7-17    int status + pt_last_error()
 *
 * All structs are plain C PODs mirroring the reference's host `Scene`
 * (scene.h:17-35): shapes, meshes, materials, lights, BVH nodes.  The caller
 * owns every input array; pt_scene_create copies what it needs (and re-lays it
 * out for the GPU), so inputs may be freed right after it returns.
 *
 * No torch / C++ types cross this boundary.  Thread-compatible: no hidden
 * global state except the thread-local error string.  A scene handle owns one
 * set of scratch buffers, so its renders must not overlap: calls on one handle
 * are issued from one thread at a time, and a render on another stream is
 * enqueued only after the previous one has finished (different handles are
 * independent).
 */
#ifndef PT_API_H
#define PT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_API_VERSION 1

/* status codes (0 = ok).  The reference exits the process instead (bbox.cuh:9-17). */
enum {
    PT_OK = 0,
    PT_ERR_INVALID_ARG = 1,
    PT_ERR_BAD_SCENE = 2,      /* inconsistent ids / topology / BVH deeper than the stack cap */
    PT_ERR_DEVICE = 3,         /* HIP runtime error */
    PT_ERR_NO_DEVICE = 4,
    PT_ERR_IO = 5,
    PT_ERR_PARSE = 6,
    PT_ERR_UNSUPPORTED = 7
};

/* shape.cuh:61  enum ShapeType {SPHERE, TRIANGLE} */
enum { PT_SHAPE_SPHERE = 0, PT_SHAPE_TRIANGLE = 1 };
/* material.h:27 enum MaterialType { DIFFUSE, MIRROR, PLASTIC, PHONG } */
enum { PT_MAT_DIFFUSE = 0, PT_MAT_MIRROR = 1, PT_MAT_PLASTIC = 2, PT_MAT_PHONG = 3 };
/* light.h:17    enum LightType { POINTLIGHT, DIFFUSEAREALIGHT } */
enum { PT_LIGHT_POINT = 0, PT_LIGHT_DIFFUSE_AREA = 1 };

/* Shape (shape.cuh:63-69): tagged union of Sphere{mat,light,center,radius}
 * and Triangle{face_index, mesh_index}.  Flattened here (no union) so that
 * ctypes / cgo / JNI can bind it without tricks. */
typedef struct pt_shape {
    int32_t type;            /* PT_SHAPE_* */
    int32_t material_id;     /* sphere only (triangles take the mesh's)   */
    int32_t area_light_id;   /* sphere only; -1 = not emissive            */
    float   center[3];       /* sphere */
    float   radius;          /* sphere */
    int32_t face_index;      /* triangle: index into mesh indices         */
    int32_t mesh_index;      /* triangle: index into pt_scene_desc.meshes */
} pt_shape;

/* TriangleMesh (shape.cuh:28-41) minus the device pointers and the UVs
 * (UVs never influence the result: texture.h:69-71 is constant-colour only). */
typedef struct pt_mesh {
    int32_t material_id;
    int32_t area_light_id;       /* -1 = not emissive */
    int32_t num_vertices;
    int32_t num_faces;
    const float*   positions;    /* [num_vertices*3] */
    const int32_t* indices;      /* [num_faces*3]    */
    const float*   normals;      /* [num_vertices*3], REQUIRED (every shipped scene has them) */
} pt_mesh;

/* Material (material.h:8-36).  Textures are constant colours (texture.h:12-15). */
typedef struct pt_material {
    int32_t type;            /* PT_MAT_* */
    float   reflectance[3];
    float   eta;             /* PLASTIC index of refraction */
    float   exponent;        /* PHONG exponent              */
} pt_material;

/* Light (light.h:5-27).  Only DiffuseAreaLight::radiance is ever read by the
 * hot path (radiance.cuh:36-41); point lights are carried for fidelity. */
typedef struct pt_light {
    int32_t type;            /* PT_LIGHT_* */
    int32_t shape_id;        /* area light: emitting shape */
    float   radiance[3];     /* area: radiance; point: intensity */
    float   position[3];     /* point light only */
} pt_light;

/* BVHNode (bvh.cuh:7-15) minus the two unused device pointers. */
typedef struct pt_bvh_node {
    float   bmin[3];
    float   bmax[3];
    int32_t left;            /* -1 on leaves */
    int32_t right;           /* -1 on leaves */
    int32_t prim;            /* shape index on leaves, -1 on inner nodes */
} pt_bvh_node;

/* The flattened scene: what Scene (scene.h:17-35) holds after its ctor ran. */
typedef struct pt_scene_desc {
    int32_t num_shapes;     const pt_shape*    shapes;
    int32_t num_meshes;     const pt_mesh*     meshes;
    int32_t num_materials;  const pt_material* materials;
    int32_t num_lights;     const pt_light*    lights;
    int32_t num_nodes;      const pt_bvh_node* nodes;     /* 2*num_shapes-1, post-order (bvh.cu:16-54) */
    int32_t root;           /* = num_nodes-1 for the reference builder */
    float   background[3];
} pt_scene_desc;

/* Per-render inputs: what `render` takes by value (main.cu:30-31) plus the
 * constants the reference hard-codes (seed 1984 main.cu:61; MAX_DEPTH 50
 * radiance.cuh:12; RR after depth>5 radiance.cuh:68). */
typedef struct pt_render_params {
    float    cam_origin[3];          /* CameraRayData (camera.cuh:21-26) */
    float    cam_top_left[3];
    float    cam_horizontal[3];
    float    cam_vertical[3];
    int32_t  width, height;          /* full image size (u,v and pixel_index use these) */
    int32_t  spp;                    /* samples rendered by this call */
    int32_t  row_begin, row_end;     /* rows [row_begin,row_end) rendered by this call; 0,0 = all.  Multi-GPU shard. */
    int32_t  row_stride;             /* 0/1 = contiguous rows; k>1 = rows row_begin, row_begin+k, ... < row_end (interleaved bands of 1 row) */
    uint64_t seed;                   /* PCG seed (reference literal: 1984) */
    int32_t  max_depth;              /* 0 -> 50 */
    int32_t  rr_depth;               /* Russian roulette when depth > rr_depth; <0 -> 5 */
    int32_t  sample_offset;          /* first absolute sample index of this call (progressive) */
    int32_t  stream_stride;          /* PCG stream = pixel_index*stream_stride + sample_offset + s; 0 -> spp */
    int32_t  traversal;              /* PT_TRAVERSAL_* */
    int32_t  flags;                  /* PT_RENDER_* bits; 0 = the reference's estimator */
} pt_render_params;

/* pt_render_params.flags */
enum {
    /* Next-event estimation — an EXTENSION, the reference samples no light (its point lights are parsed,
     * light.h:5-8, and never used; its occlusion query is dead code, scene.h:306-330).  Every non-specular hit samples one
     * entry of scene.lights[] uniformly (area lights: a uniform point on the emitting primitive; point lights) and
     * connects to it with a shadow ray; emission found by BSDF sampling then counts only on camera rays and after
     * specular bounces.  Same expectation as the reference's estimator when all light comes from area lights, less
     * noise; point lights start to light the scene.  Off by default; every parity and roofline number is taken without it. */
    PT_RENDER_NEE = 1
};

enum {
    PT_TRAVERSAL_DEFAULT = 0,        /* library picks (currently EXACT) */
    PT_TRAVERSAL_EXACT   = 1,        /* visit exactly the nodes the reference visits (no closest-t pruning, scene.h:278-297) */
    PT_TRAVERSAL_PRUNED  = 2         /* skip subtrees whose box entry is beyond the closest hit; same image, fewer visits */
};

/* Work counters of the last pt_render* call on a scene (device-side 64-bit
 * sums).  `segments` = number of intersect() calls = the "samples" of the
 * Msamples/s metric. */
typedef struct pt_counters {
    uint64_t paths;
    uint64_t segments;
    uint64_t node_visits;      /* inner-node pops actually executed by the kernel */
    uint64_t leaf_tests;       /* primitive tests actually executed */
    double   kernel_ms;        /* hipEvent time of the trace kernel(s) of the last call */
    double   resolve_ms;       /* hipEvent time of the per-pixel resolve kernel(s) */
} pt_counters;

typedef struct pt_scene pt_scene;    /* opaque: owns all device memory of one scene on one GPU */

/* Create a device scene on the CURRENT HIP device.  Validates ids/topology
 * (PT_ERR_BAD_SCENE instead of device printf: scene.h:260-263). */
int pt_scene_create(const pt_scene_desc* desc, pt_scene** out);
int pt_scene_destroy(pt_scene* scene);

/* New geometry and / or new shading values on a live handle — an EXTENSION, like PT_RENDER_NEE: the reference builds everything
 * anew for every scene it loads.  The handle keeps its scratch memory, frame slots, options and timing rings; both of its trees
 * keep the TOPOLOGY pt_scene_create gave them and get exact new boxes on the device (csrc/pt_scene_refit.hip): a leaf's box is
 * the host pipeline's shape box (sphere: centre -/+ radius; triangle: per axis min(min(p0, p1), p2) / max, `a < b ? a : b`),
 * an inner node's box the union of its two children's.  That is the tree pt_host_refit_bvh writes, and an updated handle
 * renders, bit for bit and through every entry point, what a fresh pt_scene_create of the new desc with those nodes renders
 * (no other entry point's output changes by a bit on a handle that was never updated).
 *   Blocking: waits for every frame of this handle that is still in flight (a device synchronise, as in pt_scene_create), works
 *   on the default stream and synchronises again before it returns.
 *   desc->nodes, num_nodes and root are ignored.  num_shapes must be pt_scene_create's; with PT_UPDATE_SHADING num_materials and
 *   num_lights too (PT_ERR_INVALID_ARG otherwise, pt_last_error() names the field).
 *   PT_UPDATE_GEOMETRY  shapes and meshes are read again in full (positions, normals, indices, material and light ids, sphere
 *                       data; the number of meshes may differ), ids checked with pt_scene_create's messages (PT_ERR_BAD_SCENE).
 *                       A vertex coordinate, sphere centre or radius that a shape uses and that is not finite, or a new leaf
 *                       box that is not finite (an overflowing centre + radius): PT_ERR_UNSUPPORTED.  This is stricter than
 *                       pt_scene_create, which takes the caller's boxes as they are.
 *                       PT_ERR_UNSUPPORTED also on the first geometry update of a handle one of whose trees is deeper than
 *                       256 levels (the caller's tree: at most 64 by the traversal stack; the library's own: logarithmic in
 *                       num_shapes), before anything is changed: such a handle cannot be updated at all.
 *   PT_UPDATE_SHADING   materials, lights and background are read again with pt_scene_create's checks.
 *   A call that fails leaves the handle exactly as it was: new records and leaf boxes are made and checked in staging memory
 *   (kept with the handle: 144 bytes per shape — records and vertex normals in staging, and the records that were live before
 *   the last geometry update, which pt_render_guides reads; the three record buffers rotate, none is copied — 24 more for scenes
 *   beyond a few thousand shapes) before anything is replaced.
 *   Decided at pt_scene_create and not revisited: whether an internal tree exists and which topology it has, the stack caps, the
 *   order of the top-of-tree prefix kept in LDS (it stays parent-before-child; only its "largest boxes first" choice ages) and
 *   "fast_tree_cost_permille".  Boxes stay exact however far the geometry moves, their quality does not: a caller whose geometry
 *   has drifted far from what the trees were built for should create a new handle.
 *   pt_scene_get_info: "updates" = successful updates so far; "update_us0".."update_us3" = wall microseconds of the last one:
 *   total, records including uploads, refit of both trees with their octant tables (host time up to its last enqueue: what the
 *   level launches of a large tree still have to execute ends inside the closing synchronise and is in the total alone), the
 *   one-time plan build (0 after the first).  That first update costs more than a pt_scene_create.
 *   "refit_shape0" / "refit_shape1" = how geometry updates refit the caller's tree / the internal one: 0 no plan (no such tree,
 *   a one-shape scene, or no geometry update yet), 1 one launch for the whole tree, 2 a scatter, a launch per wide level and
 *   the single-workgroup launch for the narrow top, 3 a scatter and that single-workgroup launch alone. */
enum { PT_UPDATE_GEOMETRY = 1, PT_UPDATE_SHADING = 2 };
int pt_scene_update(pt_scene* scene, const pt_scene_desc* desc, int flags);

/* Rigid animation by one matrix per group of shapes, on the device — an EXTENSION, like pt_scene_update: off unless called, never
 * part of a parity or roofline number.  The handle holds its geometry as primitive records already; a caller whose objects only
 * move uploads 84 bytes per object instead of every vertex.
 *   pt_scene_set_groups  group_of_shape[num_shapes], every value in [-1, num_groups); -1 = the shape never moves, its record is
 *                        copied bit for bit.  0 <= num_groups <= 2^20.  Uploads the ids (4 bytes per shape), replaces an earlier
 *                        assignment and does not touch the geometry.  An id out of range: PT_ERR_INVALID_ARG, pt_last_error()
 *                        names group_of_shape[k]; the earlier assignment stays.
 *   pt_scene_transform   transforms[num_groups]; num_groups must be the assignment's, and there must be one (PT_ERR_INVALID_ARG).
 *                        Transforms are ABSOLUTE: they apply to the REST geometry — the records that were live after
 *                        pt_scene_create or after the last successful pt_scene_update(PT_UPDATE_GEOMETRY) —, which the handle
 *                        copies device-to-device into buffers of its own on the first transform after either of those (96 bytes
 *                        per shape, freed with the scene; a geometry update drops the copy).  Repeated calls never accumulate
 *                        rounding.
 * The rule (csrc/pt_transform.h), fp32, operations in the order written, no contraction, cross and dot as at pt_render_guides:
 *   rows r0 = (m0,m1,m2), r1 = (m4,m5,m6), r2 = (m8,m9,m10).
 *   point   x' = ((m0 x + m1 y) + m2 z) + m3, rows 1 and 2 alike.
 *   normal  c0 = cross(r1,r2), c1 = cross(r2,r0), c2 = cross(r0,r1); det = dot(r0,c0); det < 0 negates all nine entries;
 *           n'.x = (c0.x nx + c0.y ny) + c0.z nz, the other components alike.  Not renormalised: shading normalises after
 *           interpolation.  Made once per group on the host; 21 floats per group go to the device.
 *           det == 0, a NaN det or any m[i] that is not finite: PT_ERR_INVALID_ARG naming transforms[g], before anything changes.
 *           A cofactor that overflowed (a uniform scale beyond about 1e19): PT_ERR_UNSUPPORTED naming transforms[g], likewise.
 *   sphere  the centre as a point; r' = r * sqrt((m0 m0 + m4 m4) + m8 m8), sqrt correctly rounded.  The linear part is expected
 *           to be a similarity; the library does not check that.
 *   triangle  the nine corner coordinates and the nine normal components of its record; material, light and padding are copied.
 *   A RESULT that is not finite is caught as in pt_scene_update: PT_ERR_UNSUPPORTED, the handle unchanged.
 * Blocking, on the default stream, with pt_scene_update's two synchronises.  A call that fails leaves the handle exactly as it
 * was: the new records and leaf boxes are made and checked in the staging buffers pt_scene_update uses.  On success the record
 * buffers rotate as they do there (staging -> current -> previous): "prev_geometry" becomes 1 and PT_MOTION_GEOMETRY_PREVIOUS
 * sees the records from before this call.  Everything pt_scene_update documents about the result holds: topology kept, exact
 * boxes, the box sweep of small scenes dropped for the tree, the 256-level limit, the plan build on the first call.  The handle
 * then renders, bit for bit and through every entry point, what pt_scene_update(PT_UPDATE_GEOMETRY) renders when given the desc
 * that the two host functions below produce from the rest desc.
 *   pt_scene_get_info: "groups" = groups of the assignment (0: none); "rest_geometry" = 1 while a copy of the rest records is
 *   held; "transforms" = successful pt_scene_transform calls so far; "transform_us0".."transform_us3" = wall microseconds of the
 *   last one: total, records (table upload and the kernel's enqueue), refit, and the one-time copy of the rest records plus the
 *   plan build (0 when neither was due).
 * pt_transform_geometry_host / pt_transform_sphere_host: the same source compiled for the HOST; they need no GPU and no scene.
 * positions, normals, positions_out, normals_out: [n, 3] each; normals and normals_out may both be NULL; an output may be its
 * input.  A transform the rule refuses: the status pt_scene_transform gives it; a NULL argument otherwise: PT_ERR_INVALID_ARG. */
typedef struct pt_transform { float m[12]; } pt_transform;   /* row-major 3x4: x' = m[0]x + m[1]y + m[2]z + m[3], ... */   /* 48 bytes */
int pt_scene_set_groups(pt_scene* scene, const int32_t* group_of_shape, int32_t num_groups);
int pt_scene_transform(pt_scene* scene, const pt_transform* transforms, int32_t num_groups);
int pt_transform_geometry_host(const pt_transform* t, int32_t n, const float* positions, const float* normals,
                               float* positions_out, float* normals_out);
int pt_transform_sphere_host(const pt_transform* t, const float* center, float radius, float* center_out, float* radius_out);

/* A fresh internal tree on a live handle — an EXTENSION, like pt_scene_update: off unless called; no other entry point's output
 * changes by a bit and a handle that never calls it behaves and is timed as before.  pt_scene_update and pt_scene_transform keep
 * the topology of both trees; the internal tree's quality then decays with the geometry (6.8 x the node visits
 * on a grid of 343 cubes that traded places).  This call builds the internal tree anew over the leaf boxes the handle's copy of
 * the caller's tree holds now — the caller's own boxes before any geometry update, the exact ones after — by pt_scene_create's
 * own internal-tree stage (on the device from 4096 shapes, on the host below), probes it against the caller's tree as it stands
 * with pt_scene_create's rays and adopts it iff it visits at least 10 % fewer nodes.  Any tree over the same leaf boxes
 * renders the same bits, so a rebuilt handle is a freshly created one, frame for frame and node visit for node
 * visit, that has kept what a new handle loses: the previous-geometry records pt_render_guides reads, the rest records and the
 * group assignment, frame slots, options, timing rings and counters.  The caller's tree, its refit plan and the tie tables are
 * never touched (the tables hold the caller's topology only).
 *   flags must be 0 (reserved): PT_ERR_INVALID_ARG otherwise and for a NULL scene.
 *   PT_ERR_UNSUPPORTED, pt_last_error() saying which, when the handle holds no tie tables — pt_scene_create kept no internal tree:
 *   fewer than 16 shapes, boxes that do not nest, the sweep tree lost the probe on an LDS-resident scene, or no room for the
 *   tables.  A handle whose internal tree is the caller's own topology ("fast_tree_is_callers" 1) is eligible.
 *   Blocking, on the default stream, with pt_scene_update's two synchronises.  Everything is made in new buffers; a call that
 *   fails (out of memory, a HIP error, the builder refusing) leaves the handle exactly as it was.
 *   Adopted: the internal tree, its depth, stack cap, top prefix and octant tables are replaced, "fast_tree" is 1,
 *   "fast_tree_is_callers" 0, "fast_tree_cost_permille" the new ratio, "sweep_on_device" follows the new build; the tree's refit
 *   plan is built again inside this call where the handle had one; scenes of at most 64 primitives get their box sweep back
 *   under pt_scene_create's admission rules.  Not adopted: PT_OK all the same, the handle keeps the internal tree it had and
 *   nothing observable changes but the keys below.
 *   pt_scene_get_info: "rebuilds" = successful calls; "rebuild_adopted" = the last one adopted its tree; "rebuild_cost_permille" =
 *   the last candidate's probe ratio; "rebuild_us0".."rebuild_us3" = wall microseconds of the last one: total, leaf boxes + build,
 *   re-layout + probe, plan + sweep tables.
 * When to call it — pt_scene_set_option "tree_cost" 1 (default 0): every geometry update and transform also measures both trees'
 * cost, the sum over every inner node below the root of its box area in fp64 (e = (double)max - (double)min per axis,
 * a = 2.0 * ((ex ey + ey ez) + ez ex), no contraction), on the device in a fixed order (csrc/pt_tree_cost.hip: the same bits on
 * every run), read back without a further synchronise.  "tree_cost0_bits" / "tree_cost1_bits" = the fp64 bit pattern of the
 * caller's / the internal tree's cost after the last refit (0: no tree, nothing measured); "tree_cost0_permille" /
 * "tree_cost1_permille" = (int64)(1000.0 * now / reference + 0.5), the reference being the cost of the boxes as they stood
 * before the first refit after the option was set; 1000 before any refit.  An adopted rebuild makes the new tree's cost the
 * internal tree's reference, one that was not adopted makes the current cost the reference.  Switching the telemetry off (both
 * options 0) forgets its references and costs: switched on again it starts as on a new handle, the keys read 0 / 1000 and the
 * next refit takes its references from the boxes as they stand then.  pt_host_tree_cost (pt_host.h) is the host twin.  Option "rebuild_at_permille" (default 0 = never, else >= 1001; implies the telemetry): a successful
 * pt_scene_update(PT_UPDATE_GEOMETRY) or pt_scene_transform whose "tree_cost1_permille" is at or above the value rebuilds inside
 * the same call, after the refit and before the closing synchronise ("update_us0" / "transform_us0" include it).  A rebuild that
 * fails there does not fail the update; "rebuilds_auto" counts the ones that succeeded. */
int pt_scene_rebuild(pt_scene* scene, int flags);

/* Blocking render.  `fb` receives rows x width x 3 floats, rows = the rows
 * selected by (row_begin,row_end,row_stride), packed in increasing row order;
 * fb[(r*W+i)*3+c], linear radiance, row 0 = top (main.cu:35,50).
 * fb_on_device != 0: fb is a device pointer on the scene's GPU. */
int pt_render(pt_scene* scene, const pt_render_params* p, float* fb, int fb_on_device);

/* Same, enqueued on a caller-provided hipStream_t (NULL = default stream); fb
 * must be a device pointer; returns without synchronising.  What the caller can
 * observe — fb, and accum_dev below — is written in the order of that stream.  The
 * trace kernel itself reads only the scene and writes scratch memory of the handle,
 * so with "frames_in_flight" > 1 (option, default 2) a frame runs on a stream of the
 * handle's own — its resolve behind an event of the caller's stream, the caller's
 * stream behind its resolve — and the trace kernel of call k+1 fills the compute
 * units while the last paths of call k drain; same bits either way. */
int pt_render_async(pt_scene* scene, const pt_render_params* p, float* fb_dev, void* hip_stream);

/* Progressive accumulation (render_progressive, main.cu:64-89): adds the SUM
 * of p->spp new samples (absolute indices sample_offset..) into accum_dev
 * (same layout as fb; overwritten when sample_offset == 0).  Async on stream. */
int pt_render_accumulate(pt_scene* scene, const pt_render_params* p, float* accum_dev, void* hip_stream);

/* Adaptive sampling — an EXTENSION, like PT_RENDER_NEE: the reference gives every pixel the same spp.  Parameter names are
 * borrowed from Mitsuba 0.6's `adaptive` integrator (maxError, pValue, maxSampleFactor); the semantics are this library's own.
 * Never part of a parity or roofline number. */
typedef struct pt_adaptive_params {
    int32_t batch_spp;      /* samples added per round to every pixel still above target; 0 -> p->spp   */
    int32_t max_spp;        /* most samples of one pixel; 0 -> 32 * p->spp; p->spp <= max_spp <= 2^20 */
    float   max_error;      /* target: relative half-width of the confidence interval, > 0, finite   */
    float   p_value;        /* two-sided, z = Phi^-1(1 - p/2); 0 -> 0.05; else in (0, 1)             */
    float   min_luminance;  /* floor of the relative test's denominator, >= 0, used as given         */
} pt_adaptive_params;       /* 20 bytes */

/* Blocking render with per-pixel sample counts.  fb, spp_map and err_map use pt_render's [rows, W] packing of the rows selected by
 * (row_begin, row_end, row_stride); spp_map and err_map may be NULL.  on_device != 0: all three are device pointers on the
 * scene's GPU.
 *   Rounds: p->spp is the first round, every selected pixel gets that many samples; every later round adds batch_spp samples to
 *   each pixel still above target.  Checkpoints fall at n = spp, spp + batch, spp + 2 batch, ..., the last one cut to max_spp;
 *   they depend on spp, batch_spp and max_spp only (a round that does not fit "scratch_bytes" runs in several passes before its
 *   one check).  p->sample_offset must be 0; p->stream_stride is 0 (= max_spp) or >= max_spp; sample k of a pixel uses PCG stream
 *   pixel_index * stride + k, so a pixel that stops at n samples holds exactly what pt_render gives it at spp = n with that stride.
 *   Camera, seed, depths, traversal, PT_RENDER_NEE, row selection and every option mean what they mean in pt_render.
 *   The rule at a checkpoint with n samples: Y_k = 0.2126 R_k + 0.7152 G_k + 0.0722 B_k in fp64 (left to right, no contraction);
 *   S1 = sum Y_k, S2 = sum Y_k^2 in fp64 in sample order; mean = S1/n; var = max(0, (S2 - S1*S1/n)/(n-1)), +inf for n == 1;
 *   half = z sqrt(var/n); err = half == 0 ? 0 : half / max(mean, min_luminance).  The pixel stops when err <= max_error (a NaN
 *   never does) or n == max_spp.
 *   Outputs: fb = (sum of the n samples) * (1/n) as in pt_render; spp_map = n; err_map = err at the stopping checkpoint (above
 *   max_error only where n == max_spp).  pt_get_counters covers the whole call (paths = sum of spp_map; kernel_ms / resolve_ms
 *   summed over all rounds); pt_scene_get_info "adaptive_rounds" = rounds of the last adaptive call.  Runs on the default stream. */
int pt_render_adaptive(pt_scene* scene, const pt_render_params* p, const pt_adaptive_params* a,
                       float* fb, int32_t* spp_map, float* err_map, int on_device);

/* An explicit list of pixels — an EXTENSION, like PT_RENDER_NEE: the reference renders whole frames.  Picking, a region of
 * interest, sparse probes, and the re-trace pt_temporal_gradient_sparse reads.  DESIGN.md §22.
 *   pixels[k] = j * width + i, the pixel index the PCG stream uses; out is [n, 3].  out[k] holds the bits pt_render writes to fb
 *   for that pixel with the same parameters and every row selected — for any spp, seed, sample_offset, stream_stride, depths,
 *   traversal, PT_RENDER_NEE and any option.  Order is free, duplicates are allowed, every entry is independent.
 *   p->row_begin / row_end / row_stride must select every row (0, 0 or 0, height; 0 or 1): PT_ERR_INVALID_ARG otherwise.
 *   on_device != 0: pixels and out are device pointers; the call is enqueued on hip_stream without a host sync, as
 *   pt_render_async is, and what the caller observes is written in the order of that stream.  It is a plain frame (not an
 *   adaptive round) and takes its turn in the "frames_in_flight" rotation of scratch memory, but always runs on the caller's
 *   stream: its trace kernel reads the caller's list, which must stay valid until the stream has passed the call.  The library
 *   cannot inspect such a list: out[k] of an entry outside [0, W * H) is unspecified and nothing else is affected — no address
 *   is formed from an entry, only u, v and the PCG stream (out and the scratch memory are indexed by k).
 *   on_device == 0: host pointers, blocking, on the default stream, staged through memory of the handle (grown on demand,
 *   freed with the scene); an entry outside [0, W * H): PT_ERR_INVALID_ARG, pt_last_error() names pixels[k].
 *   n < 0, n > 2^30, n > 0 with a NULL pixels or out: PT_ERR_INVALID_ARG, pt_last_error() names the argument; pt_render's own
 *   parameter errors as in pt_render.  n == 0: PT_OK, nothing is written, the counters read zero.
 *   The launch is a frame of n rows of width 1 run by the LIST instantiation of the trace kernel that the later rounds of
 *   pt_render_adaptive run (info "trace_variant" has bit 11 set), and options mean what they mean there: "kernel" 1 is
 *   honoured, 3 runs on 2; "v2_thresh" / "v2_inner" / "v2_minw" are ignored (the LIST kernels are compiled for the automatic
 *   schedule of each residency only; no schedule changes a bit); "reg_stack", "leaf_sweep" and the path bank do not apply;
 *   "scratch_bytes", "xcd_regions", "item_order", "chunk", "blocks_per_cu", "stats", "force_global", "fast_tree" and the rest
 *   act on the n x 1 frame.  pt_get_counters covers the call (paths = n * spp). */
int pt_render_pixels(pt_scene* scene, const pt_render_params* p, const int32_t* pixels, int32_t n, float* out, int on_device,
                     void* hip_stream);

/* Guide buffers of the first hit ("AOVs") — an EXTENSION, like PT_RENDER_NEE: the reference's only per-pixel output is radiance.
 * Never part of a parity or roofline number; no other entry point's output changes by a bit.
 *   One ray per selected pixel through the pixel CENTRE, u = ((float)i + 0.5f) / (float)width, v = ((float)j + 0.5f) / (float)height,
 *   the camera ray of camera.cuh:45-50 and the closest-hit query a camera segment of pt_render runs (tnear 0, tfar +inf).
 *   p->traversal, "fast_tree" and every other option mean what they mean in pt_render (under PT_TRAVERSAL_EXACT none of them
 *   changes an output bit); row selection and the [rows, W] packing are pt_render's.  spp, seed, sample_offset, stream_stride,
 *   depths and flags are ignored.  Blocking, on the default stream.  Any output pointer may be NULL; on_device != 0: all of them
 *   are device pointers on the scene's GPU.
 *   prim    [rows, W]     shape id of the closest hit, -1 on a miss
 *   depth   [rows, W]     the hit's t, 0 on a miss
 *   normal  [rows, W, 3]  the shading normal (interpolated vertex normals / sphere normal, normalised), turned to the side the
 *                         ray came from (negated when dot(-dir, n) < 0) as the renderer turns it; (0,0,0) on a miss
 *   albedo  [rows, W, 3]  the hit material's reflectance; (1,1,1) for PT_MAT_MIRROR; (0,0,0) on a miss and where pt_render's first
 *                         segment adds emission at this hit (light id in range, that light a diffuse area light, seen from the
 *                         front).  "All three channels 0" is what pt_denoise reads as "leave this pixel alone". */
int pt_render_aov(pt_scene* scene, const pt_render_params* p,
                  float* albedo, float* normal, float* depth, int32_t* prim, int on_device);

/* Edge-avoiding à-trous filter guided by those buffers — an EXTENSION: an image-space stage after pt_render /
 * pt_render_accumulate / pt_render_adaptive, off unless called.  DESIGN.md §17. */
typedef struct pt_denoise_params {
    int32_t width, height;        /* full frame; the filter works on whole frames only                     */
    int32_t iterations;           /* 0 -> 5; else 1..8; iteration k uses tap spacing 2^k                   */
    int32_t normal_power_log2;    /* 0..10, used as given: normal weight = max(0, n_p.n_q)^(2^this); tools use 7 */
    float   sigma_z;              /* 0 -> 0.05; else > 0, finite: relative depth difference at half weight  */
    float   sigma_c;              /* 0 = no colour term; else > 0, finite: luminance difference at half weight in
                                     iteration 0, halved per iteration */
    float   scale;                /* 0 -> 1; else > 0, finite: input colour is multiplied by it first (1/n for a pt_render_accumulate sum) */
    float   albedo_floor;         /* 0 -> 0.01; else > 0, finite                                            */
} pt_denoise_params;              /* 32 bytes */

/* color, albedo, normal [H, W, 3], depth [H, W] -> out [H, W, 3]; out may be color.  The handle supplies the device and owns the
 * scratch records (48 bytes per pixel, allocated on first use, freed with the scene).  on_device != 0: device pointers, enqueued
 * on hip_stream (NULL = default stream) without a host sync, so that it can follow pt_render_async / pt_render_accumulate on
 * the caller's stream; on_device == 0: host pointers, blocking.  A parameter out of range -> PT_ERR_INVALID_ARG, pt_last_error()
 * names the field.
 *   The rule, in fp32, operations in the order written, no contraction.  lum(c) = 0.2126f c.r + 0.7152f c.g + 0.0722f c.b and dot
 *   left to right; h = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *   A pixel is filterable iff max(albedo.r, albedo.g, albedo.b) > 0.  a' = max(albedo, albedo_floor) per channel.
 *   x_0 = color * scale / a' (IEEE division) for filterable pixels, color * scale otherwise.
 *   Iteration k = 0 .. iterations - 1, spacing s = 1 << k, reads x_k, writes x_{k+1}.  A pixel that is not filterable is copied.
 *   For a filterable pixel p: sum = (0,0,0), wsum = 0; taps q = p + s (dx, dy) in the order dy = -2..2 (outer), dx = -2..2 (inner);
 *   a tap outside the frame or not filterable is skipped; otherwise
 *     wn = max(0, dot(n_p, n_q)), squared normal_power_log2 times;
 *     rd = (z_p - z_q) * (1.0f / max(z_p, 1e-20f));  wz = 1.0f / (1.0f + (rd * rd) * kz),  kz = 1.0f / (sigma_z * sigma_z);
 *     w = ((h[dy + 2] * h[dx + 2]) * wn) * wz;
 *     with a colour term: dl = lum(x_k[p]) - lum(x_k[q]);  w = w * (1.0f / (1.0f + (dl * dl) * kc)),  kc = 1.0f / (sc * sc),
 *     sc = sigma_c * 2^-k;
 *     sum += x_k[q] * w per channel, wsum += w.
 *   x_{k+1}[p] = sum * (1.0f / wsum).  out = x_last * a' for filterable pixels, x_last otherwise.
 *   Weights are rational instead of exp so that every operation is a correctly rounded IEEE one: the device, pt_denoise_host and
 *   a numpy fp32 restatement give the same bits.  Non-finite input propagates; what it does is unspecified. */
int pt_denoise(pt_scene* scene, const pt_denoise_params* d, const float* color, const float* albedo,
               const float* normal, const float* depth, float* out, int on_device, void* hip_stream);
/* The same per-pixel source (csrc/pt_denoise.h) compiled for the HOST: needs no GPU and no scene. */
int pt_denoise_host(const pt_denoise_params* d, const float* color, const float* albedo,
                    const float* normal, const float* depth, float* out);

/* Motion vectors with the guide buffers, and temporal accumulation along them — an EXTENSION: off unless called, never part of
 * a parity or roofline number, no other entry point's output changes by a bit.  DESIGN.md §19.
 *   pt_render_guides is pt_render_aov (same rays, same traversal, same row selection and packing, the same four buffers bit for
 *   bit) with two more outputs from the same traversal, in one kernel launch: where each pixel's surface point was in the
 *   PREVIOUS frame, as seen by the previous camera.  The previous frame has the same width and height.  Blocking, on the default
 *   stream.  NULL p, m or out, or a geometry value other than the two below: PT_ERR_INVALID_ARG, pt_last_error() names it.
 *   "Previous geometry" = the primitive records that were live before the most recent successful PT_UPDATE_GEOMETRY; a handle
 *   that was never updated has previous = current; a shading-only update and a failed update change neither set.
 *   pt_scene_get_info "prev_geometry" = 1 when a distinct previous record set exists, else 0.
 *   Arithmetic: fp32 throughout, operations in the order written, no contraction; dot left to right;
 *   cross(a,b).x = a.y*b.z - a.z*b.y, cyclic for .y and .z; / is IEEE division; sqrt correctly rounded.
 *   A hit pixel has ray (o, d) and hit (k, t, u, v): what pt_debug_intersect returns for the pixel-centre ray.  Primed records
 *   are those `geometry` selects, unprimed the current ones.
 *     sphere flags of the two records differ: the pixel is invalid
 *     triangle: w = (1.0f - u) - v;  Q = (p0' w + p1' u) + p2' v per component (also with GEOMETRY_CURRENT, where p' = p)
 *     sphere:   P = o + d t;  Q = c' + (P - c) (r' / r)
 *   With the previous camera (o', tl', H', V'):
 *     e = Q - o';  a = tl' - o';  hv = cross(H', V');  D = dot(a, hv);  n0 = dot(e, hv);  s = n0 / D
 *     n1 = dot(a, cross(e, V'));  n2 = dot(a, cross(H', e))
 *     motion = ((n1 / n0) (float)width, (-(n2 / n0)) (float)height);  prev_depth = sqrt(dot(e, e))
 *   motion is the previous position in continuous pixel coordinates, the centre of pixel (i, j) being (i + 0.5, j + 0.5);
 *   coordinates outside the frame are valid output.  A pixel is INVALID when it is a miss, its record types differ, s > 0 is
 *   not true, or motion.x, motion.y or prev_depth is not finite; it gets motion = (0, 0) and prev_depth = 0, and
 *   prev_depth == 0 is the only flag a consumer reads.  Not covered: what is seen in a mirror moves with the mirror's surface. */
enum { PT_MOTION_GEOMETRY_CURRENT = 0, PT_MOTION_GEOMETRY_PREVIOUS = 1 };
typedef struct pt_motion_params {
    float   prev_cam_origin[3], prev_cam_top_left[3], prev_cam_horizontal[3], prev_cam_vertical[3];
    int32_t geometry;             /* PT_MOTION_GEOMETRY_* */
} pt_motion_params;               /* 52 bytes */
typedef struct pt_guide_buffers { /* any pointer may be NULL; on_device != 0: all are device pointers on the scene's GPU */
    float*   albedo;              /* pt_render_aov's four */
    float*   normal;
    float*   depth;
    int32_t* prim;
    float*   motion;              /* [rows, W, 2] */
    float*   prev_depth;          /* [rows, W]    */
} pt_guide_buffers;
int pt_render_guides(pt_scene* scene, const pt_render_params* p, const pt_motion_params* m, const pt_guide_buffers* out,
                     int on_device);
/* pt_render_guides for a frame that is enqueued and left alone: the same arguments, rules, row selection and NULL-output rule,
 * the same bits in every buffer, on DEVICE pointers only, enqueued on hip_stream (NULL = the default stream) without a host
 * sync; what the caller observes is written in stream order.  m == NULL: pt_render_aov's four buffers (motion and prev_depth
 * are not written).  NULL p or out, a bad geometry value, a bad frame or row selection: PT_ERR_INVALID_ARG as there.
 * It reads scene memory only, takes no frame slot and leaves pt_get_counters, pt_get_frame_times and info "trace_variant" as
 * they were.  The kernel: option "query_guides" 0 (default) = automatic, 1 = the lane-refilling query kernel of pt_trace_rays
 * (below), 2 = pt_render_guides' own one-shot kernel on hip_stream.  Automatic is the one-shot kernel — camera rays are coherent,
 * and the refilling kernel measured slower on them at every scene and size tried — unless "query_blocks" is set, which asks for
 * the refilling kernel; info "query_guides" reports what the last call ran on (1 refilling, 0 one-shot).  DESIGN.md §24. */
int pt_render_guides_async(pt_scene* scene, const pt_render_params* p, const pt_motion_params* m, const pt_guide_buffers* out,
                           void* hip_stream);

/* Carries a colour history along those motion vectors: an exponential average whose length grows by one per frame up to
 * max_history where the reprojected history agrees with this frame in depth and normal, and restarts elsewhere. */
typedef struct pt_temporal_params {
    int32_t width, height;        /* whole frames only                                                      */
    int32_t max_history;          /* 0 -> 32; else 1..65536                                                 */
    float   sigma_z;              /* 0 -> 0.1; else > 0, finite: relative depth tolerance                   */
    float   normal_min;           /* used as given, in [-1, 1]; tools use 0.9                               */
    float   scale;                /* 0 -> 1; else > 0, finite: color is multiplied by it first              */
} pt_temporal_params;             /* 24 bytes */

/* color, normal, hist_color, hist_normal, out_color [H, W, 3]; motion [H, W, 2]; prev_depth, hist_depth, hist_len, out_len [H, W].
 * on_device != 0: device pointers, enqueued on hip_stream (NULL = default stream) without a host sync, as pt_denoise is;
 * on_device == 0: host pointers, blocking (staged through memory of the handle).  The library keeps no state: after a call,
 * (out_color, normal, depth, out_len) of this frame are the next call's hist_*, and the caller ping-pongs them.  out_color may
 * be color.  out_color == hist_color or out_len == hist_len: PT_ERR_INVALID_ARG, because neighbours are gathered.  All four
 * hist_* NULL = no history, every pixel takes the fallback (some but not all NULL: PT_ERR_INVALID_ARG).  A parameter out of
 * range, a NULL parameter struct: PT_ERR_INVALID_ARG, pt_last_error() names the field.
 *   The rule per pixel p = (i, j), in fp32, in the order written, no contraction, with c = color[p] * scale.
 *   Fallback: out = c, out_len = 1.
 *   1. prev_depth[p] == 0: fallback.
 *   2. x = motion.x - 0.5f, y = motion.y - 0.5f.
 *   3. Unless x >= -1 && x < W && y >= -1 && y < H: fallback.
 *   4. x0 = floorf(x), y0 = floorf(y), fx = x - x0, fy = y - y0.
 *   5. Taps in the order (dy, dx) = (0,0), (0,1), (1,0), (1,1): q = ((int)x0 + dx, (int)y0 + dy),
 *      b = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy).
 *   6. A tap is skipped when q is outside the frame (no address is formed for it), hist_len[q] > 0 is not true,
 *      hist_depth[q] == 0, fabsf(hist_depth[q] - prev_depth[p]) <= sigma_z * prev_depth[p] is not true, or
 *      dot(normal[p], hist_normal[q]) >= normal_min is not true (dot left to right).
 *   7. A kept tap: sum += hist_color[q] * b per channel, lsum += hist_len[q] * b, wsum += b.
 *   8. wsum > 0: r = 1.0f / wsum, h = sum * r, n = min(lsum * r + 1.0f, (float)max_history),
 *      out = h + (c - h) * (1.0f / n), out_len = n.  Otherwise fallback.
 *   Normals are compared in WORLD space: an object that rotates fast loses its history although its surface points are
 *   followed correctly.  Non-finite input propagates; what it does is unspecified. */
int pt_temporal_accumulate(pt_scene* scene, const pt_temporal_params* t, const float* color, const float* normal,
                           const float* motion, const float* prev_depth, const float* hist_color, const float* hist_normal,
                           const float* hist_depth, const float* hist_len, float* out_color, float* out_len, int on_device,
                           void* hip_stream);
/* The same per-pixel source (csrc/pt_temporal.h) compiled for the HOST: needs no GPU and no scene. */
int pt_temporal_accumulate_host(const pt_temporal_params* t, const float* color, const float* normal, const float* motion,
                                const float* prev_depth, const float* hist_color, const float* hist_normal,
                                const float* hist_depth, const float* hist_len, float* out_color, float* out_len);

/* Temporal luminance moments and a variance-guided à-trous filter — an EXTENSION: off unless called, never part of a parity or
 * roofline number, no other entry point's output changes by a bit.  DESIGN.md §20.
 *   pt_temporal_accumulate_moments is pt_temporal_accumulate with the first and second moment of the pixel's luminance carried
 *   along the same reprojection, in one launch; pt_denoise_variance is pt_denoise with a per-pixel, per-iteration luminance
 *   tolerance derived from those moments and propagated through the iterations.  lum, dot, filterable, a', x_0, wn, wz and h are
 *   pt_denoise's definitions above; fp32, operations in the order written, no contraction, IEEE division. */
typedef struct pt_temporal_io {   /* on_device != 0: all are device pointers on the scene's GPU */
    const float *color, *albedo, *normal, *motion, *prev_depth;                   /* this frame; albedo [H, W, 3] */
    const float *hist_color, *hist_normal, *hist_depth, *hist_len, *hist_moments; /* all five NULL = no history; some but not
                                                                                     all: PT_ERR_INVALID_ARG */
    float *out_color, *out_len, *out_moments;                                     /* moments: [H, W, 2] */
} pt_temporal_io;                 /* 104 bytes */

/* Buffers, call forms, staging and errors as pt_temporal_accumulate; albedo_floor: 0 -> 0.01, else > 0 and finite.  A NULL t or
 * io, a NULL pointer among this frame's five or the three outputs: PT_ERR_INVALID_ARG.  out_color may be color; out_color ==
 * hist_color, out_len == hist_len or out_moments == hist_moments: PT_ERR_INVALID_ARG.  After a call, (out_color, normal, depth,
 * out_len, out_moments) are the next call's hist_*.
 *   The rule per pixel p.  out_color and out_len are pt_temporal_accumulate's bit for bit: steps 1-8, the taps, the skip tests
 *   and b are the same.  With c = color[p] * scale:
 *     l = lum(c.r / a'.r, c.g / a'.g, c.b / a'.b) if filterable(albedo[p]), lum(c) otherwise;  m_c = (l, l * l)
 *   — the moments live in the demodulated space in which the spatial filter works.
 *   Fallback: out_moments = m_c.
 *   7. A kept tap, after lsum: msum += hist_moments[q] * b per component.
 *   8. wsum > 0: mh = msum * r, out_moments = mh + (m_c - mh) * (1.0f / n) per component, with step 8's r and n. */
int pt_temporal_accumulate_moments(pt_scene* scene, const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io,
                                   int on_device, void* hip_stream);
/* The same per-pixel source (csrc/pt_temporal.h) compiled for the HOST: needs no GPU and no scene. */
int pt_temporal_accumulate_moments_host(const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io);

typedef struct pt_vdenoise_params {
    int32_t width, height;        /* full frame; the filter works on whole frames only                      */
    int32_t iterations;           /* 0 -> 5; else 1..8; iteration k uses tap spacing 2^k                    */
    int32_t normal_power_log2;    /* 0..10, used as given, as in pt_denoise_params                          */
    float   sigma_z;              /* 0 -> 0.05; else > 0, finite                                            */
    float   sigma_l;              /* 0 -> 4; else > 0, finite: luminance tolerance in standard deviations   */
    float   scale, albedo_floor;  /* as in pt_denoise_params                                                */
    int32_t min_history;          /* 0 -> 4; else 1..65536: a shorter history takes the spatial variance estimate */
    float   var_floor;            /* 0 -> 1e-10; else > 0, finite: added to the tolerance, keeps it positive */
} pt_vdenoise_params;             /* 40 bytes */

/* color, albedo, normal [H, W, 3], depth, hist_len [H, W], moments [H, W, 2] -> out [H, W, 3], out_variance [H, W] (may be NULL);
 * out may be color.  moments and hist_len are pt_temporal_accumulate_moments' out_moments and out_len of the same frame (color
 * its out_color).  Call forms as pt_denoise: on_device != 0 enqueues 1 + iterations kernels on hip_stream without a host sync;
 * on_device == 0 is blocking and staged (56 bytes per pixel).  The handle owns the scratch records: 48 bytes per pixel of its
 * own, beside pt_denoise's, allocated on first use, freed with the scene.  A NULL pointer other than out_variance, a parameter
 * out of range: PT_ERR_INVALID_ARG, pt_last_error() names the argument or field.
 *   Prep.  x_0, a' and filterable as in pt_denoise.  A pixel that is not filterable has v = 0 at every stage, is copied through
 *   and is never a tap.  kz = 1.0f / (sigma_z * sigma_z), sl2 = sigma_l * sigma_l.
 *   Initial variance of a filterable p:  L = hist_len[p], m = moments[p], tv = max(0, m.y - m.x * m.x).
 *     L >= (float)min_history: v_0 = tv.
 *     Otherwise s1 = s2 = ws = 0; taps q = p + (dx, dy) in the order dy = -3..3 (outer), dx = -3..3 (inner), centre included;
 *     a tap outside the frame (no address is formed for it) or not filterable is skipped; otherwise w = wn * wz (pt_denoise's
 *     two guide weights from normal and depth, rd with 1.0f / max(z_p, 1e-20f)), s1 += moments[q].x * w, s2 += moments[q].y * w,
 *     ws += w.  ws > 0: r = 1.0f / ws, M1 = s1 * r, M2 = s2 * r, v_0 = max(0, M2 - M1 * M1) * (4.0f / max(L, 1.0f)); else v_0 = tv.
 *   Iteration k, spacing s = 1 << k, for a filterable p:
 *     g: gsum = cwsum = 0; taps q = p + (dx, dy) at spacing 1, dy = -1..1 (outer), dx = -1..1 (inner), in the frame and
 *     filterable only: cw = c3[dy + 1] * c3[dx + 1] with c3 = {1/4, 1/2, 1/4}, gsum += v_k[q] * cw, cwsum += cw;
 *     g = gsum * (1.0f / cwsum);  den = sl2 * g + var_floor.
 *     The 25 taps q = p + s (dx, dy) in pt_denoise's order and with its skips:  w = ((h[dy + 2] * h[dx + 2]) * wn) * wz;
 *     dl = lum(x_k[p]) - lum(x_k[q]);  w = w * (den / (den + dl * dl));
 *     sum += x_k[q] * w per channel, vsum += v_k[q] * (w * w), wsum += w.
 *     r = 1.0f / wsum;  x_{k+1}[p] = sum * r;  v_{k+1}[p] = vsum * (r * r).
 *   out = x_last * a' for filterable pixels, x_last otherwise; out_variance = v_last (of the demodulated luminance). */
int pt_denoise_variance(pt_scene* scene, const pt_vdenoise_params* d, const float* color, const float* albedo,
                        const float* normal, const float* depth, const float* moments, const float* hist_len, float* out,
                        float* out_variance, int on_device, void* hip_stream);
/* The same per-pixel source (csrc/pt_denoise.h) compiled for the HOST: needs no GPU and no scene. */
int pt_denoise_variance_host(const pt_vdenoise_params* d, const float* color, const float* albedo, const float* normal,
                             const float* depth, const float* moments, const float* hist_len, float* out, float* out_variance);

/* Temporal gradients: a history that follows light and material changes — an EXTENSION: off unless called, never part of a
 * parity or roofline number, no other entry point's output changes by a bit.  DESIGN.md §21.
 *   pt_temporal_accumulate* reject history on depth and normal only, so after pt_scene_update(PT_UPDATE_SHADING) the old lighting
 *   stays in the image for up to max_history frames.  A pixel's samples depend only on (pixel index, seed, sample_offset,
 *   stream_stride), so pt_render with the PREVIOUS frame's parameters and a row selection, on the CURRENT scene, re-traces a
 *   sparse set of the previous frame's samples with the same random numbers: where nothing that the paths of a pixel touch has
 *   changed the result is the previous frame's, bit for bit.  pt_temporal_gradient turns the difference into a map lambda in
 *   [0, 1] per tile of stride x stride pixels; pt_temporal_accumulate_adaptive drops that share of a pixel's history.
 *   fp32, operations in the order written, no contraction, IEEE division. */
typedef struct pt_gradient_params {
    int32_t width, height;   /* full frame */
    int32_t stride;          /* 0 -> 3; else 1..16: strata of stride x stride pixels, one sampled row each */
    int32_t iterations;      /* 0 -> 3; else 1..8 */
    float   gain;            /* 0 -> 2; else > 0, finite */
    float   norm_floor;      /* 0 -> 1e-6; else > 0, finite */
} pt_gradient_params;        /* 24 bytes */

/* Grid.  With s = stride: r0 = s / 2, TW = (W + s - 1) / s, TH = (H - r0 + s - 1) / s; tile (ty, tx) holds the pixels of rows
 * s ty .. s ty + s - 1 and columns s tx .. s tx + s - 1 that are in the frame, and its sampled row is r0 + s ty.  H <= r0:
 * PT_ERR_INVALID_ARG.
 * prev_color [H, W, 3]: the previous frame's own noisy pt_render output (not an accumulated one).  resampled [TH, W, 3]: what
 * pt_render / pt_render_async writes for the previous frame's parameters with row_begin = r0, row_end = H, row_stride = s on
 * the current scene.  lambda_out [TH, TW].  on_device != 0: device pointers, 1 + iterations kernels are enqueued on hip_stream
 * without a host sync; on_device == 0: host pointers, blocking, staged through memory of the handle.  The handle owns two
 * ping-pong buffers of 32 bytes per tile, allocated on first use, grown when a larger frame arrives, freed with the scene.
 * A NULL pointer, a parameter out of range: PT_ERR_INVALID_ARG, pt_last_error() names the argument or field.
 *   Reduce, tile (ty, tx): y = r0 + s ty; a = b = 0 per channel; for x = s tx .. min(W, s tx + s) - 1 in increasing order
 *     a_c += prev_color[y, x, c], b_c += resampled[ty, x, c];  d_c = b_c - a_c, m_c = a_c < b_c ? b_c : a_c;
 *     x_0 = (d_r, d_g, d_b, m_r, m_g, m_b).
 *   Filter, k = 0 .. iterations - 1, spacing 1 << k on the tile grid, unguided, with pt_denoise's h = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *     sum = 0 (six components), wsum = 0; taps q = t + (dx, dy) << k, dy = -2..2 (outer), dx = -2..2 (inner); a tap outside the
 *     grid is skipped and no address is formed for it; w = h[dy + 2] * h[dx + 2], sum += x_k[q] * w, wsum += w;
 *     x_{k+1}[t] = sum * (1.0f / wsum).
 *   Final, on x_iterations: r_c = fabsf(d_c) / max(m_c, norm_floor), r = max(max(r_r, r_g), r_b), lambda = min(gain * r, 1.0f).
 *   Non-finite input propagates; what it does is unspecified.
 *   A property callers may rely on: prev_color equal to resampled on every sampled row gives lambda == +0 (the bits) at every
 *   tile — and pt_temporal_accumulate_adaptive then is pt_temporal_accumulate_moments. */
int pt_temporal_gradient(pt_scene* scene, const pt_gradient_params* g, const float* prev_color, const float* resampled,
                         float* lambda_out, int on_device, void* hip_stream);
/* The same per-tile source (csrc/pt_gradient.h) compiled for the HOST: needs no GPU and no scene. */
int pt_temporal_gradient_host(const pt_gradient_params* g, const float* prev_color, const float* resampled, float* lambda_out);

/* The sparse variant: one re-traced PIXEL per tile in place of a row, 1 / s^2 of the previous frame's paths instead of 1 / s.
 * DESIGN.md §22.  The grid — s, r0, TW, TH, tile t = ty * TW + tx — is pt_temporal_gradient's, so lambda_out [TH, TW] feeds
 * pt_temporal_accumulate_adaptive as it is; field checks and their messages are pt_temporal_gradient's.
 *   pt_gradient_pixels writes pixels_out [TH * TW]: the pixel of every tile at `seed` (callers pass the frame number, so that
 *   the sampled pixel of a tile moves from frame to frame).  All arithmetic in uint32, wrapping:
 *     v = t * 747796405 + (seed * 2891336453 + 1);  w = ((v >> ((v >> 28) + 4)) ^ v) * 277803737;  h = (w >> 22) ^ w;
 *     ox = (h & 0xffff) % s, oy = (h >> 16) % s;  x = min(s tx + ox, W - 1), y = min(s ty + oy, H - 1);  pixels_out[t] = y * W + x.
 *   Every tile of the grid has at least pixel (s tx, s ty) inside the frame.  on_device != 0: a device pointer, one kernel
 *   enqueued on hip_stream without a host sync; on_device == 0: a host pointer, blocking.
 *   resampled [TH * TW, 3] is what pt_render_pixels writes for the previous frame's parameters and this list on the current
 *   scene; prev_color [H, W, 3] as in pt_temporal_gradient.
 *   Reduce, tile t: e = pixels[t]; a_c = prev_color[3 e + c], b_c = resampled[3 t + c]; d_c = b_c - a_c, m_c = a_c < b_c ? b_c : a_c;
 *     x_0 = (d_r, d_g, d_b, m_r, m_g, m_b).  An entry outside [0, W * H) forms no address and that tile takes a = b (in both
 *     call forms and in the host twin).
 *   Filter and Final: pt_temporal_gradient's, unchanged; 1 + iterations kernels on the same ping-pong buffers of the handle.
 *   Call forms, staging and errors as in pt_temporal_gradient; pt_last_error() names pixels_out, prev_color, pixels, resampled
 *   or lambda_out.
 *   A property callers may rely on: prev_color equal to resampled at every listed pixel gives lambda == +0 (the bits) at every
 *   tile. */
int pt_gradient_pixels(pt_scene* scene, const pt_gradient_params* g, uint32_t seed, int32_t* pixels_out, int on_device, void* hip_stream);
int pt_temporal_gradient_sparse(pt_scene* scene, const pt_gradient_params* g, const float* prev_color, const int32_t* pixels,
                                const float* resampled, float* lambda_out, int on_device, void* hip_stream);
/* The same per-tile source (csrc/pt_gradient.h) compiled for the HOST: need no GPU and no scene. */
int pt_gradient_pixels_host(const pt_gradient_params* g, uint32_t seed, int32_t* pixels_out);
int pt_temporal_gradient_sparse_host(const pt_gradient_params* g, const float* prev_color, const int32_t* pixels,
                                     const float* resampled, float* lambda_out);

/* pt_temporal_accumulate_moments with pt_temporal_gradient's map.  Buffers, call forms, aliases, staging and errors are
 * pt_temporal_accumulate_moments'.  lambda [TH, TW] and stride (0 -> 3; else 1..16) are the map and the stride of the
 * pt_temporal_gradient call for the same frame size; lambda == NULL, a stride out of range, H <= r0: PT_ERR_INVALID_ARG,
 * pt_last_error() names lambda, stride or height.  With no history lambda is never read.
 *   The rule per pixel p: steps 1-7 of pt_temporal_accumulate_moments unchanged.  In step 8 (wsum > 0), after n:
 *     a0 = 1.0f / n;  jx = (int)floorf(motion.x) clamped to [0, W - 1], jy = (int)floorf(motion.y) clamped to [0, H - 1];
 *     tx = jx / s, ty = min(jy / s, TH - 1);  l = lambda[ty * TW + tx];  L = l > 1.0f ? 1.0f : l  (min; a NaN stays a NaN).
 *     L > 0:  a = a0 + L * (1.0f - a0);  out = h + (c - h) * a, out_moments = mh + (m_c - mh) * a, out_len = 1.0f / a.
 *     Otherwise (L is 0, negative or NaN): every output of the pixel is pt_temporal_accumulate_moments', bit for bit.
 *   L == 1 gives a == 1: out = h + (c - h), out_len = 1 — the history is dropped up to one rounding. */
int pt_temporal_accumulate_adaptive(pt_scene* scene, const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io,
                                    const float* lambda, int32_t stride, int on_device, void* hip_stream);
/* The same per-pixel source (csrc/pt_temporal.h) compiled for the HOST: needs no GPU and no scene. */
int pt_temporal_accumulate_adaptive_host(const pt_temporal_params* t, float albedo_floor, const pt_temporal_io* io,
                                         const float* lambda, int32_t stride);

/* What do these rays hit: picking, occlusion and visibility probes, baking, a caller's own light sampling.  DESIGN.md §24.
 *   rays: n x {org[3], dir[3], tnear, tfar} (pt_debug_intersect's layout).  traversal: PT_TRAVERSAL_* as in pt_debug_intersect,
 *   PT_TRAVERSAL_DEFAULT = exact.  The tree is the one a render traverses: option "fast_tree" is honoured.
 *   PT_QUERY_CLOSEST: out_tuv [n, 3] and out_prim [n] hold exactly what pt_debug_intersect writes — {t, u, v} and the shape id of
 *     the closest hit inside (tnear, tfar), -1 and zeros on a miss; ties on t go to the primitive the caller's tree visits
 *     first, rays with a zero direction component are traced on the caller's tree.
 *   PT_QUERY_ANY: out_prim[k] = 1 if any primitive test of ray k succeeds inside its interval, else 0 — by definition
 *     (closest prim >= 0) of the same ray; the ray stops at its first hit.  out_tuv may be NULL and is not written.
 *   on_device != 0: device pointers, enqueued on hip_stream (NULL = the default stream) without a host sync; the results are
 *     written in stream order, and `rays` must stay valid until the stream has passed the call.
 *   on_device == 0: host pointers, blocking; staged through memory of the handle that grows on demand and is freed with it.
 *   PT_ERR_INVALID_ARG, pt_last_error() naming the argument: n < 0, n > 2^30, an unknown mode or traversal, and with n > 0 a
 *   NULL rays or out_prim, or PT_QUERY_CLOSEST with a NULL out_tuv.  n == 0: PT_OK, nothing is written.
 * The kernel (csrc/pt_query.h): a fixed grid of waves works through the rays; a lane whose ray is finished takes the next one,
 * so a ray that walks hundreds of nodes holds up one lane, not a wave.  A wave works through ranges of 64 ray indices (info
 * "query_chunk"): the first is its own, every further one it reserves with one atomic add on the launch's work counter.  Results
 * are stored and rays handed out when 16 lanes of a wave are idle (option "query_refill", 1 .. 64; 0 = that default).  Every
 * launch takes the next of 64 counters the handle rotates through (the ring's size), so launches in flight on different streams
 * never share one; the 65th launch waits, on its stream, for the launch that had its counter.  The call reads scene memory only, takes no frame slot and leaves pt_get_counters, pt_get_frame_times and info
 * "trace_variant" as they were; pt_scene_update and pt_scene_transform synchronise the device before they write. */
enum { PT_QUERY_CLOSEST = 0, PT_QUERY_ANY = 1 };
int pt_trace_rays(pt_scene* scene, const float* rays, int32_t n, int mode, int traversal,
                  float* out_tuv, int32_t* out_prim, int on_device, void* hip_stream);

int pt_get_counters(pt_scene* scene, pt_counters* out);   /* synchronises the scene's last stream */

/* HIP-event times of the last render calls on the scene, oldest first: kernel_ms[k] / resolve_ms[k] of up to max_frames calls,
 * *n_out of them written.  The library keeps the events of the last "timing_frames" calls (option, default 1), so a caller
 * may enqueue many frames on a stream without a host sync in between and read every frame's kernel time afterwards
 * (bench.py's timed loop).  Synchronises the scene's last stream. */
int pt_get_frame_times(pt_scene* scene, int max_frames, double* kernel_ms, double* resolve_ms, int* n_out);

/* BVH construction on the device — an alternative producer of `pt_scene_desc.nodes` to the host's
 * construct_bvh (bvh.cu:16-54: object-median split, O(N log^2 N), 10-57 s start-up in README.md:123,132).
 *   PT_BVH_DEVICE_LBVH  Morton order + Karras hierarchy
 *   PT_BVH_DEVICE_SAH   Morton order + per-node surface-area-cost cut, top-down
 * desc->nodes / desc->root are ignored.  out_nodes receives 2*num_shapes-1 nodes in the reference's layout (HOST
 * memory: the same array can be handed to pt_scene_create and to a CPU checker); *out_root the root's index;
 * *out_depth (optional) the depth with leaves counting 1 (computeMaxDepth, bvh.cu:56-65); *out_build_ms (optional)
 * the device time from primitive boxes to finished nodes (uploads and the copy back to the host excluded).
 * Such trees visit fewer nodes per ray than the reference's; closest hits — and so images — are the same except where
 * two primitives tie on t (the first one VISITED wins, scene.h:270).  Parity and roofline numbers use the reference tree.
 * Depth: PT_BVH_DEVICE_SAH caps its tree at min(48, max(8, ceil(log2 N) + 5)) levels, always within the reference's 64-entry
 * stack (scene.h:251).  PT_BVH_DEVICE_LBVH has no cap: the hierarchy of 63-bit codes plus a run of equal codes can be deeper
 * than 64 levels for adversarial input (centroids a factor of two apart on every level).  The call still returns PT_OK, the
 * complete tree and its true depth in *out_depth; pt_scene_create accepts a caller's tree of up to 64 levels and rejects a
 * deeper one with PT_ERR_BAD_SCENE in host code, before anything is launched — check *out_depth, or build with PT_BVH_DEVICE_SAH. */
enum { PT_BVH_DEVICE_LBVH = 0, PT_BVH_DEVICE_SAH = 1 };
int pt_bvh_build_device(const pt_scene_desc* desc, int method, pt_bvh_node* out_nodes, int32_t* out_root,
                        int32_t* out_depth, double* out_build_ms);

/* The builder behind the library's internal tree (pt_scene_create), exposed so that the tree can be inspected, checked by
 * a CPU oracle, or handed in as the caller's own: top-down, every cut along x, y and z considered at every node,
 * smallest  SA(left) n_left + SA(right) n_right  wins.  Runs on the HOST (no GPU needed), deterministic.
 * Input: the LEAF boxes of desc->nodes (one leaf per shape; the inner nodes of desc are ignored).  Output as for
 * pt_bvh_build_device; out_build_ms = host wall time.  The tree may be deeper than the reference's 64-entry stack
 * allows (scene.h:251) for adversarial input — *out_depth tells; pt_scene_create rejects such a tree as a CALLER's. */
int pt_bvh_build_sweep(const pt_scene_desc* desc, pt_bvh_node* out_nodes, int32_t* out_root, int32_t* out_depth,
                       double* out_build_ms);

/* The same builder run on the GPU (csrc/pt_sweep_build.hip: level-synchronous segmented scans and reductions): the SAME tree,
 * byte for byte — pt_scene_create uses it from 4,096 shapes up.  out_build_ms = device time (sorts to finished nodes, without the
 * upload of the leaf boxes and the copy back).  PT_ERR_UNSUPPORTED for input that runs into the host builder's depth guard
 * (2 log2 n + 16 levels): only the host builder holds the median-cut fallback for such branches. */
int pt_bvh_build_sweep_device(const pt_scene_desc* desc, pt_bvh_node* out_nodes, int32_t* out_root, int32_t* out_depth,
                              double* out_build_ms);

/* Tuning knobs (all optional; none of them changes a bit of the rendered image):
 *   "kernel"        2 (default) decoupled traversal/shading scheduler, 1 segment-synchronous wavefront kernel, 3 paths regrouped
 *                   across the waves of a workgroup through LDS rings (csrc/pt_kernel_q.h; exact traversal without PT_RENDER_NEE,
 *                   anything else runs on 2; "q_target" / "q_swap" / "q_low" are its schedule knobs, 0 = automatic)
 *   "v2_thresh" / "v2_inner" / "v2_minw"   scheduler variant of kernel 2; 0 = automatic (by scene residency).
 *                   v2_inner: < 0 vote burst of -n steps; 1..9 n inner steps + 1 leaf step per burst; >= 100 encodes
 *                   rounds*100 + inner*10 + leaf steps (162 = 6 inner + 2 leaf steps); 1000 + burst = the same burst with
 *                   leaves set aside and tested together (internal tree only).  Only compiled-in variants are
 *                   accepted (PT_ERR_INVALID_ARG otherwise); every variant renders the same bits.
 *   "reg_stack"     1 (default) trace_kernel_v2 keeps the traversal stack of a lane in one register instead of an LDS column
 *                   where that is possible: an LDS-resident scene of triangles with diffuse materials on its automatic
 *                   schedule ("v2_thresh" and "v2_inner" 0; "v2_minw" 0, 5 or 6), traversed on the internal tree, whose tree
 *                   holds at most 4 stack entries ("stack_entries" <= 5) with at most 126 inner nodes and 127 primitives,
 *                   rendered without PT_RENDER_NEE and outside the later rounds of pt_render_adaptive.  0 = always the LDS
 *                   stack.  Same nodes, same leaves, same order: the same bits.  Info "reg_stack" reports the last launch.
 *   "leaf_sweep"    1 (default) a launch that "reg_stack" admits, with exact traversal, without "stats", on a scene of at most 64
 *                   primitives staged with its octant tables ("residency" 2), finds the leaves a segment tests without the
 *                   tree: the leaves of the internal tree are grouped by the bit pattern of their boxes at pt_scene_create
 *                   (info "sweep_boxes": the number of groups; at most 32 are admitted), every group's box is tested once when
 *                   the segment starts, and a lane keeps one hit bit per group; a group's primitives are tested along a chain
 *                   of records the block stages in place of the octant tables (trace_kernel_v2_sweep).  Exact traversal
 *                   tests a leaf iff the ray hits the leaf's own box (see "fast_tree"), so the same leaves are tested and the
 *                   frame is the same, bit for bit.  0 = always the tree.  A handle whose geometry was updated keeps to the
 *                   tree.  Info "leaf_sweep" reports the last launch; node visits ("stats") always count the tree's.
 *   "sweep_pairs"   1 (default) a "leaf_sweep" launch tests its groups two by two in an order made at pt_scene_create: two
 *                   groups whose boxes have the same interval on an axis (both floats equal bit for bit; -0.0 is not +0.0)
 *                   share that axis's slab products, and where the interval is flat (min == max) one product serves as near
 *                   and far of both (csrc/pt_sweep_pairs.h).  0 = the groups in the order the tree lists them, every pair
 *                   computed in full.  The same operations on the same operands either way: the same bits.  Info
 *                   "sweep_share_pairs", "sweep_flat_pairs" (each also with _x, _y, _z for one axis) and "sweep_general_pairs"
 *                   report the pairs of each kind a sweep launch of the handle runs under the option as it stands.
 *   "sweep_families" under "sweep_pairs" 1: 1 (default) one more kind of record stands in front of the pairs
 *                   (csrc/pt_sweep_families.h): PAIR2, two groups with the same interval on TWO axes (each of them flat or
 *                   not), both axes computed once.  Which groups go into which record is chosen at pt_scene_create (and
 *                   again by pt_scene_rebuild) so that a count of the sweep's vector instructions is smallest; never above
 *                   the count of the pairs alone.  0 = the pairs alone, exactly as before the records existed (A/B runs,
 *                   tests).  The same bits under either value.  Info "sweep_pair2_records" reports the records of a sweep
 *                   launch under the options as they stand, and "sweep_valu_model" that count (general pair 35, pair
 *                   sharing an axis 31, flat 29, single 17, PAIR2 27 / 25 / 23 with 0 / 1 / 2 flat axes).  In
 *                   "sweep_share_pairs" and "sweep_flat_pairs" a PAIR2 counts as one pair (flat where one of its axes is);
 *                   with _x, _y, _z it counts under each of the two axes it shares.
 *   "sweep_self_skip" 1 (default) a "leaf_sweep" launch leaves out leaf tests that cannot keep a hit: a bounce that starts on a
 *                   triangle whose group has a box flat on an axis (an axis-aligned wall), with the new origin's coordinate on
 *                   that axis equal to the plane's as floats, does not test the triangles of that plane: the group it left
 *                   and every other group flat on the same axis at the same coordinate (csrc/pt_sweep_skip.h has the
 *                   argument: such a test computes t = +-0 or NaN and is rejected whatever the direction).  Camera rays and
 *                   origins off the plane by as little as one ulp test every group the sweep hits.  0 = every group the
 *                   sweep hits is tested (A/B runs, tests).  The same bits under either value.  Info "sweep_skip_groups"
 *                   reports the groups that can be skipped under the options as they stand, "sweep_skip_planes" the
 *                   distinct planes (axis, coordinate) they lie on; both 0 under option 0 or without sweep tables.
 *   "octants"       1 (default) keep 8 ray-octant node tables in LDS for very small scenes, 0 = one table
 *   "fast_tree"     1 (default) traversal (exact and pruned) on the library's INTERNAL tree where pt_scene_create kept one,
 *                   0 = on the caller's tree.  Same image either way, bit for bit: the reference never prunes, so a leaf is tested iff the
 *                   ray hits the leaf's own box (nested boxes) — any tree over the caller's leaf boxes tests the same leaves;
 *                   ties on t are settled in the caller's visit order (one box test at the node of the caller's tree where
 *                   the two leaves' paths part), rays with a zero direction component are traced on the caller's tree.  The
 *                   internal tree (pt_bvh_build_sweep) is kept when probe rays visit >= 10 % fewer nodes in it, the caller's
 *                   boxes nest, and the scene has 16+ primitives.  DESIGN.md §12.
 *   "top_cache"     1 (default) scenes read from global memory keep the most-visited top nodes of the tree in LDS, 0 = all from memory
 *   "lds_budget_kb" LDS per block for traversal stacks + that cache (0 = 26: 6 resident blocks per CU)
 *   "chunk"         work items a wave reserves per atomic, 64..256 (0 = automatic: 128 for big launches)
 *   "xcd_regions"   0 (default) 8 row bands with XCD affinity, 1 = a single work queue
 *   "item_order"    1 (default) a band is worked through row by row (all samples of a row first), 0 = sample by sample
 *   "force_global"  1 = never stage the scene in LDS
 *   "blocks_per_cu" persistent blocks per CU (0 = occupancy query; at most 32)
 *   "query_blocks"  blocks of a query launch (pt_trace_rays, pt_render_guides_async): 0 (default) = resident blocks per CU (an
 *                   explicit "blocks_per_cu" as given) x CUs, and no more than give every lane a ray; 1 .. 4096 = exactly that
 *                   many (and pt_render_guides_async then takes the refilling kernel).  Same results whatever the grid.
 *   "query_refill"  idle lanes from which a wave of the query kernel stores results and hands out rays, 1 .. 64 (0 = 16)
 *   "query_guides"  the kernel of pt_render_guides_async: 0 (default) automatic, 1 refilling, 2 one-shot (see there)
 *   "timing_frames" render calls whose HIP events are kept for pt_get_frame_times (0 .. 4096, default 1).  0 = no timing events
 *                   at all (pt_counters.kernel_ms / resolve_ms read 0): four event records less per frame, which an interactive
 *                   loop of 2-spp frames feels (cbox 640x480, host sync per frame: 3,250 -> 3,540 frames/s; scene1 5,300 -> 6,110)
 *   "frames_in_flight" 1 .. 4 (default 2): sets of per-frame scratch memory (per-sample buffer, work and statistics counters)
 *                   the handle rotates through; with more than one, consecutive render calls overlap as described at
 *                   pt_render_async (frames that need several sample passes, and frames that find the GPU idle, run on the
 *                   caller's stream as with 1).  A frame that overlaps leaves its successor room on every CU: all but one of
 *                   the resident blocks with 2 slots (never slower than 1 slot, whatever the caller's submission pattern),
 *                   half of them with 3 or 4 (the fastest for an unbroken stream of frames — bunny 4.41 ms per frame against
 *                   4.52 with 2 and 4.91 with 1 — but a burst that ends leaves its last frame on half a chip);
 *                   an explicit "blocks_per_cu" is used as given.
 *                   kernel_ms of a frame that overlapped with its neighbours includes the time its blocks waited for theirs.
 *   "scratch_bytes" cap of the per-sample scratch buffer (0 = 8 GiB); larger jobs run in sample passes
 *   "stats"         1 = also count node visits / leaf tests (pt_counters), schedule diagnostics ("diag0".."diag7") and the
 *                   launch timeline ("diag8".."diag15", 10-ns ticks; "diag16".."diag271" per-wave histograms; tools/gpu_diag.py)
 * pt_scene_get_info keys: "grid", "lds_bytes", "lds_scene", "residency" (0 global, 1 LDS, 2 LDS + octant tables, 3 global + top of the tree in LDS), "top_nodes",
 * "passes", "occupancy", "blocks_per_cu", "num_cus", "bvh_depth", "scene_bytes", "num_inner_nodes", "device", "vgprs", "vgprs_pruned",
 * "fast_tree" (an internal tree exists), "fast_tree_on" (the next render uses it), "fast_tree_is_callers" (it is the caller's own
 * topology in internal form: the sweep tree did not win the probe), "fast_tree_depth",
 * "fast_tree_cost_permille" (probe-ray node visits, internal / caller's x 1000; 0 = none built), "stack_entries" (per lane),
 * "prev_geometry", "redo_segments" (with "stats": segments of the last frame traced on the caller's tree), "debug_reruns" (same for pt_debug_intersect),
 * "kernel" / "block_threads" (what the last render ran on), "trace_variant" (the template arguments of the trace kernel that call
 * launched last — for pt_render_adaptive the LIST kernel of its last round, for pt_render_pixels a LIST kernel; 0 = none launched — packed into one value:
 *     bits  0-3  family: 1 trace_kernel, 2 trace_kernel_v2, 3 trace_kernel_q      bit  10  NEE
 *     bits  4-5  RES (family 1: LDS_SCENE)                                      bit  11  LIST
 *     bit   6    PRUNE       bit 7  STATS       bits 8-9  SPEC                    bit  12  POSTPONE
 *     bit  13    the traversal state of a lane is a register (trace_kernel_v2_reg: the trace_kernel_v2 of the other fields with
 *                the stack in a register; info "leaf_sweep" says which body ran: 0 that one, 1 trace_kernel_v2_sweep, which
 *                stands in for it with the same fields, "reg_stack", "path_bank" and "lds_bytes")
 *     bits 16-23 THRESH      bits 24-39 INNER, 16-bit two's complement          bits 40-43 MINW
 *   a field the family's template does not have is 0), "path_bank" (1 = that kernel handed out path starts from a per-wave
 * register bank filled 64 at a time: trace_kernel_v2 on LDS-resident scenes of triangles with diffuse materials),
 * "reg_stack" (1 = that kernel kept its traversal stack in a register, see option "reg_stack"; "lds_bytes" of such a launch has no
 * stack columns), "leaf_sweep" (1 = that kernel found its leaves by the box sweep, see option "leaf_sweep"), "sweep_boxes",
 * "sweep_share_pairs", "sweep_flat_pairs", "sweep_general_pairs" (see option "sweep_pairs"),
 * "sweep_pair2_records", "sweep_valu_model" (see option "sweep_families"),
 * "sweep_skip_groups", "sweep_skip_planes" (see option "sweep_self_skip"),
 * "frames_in_flight", "sweep_on_device" (the internal tree was built on the GPU), "query_chunk" (ray indices a wave of the query
 * kernel reserves per atomic), "query_grid" (blocks of the last query launch), "query_guides" (the last pt_render_guides_async
 * ran on the refilling kernel: 1, or the one-shot kernel: 0),
 * "create_us0".."create_us6" (wall microseconds of pt_scene_create: total, primitive records, caller's tree checked and re-laid,
 * internal tree built, ... re-laid, uploads + probe, tie tables). */
int pt_scene_set_option(pt_scene* scene, const char* key, int64_t value);
int pt_scene_get_info(pt_scene* scene, const char* key, int64_t* value);
/* Environment variables the library reads (A/B runs and debugging; results are the same whatever they say):
 *   PT_SWEEP_BUILD=host              pt_scene_create prepares big scenes on the host as in round 2 (default: on the device from 4,096 shapes)
 *   PT_SWEEP_SCANS=rocprim           the device sweep builder's box scans as rocPRIM scans-by-key (default: tiled)
 *   PT_SLOT_STREAM_PRIORITY=normal|high   priority of the handle's own streams (default: lowest) */

/* Deterministic fp32 helpers evaluated ON THE DEVICE, exported so tests can
 * pin device arithmetic against the CPU oracle bit-for-bit.
 * op: 0 sincos(x)->(out0=sin,out1=cos)   1 powf(x,y)->out0
 *     2 pcg32: stream = bit pattern of x, seed = bit pattern of y -> first two float draws */
int pt_debug_math(int op, const float* x, const float* y, float* out0, float* out1, int n);
/* Same functions (the very same source, csrc/pt_math.h) evaluated by the HOST half of the
 * library: lets CPU-only tests pin the shared arithmetic header without a GPU. */
int pt_debug_math_host(int op, const float* x, const float* y, float* out0, float* out1, int n);

/* The exact short sequences of csrc/pt_math.h (rcp_exact, div_pi_exact, sqrt_exact) evaluated ON THE DEVICE
 * against the IEEE expressions they replace, over the fp32 bit patterns begin .. begin + count - 1
 * (begin + count <= 2^32).  op: 0 rcp_exact(x) vs 1.0f / x   1 div_pi_exact(x) vs x / pi   2 sqrt_exact(x) vs sqrtf(x)
 *     3 the bare hardware reciprocal vs 1.0f / x (a control for the checker: it is not correctly rounded).
 * out: number of inputs whose result bits differ, and the first such bit pattern (-1 if none). */
int pt_debug_exact_math(int op, uint32_t begin, uint64_t count, uint64_t* mismatches, int64_t* first_mismatch);

/* Closest-hit query for explicit rays (tests / per-ray KATs).
 * rays: n x {org[3], dir[3], tnear, tfar}; out: n x {t,u,v} and prim id (-1 = miss). */
int pt_debug_intersect(pt_scene* scene, const float* rays, int n, int traversal,
                       float* out_tuv, int32_t* out_prim);

const char* pt_last_error(void);
int pt_api_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_API_H */
