/*
 * capsaicin_hip.h — C ABI of the MI355X (gfx950) wavefront path tracer: the device-side drop-in for the
 * reference's RaytracingSystem + BLAS/TLAS systems.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Each entry point names the reference interface it replaces (paths relative to /root/reference/src/core).
 * All functions return CAP_OK (0) or a CapStatus error; cap_last_error() gives the thread-local message.
 * No exception crosses this boundary.  A context is single-threaded (the reference runs every system on the
 * UI thread, capsaicin.cpp:38-45, main.cpp:17-19); use one context per GPU.
 * Host pointers are borrowed for the duration of the call only.  Pointers documented as "device" must be
 * device-accessible on the context's GPU.
 */
#ifndef CAPSAICIN_HIP_H
#define CAPSAICIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CapContext CapContext;

typedef enum CapStatus
{
    CAP_OK                = 0,
    CAP_ERR_INVALID_ARG   = 1,
    CAP_ERR_HIP           = 2, /* a HIP runtime call failed (no GPU, out of memory, ...) */
    CAP_ERR_STATE         = 3, /* call order violated (e.g. render before bvh_build) */
    CAP_ERR_UNSUPPORTED   = 4,
    CAP_ERR_IO            = 5
} CapStatus;

/* CameraData, src/systems/camera_system.h:16-31 == shaders/data_payload.h:7-18 (72 bytes). */
typedef struct CapCameraData
{
    float position[3];
    float focal_length;
    float right[3];
    float znear;
    float forward[3];
    float focus_distance;
    float up[3];
    float aperture;
    float sensor_size[2];
} CapCameraData;

/* MeshComponent, src/systems/asset_load_system.h:29-39 == shaders/data_payload.h:20-30 (32 bytes). */
typedef struct CapMeshDesc
{
    uint32_t vertex_count;
    uint32_t first_vertex_offset;
    uint32_t index_count;
    uint32_t first_index_offset;
    uint32_t index;
    uint32_t texture_index; /* MeshComponent::material_index; ~0u = untextured */
    uint32_t padding[2];
} CapMeshDesc;

/* EXT (no reference counterpart): per-mesh material for CAP_RENDER_EXT_MATERIALS. */
typedef struct CapMaterial
{
    float kd[3];
    float roughness; /* GGX alpha = max(roughness^2, 1e-3): only the square enters; values above 1 are legal and are not Lambert */
    float ks[3];
    float pad0;
    float ke[3];
    float pad1;
} CapMaterial;

/* cap_render flags */
enum
{
    CAP_RENDER_AOV           = 1u << 0, /* keep the per-frame planes of the LAST frame for cap_readback */
    CAP_RENDER_EXT_MATERIALS = 1u << 1, /* EXT shading model (materials uploaded with cap_materials_upload) */
    CAP_RENDER_STAGE_TIMERS  = 1u << 2, /* bracket every kernel with hipEvents (fills CapStats::ms_<stage>) */
    /* RaytracingOptions::gbuffer_feedback (raytracing_system.h:26, rt_indirect.hlsl:116-145): a path vertex of bounce >= 1
     * that the previous frame saw takes that frame's cap_post_frame output and ends the path.  One frame per call, reference
     * shading model (sharded contexts: cap_feedback_export / _import carry the previous output to every rank); needs
     * cap_prev_camera_set and cap_post_frame after every frame. */
    CAP_RENDER_GBUFFER_FEEDBACK = 1u << 3,
    /* RaytracingOptions::lowres_indirect (raytracing_system.h:24; LOWRES_INDIRECT, rt_indirect.hlsl:53-59): only the pixel at
     * sp_offset = ((frame % 4) / 2, (frame % 4) % 2) of every 2x2 block gets an indirect sample.  One frame per call, even width
     * and height, reference shading model; the frame is not added to the accumulation buffer.  Read the
     * (W/2, H/2) image with CAP_BUF_INDIRECT_LOWRES or hand it to cap_post_frame (settings.lowres_indirect = 1). */
    CAP_RENDER_LOWRES_INDIRECT = 1u << 4
};

/* cap_readback kinds: the reference's RaytracingSystem outputs (raytracing_system.h, cpp:466-575). */
typedef enum CapBufferKind
{
    CAP_BUF_GBUFFER_GEO  = 0, /* rt_primary_visibility.hlsl:46  (u, v, asfloat(instance), asfloat(prim)) */
    CAP_BUF_DIRECT       = 1, /* rt_direct_lighting.hlsl:78      output_direct_                           */
    CAP_BUF_ALBEDO       = 2, /* rt_direct_lighting.hlsl:79      gbuffer_albedo_                          */
    CAP_BUF_NORMAL_DEPTH = 3, /* rt_direct_lighting.hlsl:80      gbuffer_normal_depth_                    */
    CAP_BUF_INDIRECT     = 4, /* rt_indirect.hlsl:176            output_indirect_                         */
    CAP_BUF_COMBINED     = 5, /* combine_illumination.hlsl:29    indirect*albedo + direct (xyz; w = 1)    */
    CAP_BUF_ACCUM_SUM    = 6, /* running fp32 sum of COMBINED over all frames since cap_accum_reset (w = frames) */
    CAP_BUF_ACCUM_MEAN   = 7, /* ACCUM_SUM / frames                                                       */
    CAP_BUF_INDIRECT_LOWRES = 8 /* output_indirect_ of a CAP_RENDER_LOWRES_INDIRECT frame: (width/2)*(height/2)*4 floats */
} CapBufferKind;

/* Per-stage names follow the reference's timestamp labels (raytracing_system.cpp:1024, 1099, 1207). */
typedef struct CapStats
{
    uint64_t rays_primary;   /* rays actually traced since the last cap_stats_reset */
    uint64_t rays_extension;
    uint64_t rays_shadow;
    uint64_t shaded_vertices;
    uint64_t frames;
    double   ms_total;          /* GPU time of cap_render calls (hipEvent, context stream) */
    double   ms_primary;        /* "RaytracePrimaryVisibility" (fused small-scene path: + shading of the camera vertex) */
    double   ms_trace_closest;  /* extension-ray traversal ("RT Indirect diffuse"; fused small-scene path: + shading) */
    double   ms_trace_any;      /* shadow-ray traversal */
    double   ms_shade;          /* shading / BSDF sampling / compaction */
    double   ms_resolve;        /* radiance accumulate */
    uint64_t launches_trace_closest;
    uint64_t launches_trace_any;
    uint64_t launches_shade;   /* 0 when the small-scene path fuses shading into the closest-hit kernel */
    uint64_t rays_extension_bounce0; /* extension / shadow rays emitted by the bounce-0 (camera-vertex) kernel */
    uint64_t rays_shadow_bounce0;
    uint64_t guard_shade;     /* malformed queue entries caught by the kernels' bounds guards: always 0 in a correct run */
    uint64_t guard_trace_any;
    uint64_t guard_last;      /* (queue index or bounce) << 32 | path id of the last offender */
    double   ms_post;         /* reconstruction chain, "Spatial gather" .. "TAA" (cap_post_frame), always timed */
    uint64_t post_frames;
    /* The reference's remaining timestamp labels (gui_system.cpp:94-104 lists what AllocateTimestampQueryPair named). */
    double   ms_direct;       /* "RT Direct lighting": shading of the camera vertex + its shadow rays (part of ms_primary on the fused
                                 small-scene path, of ms_shade / ms_trace_any otherwise; CAP_RENDER_STAGE_TIMERS) */
    double   ms_post_pass[5]; /* "Spatial gather", "Temporal upscale", "EAW", "Combine illumination", "TAA" (sum = ms_post) */
    /* Shadow rays that were stored as an entry before being traced: in the shadow queue for an any-hit launch, or -- small-scene path,
     * bounces >= 1 -- in the per-wave ring of the kernel that generated them (origin in LDS, the 16-B contribution in the wave's slice
     * of the shadow queue's memory; bench.py prices either kind at 32 B: 16 + 16 written for a queue entry, 16 written + 16 read back
     * for a ring entry).  rays_shadow counts every shadow ray traced; on the small-scene path the generating kernel answers a shadow
     * ray itself when it can (reference model: a probe against the most likely occluder; EXT model: the whole test), and only the
     * rest become entries. */
    uint64_t shadow_entries;
    uint64_t shadow_entries_bounce0;
    /* Waves whose queue append ran past the capacity of their class's sub-queue: always 0 in a correct run (a path keeps the class
     * it got at bounce 0, so a sub-queue cannot receive more entries than the class has paths).  The entries beyond the capacity are
     * NOT stored -- nothing is written out of bounds -- and their paths are lost; guard_last then holds the two counter values the
     * offending wave saw (extension << 32 | shadow).  cap_debug_set(CAP_DEBUG_QUEUE_CAPACITY_DIV) provokes it for the tests. */
    uint64_t guard_append;
    /* cap_render calls that wanted two batch lanes (tree path, see cap_render) and ran on one because the second working set could not
     * be allocated: same image, ~7 % less throughput.  A (paths, bounces) size that has failed is not tried again until
     * cap_scene_upload / cap_set_resolution / cap_set_shard / cap_set_batch_paths change what is needed, the device reports enough free
     * memory for it (memory can come back without a call on this context), or every 32nd call. */
    uint64_t lane1_dropped;
} CapStats;

typedef struct CapBvhInfo
{
    uint32_t triangle_count;
    uint32_t node_count;  /* internal nodes (triangle_count - 1, or 0) */
    uint32_t max_depth;
    uint32_t stack_entries; /* per-lane LDS traversal stack the trace kernels were specialised for */
    float    bounds_lo[3];
    float    bounds_hi[3];
    double   build_ms;
} CapBvhInfo;

const char* cap_last_error(void);
/* number of HIP devices visible (0 without a GPU); never fails */
int cap_device_count(void);

/* Replaces Dx12 device/queue creation (dx12/dx12.cpp:165-235) + RaytracingSystem ctor (raytracing_system.cpp:182).
 * hip_stream: an existing hipStream_t to run on (e.g. the caller's torch stream), or NULL to create one. */
int  cap_ctx_create(int device_id, void* hip_stream, CapContext** out_ctx);
void cap_ctx_destroy(CapContext* ctx);

/* GeometryStorage upload, CreateGeometryStorage (asset_load_system.cpp:162-255): pooled positions/normals
 * (3 floats per vertex), texcoords (2 per vertex), mesh-local uint32 indices, 32-byte mesh descriptors. */
int cap_scene_upload(CapContext* ctx, const float* positions, const float* normals, const float* texcoords,
                     const uint32_t* indices, const CapMeshDesc* meshes, uint32_t vertex_count, uint32_t index_count,
                     uint32_t mesh_count);
/* TextureSystem::LoadTexture upload half (texture_system.cpp:58-118): RGBA8, row 0 first. rgba8 == NULL
 * installs the reference's "missing texture" 1x1 zero texel (texture_system.cpp:47-56). */
int cap_texture_upload(CapContext* ctx, uint32_t index, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* Blue-noise texture load (raytracing_system.cpp:642-646): 256x256 RGBA8; only R,G are read (sampling.h:13-23). */
int cap_bluenoise_upload(CapContext* ctx, const uint8_t* rgba8_256x256);
/* EXT */
int cap_materials_upload(CapContext* ctx, const CapMaterial* materials, uint32_t mesh_count);

/* Replaces BLASSystem::BuildBLAS + TLASSystem::BuildTLAS (blas_system.cpp:14-67, tlas_system.cpp:11-73):
 * explicit on-device LBVH over all meshes; (instance, primitive) ids are kept per triangle. */
int cap_bvh_build(CapContext* ctx);
/* How cap_bvh_build builds the tree (the hits are the same either way; every build ends with the collapse into the compressed
 * 8-wide view).  LBVH: Morton hierarchy on the device, ~4 ms for 262 k triangles.  PLOC: agglomerative clustering on the device
 * with a surface-area distance (ploc.hip), ~3 ms, shadow and camera rays as fast as with the SAH tree -- the build for scenes
 * that change.  SAH: binned surface-area heuristic on the host, ~0.15 s for 262 k triangles, fastest traversal -- the counterpart of
 * D3D12_RAYTRACING_ACCELERATION_STRUCTURE_BUILD_FLAG_PREFER_FAST_TRACE, which the reference asks for (blas_system.cpp:42-47) while
 * building only once (tlas_system.cpp:111-121).  AUTO: PLOC above 64 triangles (trace times within 1 % of the SAH tree's; smaller
 * scenes are traced exhaustively and get the Morton hierarchy). */
typedef enum CapBvhBuild
{
    CAP_BVH_BUILD_AUTO = 0,
    CAP_BVH_BUILD_LBVH = 1,
    CAP_BVH_BUILD_SAH  = 2,
    CAP_BVH_BUILD_PLOC = 3, /* on the device: agglomerative clustering over the Morton order with a surface-area distance */
    CAP_BVH_BUILD_SAH_DEVICE = 4 /* on the device: binned surface-area splits from the root down to small segments, the clustering
                                  * inside those -- the tree quality the reference requests (PREFER_FAST_TRACE, blas_system.cpp:44) */
} CapBvhBuild;
int cap_set_bvh_build(CapContext* ctx, uint32_t mode);
int cap_bvh_info(CapContext* ctx, CapBvhInfo* out);
/* Debug/test readback: nodes = node_count * 16 floats (see DESIGN.md "BVH node"), leaf_triangles = triangle ids in leaf order. */
int cap_bvh_readback(CapContext* ctx, float* nodes, uint32_t* leaf_triangles);
/* The compressed 8-wide view the extension- and shadow-ray kernels walk (capsaicin_amd/csrc/cap_wide.h): nodes = 20 uint32 per
 * node (info[0] nodes; call with nodes = NULL first), tri_src = leaf position per wide-order triangle record (triangle_count
 * entries), info = {node count, depth, leading top-level nodes}.  Built by cap_bvh_build: on the device when the device built
 * the binary tree (CAP_BVH_BUILD_LBVH), on the host from the host's SAH tree.  For tests and tools. */
int cap_bvh_wide_readback(CapContext* ctx, uint32_t* nodes, uint32_t* tri_src, uint32_t* info);

/* ---- animated geometry: vertex updates and in-place refit (DXR ALLOW_UPDATE / PERFORM_UPDATE) ----
 * cap_scene_update_vertices replaces vertex attributes of the uploaded scene; topology (indices, mesh table, triangle count) is
 * unchanged.  positions / normals: 3 * vertex_count floats, texcoords: 2 * vertex_count floats (vertex_count of cap_scene_upload);
 * a NULL array keeps the current one.  Host arrays are copied before the call returns.  With CAP_VERTICES_DEVICE the three
 * pointers are 4-byte aligned device pointers on the context's GPU, copied on the context stream after everything enqueued
 * (a render's second batch lane included); the source must be ready when the call is made and may be reused once cap_bvh_refit
 * or cap_sync has returned.  Positions must be finite.  The update marks the trees stale: cap_render, cap_trace_rays,
 * cap_trace_occlusion, cap_bvh_readback and cap_bvh_wide_readback return CAP_ERR_STATE until cap_bvh_refit or cap_bvh_build.
 * Errors: CAP_ERR_STATE (no scene), CAP_ERR_INVALID_ARG (unknown flags, a device pointer misaligned or not on the context's GPU).
 *
 * cap_bvh_refit refits the trees of the last cap_bvh_build to the current vertices: same topology (binary tree, 8-wide view,
 * leaf orders), new boxes, and everything else the build derives from the vertices.  Hits and images are bit-identical to a
 * fresh build of the moved scene; the boxes may be looser (CapRefitInfo).  With unchanged positions it reproduces the build's
 * trees byte for byte.  A later cap_set_bvh_build does not affect it.  Waits for the device, like cap_bvh_build.
 * Errors: CAP_ERR_STATE (no tree built since the last cap_scene_upload).  out may be NULL. */
enum
{
    CAP_VERTICES_DEVICE = 1u << 0 /* the three pointers are device pointers on the context's GPU */
};
int cap_scene_update_vertices(CapContext* ctx, const float* positions, const float* normals, const float* texcoords, uint32_t flags);
typedef struct CapRefitInfo
{
    double ms;                         /* host wall time of the call (as CapBvhInfo::build_ms) */
    double expected_node_visits;       /* binary tree after the refit: 1 + sum(inner child box area) / root box area */
    double expected_node_visits_built; /* the same for the boxes the last cap_bvh_build produced */
} CapRefitInfo;
int cap_bvh_refit(CapContext* ctx, CapRefitInfo* out);

/* CameraSystem::Run upload (camera_system.cpp:89-131). sensor_size is used as given (the caller applies
 * AdjustCameraAspectBasedOnWindow, camera_system.cpp:10-17). */
int cap_camera_set(CapContext* ctx, const CapCameraData* camera);
/* CameraComponent::prev_camera_buffer (camera_system.cpp:89-131; bound as g_prev_camera, raytracing_system.cpp:1227-1228) */
int cap_prev_camera_set(CapContext* ctx, const CapCameraData* camera);
/* RenderSystem::window_width/height (render_system.h) */
int cap_set_resolution(CapContext* ctx, uint32_t width, uint32_t height);
/* Screen-tile sharding: this context renders the 8x8 tiles t with t % shard_count == shard_index. */
int cap_set_shard(CapContext* ctx, uint32_t shard_index, uint32_t shard_count);
/* Upper bound of (frame, pixel) paths kept in flight per batch.  0 = default: 128 Mi paths (~28 GB of queues and planes per working
 * set; the tree path keeps two) when a call has more than 64 Mi to render and the device reports room for three such working sets,
 * 64 Mi otherwise; at most 64 frames per batch either way.  Results do not depend on it. */
int cap_set_batch_paths(CapContext* ctx, uint64_t max_paths);
/* Test hooks (no reference counterpart; never needed by a host program).  CAP_DEBUG_QUEUE_CAPACITY_DIV: the sub-queues of the next
 * renders get 1 / value of the capacity they need (value 1 = normal), so that the kernels' append guard (CapStats::guard_append) can
 * be seen to fire -- entries beyond a sub-queue are dropped and counted, never written. */
enum
{
    CAP_DEBUG_QUEUE_CAPACITY_DIV = 1,
    /* The extension- and shadow-ray kernels walk the compressed 8-wide view of the tree while its depth fits their per-lane stacks
     * (LDS part + spill slice: 21 levels) and fall back to the binary tree's kernels beyond.  WIDE_DEPTH_LIMIT (0 = none) lowers that
     * bound so that the fallback can be exercised on ordinary scenes; WIDE_IN_USE (read-only) says which kernels the next render
     * takes. */
    CAP_DEBUG_WIDE_DEPTH_LIMIT   = 2,
    CAP_DEBUG_WIDE_IN_USE        = 3,
    /* FAIL_LANE1 (0 / 1): the allocation of cap_render's second batch lane fails (what running out of HBM does), so that the one-lane
     * fallback and CapStats::lane1_dropped can be tested; LANES_USED (read-only): the lanes the last cap_render ran on (1 or 2). */
    CAP_DEBUG_FAIL_LANE1         = 4,
    CAP_DEBUG_LANES_USED         = 5,
    /* Canary behind the last queue class (the append guard's direct proof).  CANARY_FILL (set, after a first cap_render has allocated
     * them): every entry of the context's extension-queue planes takes one marker word.  CANARY_BEHIND (get): entries BEHIND the 64
     * sub-queues of the last render (index >= 64 x its sub-queue capacity) that no longer hold the marker -- 0 unless something wrote
     * past the last class; CANARY_USED (get): the same count inside the sub-queues (> 0 after any render: the check can see writes). */
    CAP_DEBUG_QUEUE_CANARY_FILL   = 6,
    CAP_DEBUG_QUEUE_CANARY_BEHIND = 7,
    CAP_DEBUG_QUEUE_CANARY_USED   = 8,
    /* SELFTEST_DIV (get, ~0.5 s): the reconstruction chain's exact mode evaluates its per-tap divisions without the scaling steps of
     * the compiler's IEEE expansion where the operands are in a range that never triggers them (post.hip div_unscaled); this runs both
     * forms on the device -- every normal float through log2, 2^30 operand pairs over the whole range -- and returns the number of
     * results that differ in any bit: 0. */
    CAP_DEBUG_SELFTEST_DIV        = 9,
    /* NEE_PAIRS (get): fan pairs the EXT model's next-event rays test on the small-scene path << 32 | fan pairs of the scene.  Pairs that
     * support the scene's convex hull with every light at a safe distance inside cannot occlude a segment between a scene point and a
     * light point under the intersection contract (rule and error bound: ctx_scene.hip update_nee_pairs) and are left out. */
    CAP_DEBUG_NEE_PAIRS           = 10,
    /* The fused small-scene kernels evaluate the square roots and divisions of a vertex's shading without the scaling steps of the
     * compiler's IEEE expansions where the operands cannot trigger them (csrc/cap_unscaled.h).  SELFTEST_SHADE_UNARY (get, ~1 s): every
     * such unary form against the plain one over every float of its range; SELFTEST_SHADE_DIV2 (get): the pair of quotients of the
     * tangent frame over more than 2^30 operand pairs inside its guard.  Both return the number of results that differ in any bit: 0.
     * SHADE_TAME (get, after cap_bvh_build / cap_bvh_refit): 1 if every triangle's stored vertex normals have squared lengths in
     * [0.5, 2] and pairwise dot products >= 0.25 -- what those kernels need to take the unscaled forms; 0: they take the plain ones. */
    CAP_DEBUG_SELFTEST_SHADE_UNARY = 11,
    CAP_DEBUG_SELFTEST_SHADE_DIV2  = 12,
    CAP_DEBUG_SHADE_TAME           = 13,
    /* CAMERA_CULL (get): 1 if the last cap_render let the camera-ray tiles of the small-scene path skip the fan pairs whose screen
     * bounds miss them, 0 if every tile tested every pair: the switch CAP_NO_CAMERA_CULL, or a camera basis whose deviation from an
     * orthonormal one could move a projected vertex by more than an eighth of the bounds' two-pixel pad (context.hip cap_render). */
    CAP_DEBUG_CAMERA_CULL          = 14,
    /* MARK_FORM (get, after cap_bvh_build): form << 8 | dense.  dense: 1 if the scene's small-scene records are fan pairs only with pair j
     * holding triangles 2j and 2j + 1 (cap_debug_pair_ids_dense), so that a triangle's id is its position in the list.  form: how the
     * last cap_render's fused small-scene launches of bounce >= 1 built the closest-hit candidate mask -- 0: no such launch, or a kernel
     * without the two-phase loop; 1: by triangle id (one bit word per triangle); 2: by position, one carry-chain step per triangle (dense
     * scenes); 3: the same over two words (33-64 triangles). */
    CAP_DEBUG_MARK_FORM            = 15,
    /* SAMPLE_TABLE (get): 1 if the fused small-scene launches of the last cap_render took a vertex's direction-sample terms (sin / cos of
     * the azimuth times sin theta, cos theta: functions of the blue-noise sample alone) from a table built once per batch -- 4 096 entries
     * per frame slot and sampling bounce -- instead of computing them per vertex; 0 if they computed them (the switch CAP_SAMPLE_TABLE = 0,
     * the EXT model, feedback, the tree path, untame records, num_bounces 0).  Same bits either way.
     * SELFTEST_SAMPLE_TABLE (get, after such a render): every entry of the last batch's table against the per-vertex evaluation, on the
     * device: entries that differ in any bit << 32 | (bounce, frame slot) rows compared, 4 096 entries each. */
    CAP_DEBUG_SAMPLE_TABLE          = 16,
    CAP_DEBUG_SELFTEST_SAMPLE_TABLE = 17,
    /* CAMERA_TABLE (get): 1 if the last batch of the last cap_render ran bounce 0 inside bounce 1's launch -- the camera rays traced once
     * per group of frame slots that share a sub-pixel jitter into a table of camera vertices, the per-slot shading of those vertices at the
     * head of the first bounce >= 1 launch, the shadow rays through the wave rings -- and 0 if bounce 0 was a launch of its own (the switch
     * CAP_NO_CAMERA_TABLE, CAP_RENDER_AOV, num_bounces 0, every render without the sample table or without the code in the colour plane).
     * Same bits and the same CapStats either way: launches_trace_any still counts bounce 0's shadow rays as one any-hit pass per batch.
     * SELFTEST_CAMERA_TABLE (get, right after such a render): bounce 0's camera vertex of every (frame slot, padded pixel) of the last
     * batch, evaluated with the slot's own frame constants, against the table entry of the slot's group, on the device: entries that
     * differ in any bit << 32 | groups << 16 | frame slots compared. */
    CAP_DEBUG_CAMERA_TABLE          = 18,
    CAP_DEBUG_SELFTEST_CAMERA_TABLE = 19,
    /* GRAY_ENTRIES (get): 1 if the fused small-scene launches of the last cap_render used 32-byte extension-queue entries -- (origin,
     * throughput) (direction, path id), the throughput being one float -- and 0 if they used the 48-byte entries with three throughput
     * words (the switch CAP_NO_GRAY_ENTRIES, a scene with textures, every render without the sample table).  Same bits and the same
     * CapStats either way: without textures the three components of a throughput are the same operations on the same operands.
     * SELFTEST_GRAY (get, right after a render in the 48-byte form on the small-scene path): that premise on the device -- every entry the
     * last batch left in its two extension queues, up to the class counts: entries whose three throughput words are not bitwise equal
     * << 32 | entries looked at (saturating at 2^32 - 1). */
    CAP_DEBUG_GRAY_ENTRIES          = 20,
    CAP_DEBUG_SELFTEST_GRAY         = 21,
    /* GROUP_WALK (get): how the head kernel of the last batch of the last cap_render (CAMERA_TABLE = 1) walked bounce 0's chunks.  m >= 1:
     * every group of frame slots sharing a sub-pixel jitter had m slots, and the m slots of a group visited each 64-pixel group back to
     * back, group after group, so that a camera-table entry is fetched once for its m readers (cap_debug_head_chunk below is the
     * mapping).  0: slot-major, every slot sweeping the image on its own -- groups of unequal sizes, the switch CAP_NO_GROUP_WALK, or no
     * head kernel.  Same bits and the same CapStats either way.
     * CAMERA_TABLE_REUSED (get): 1 if the last batch of the last cap_render found the camera-vertex table of its working set already built
     * from the same inputs -- camera, resolution and shard, the groups' jitters, the scene's records -- and launched no builder; 0 if it
     * built the table (any of those changed, the switch CAP_NO_TABLE_REUSE, a failed call in between, or no table).  SELFTEST_CAMERA_TABLE
     * checks a reused table like a built one. */
    CAP_DEBUG_GROUP_WALK            = 22,
    CAP_DEBUG_CAMERA_TABLE_REUSED   = 23,
    /* SKY_PLANE (get): 1 if the fused small-scene launches of the last cap_render wrote the sky term of a path that escapes at bounce >= 1
     * as one store of its throughput into a plane of one float per (frame slot, padded pixel), which the resolve adds to the path's
     * colour -- and 0 if they added it to the colour plane with three float atomics (the switch CAP_NO_SKY_PLANE, and every render
     * without GRAY_ENTRIES, without CAMERA_TABLE or with CAP_RENDER_AOV).  Same bits and the same CapStats either way: the resolve's
     * additions are the atomics', on the same operands in the same order.
     * SKY_PLANE_NONZERO (get, right after such a render): the entries of the last batch's plane that are not +0, counted on the device:
     * the paths of that batch that escaped at bounce >= 1 with a throughput other than +0. */
    CAP_DEBUG_SKY_PLANE             = 24,
    CAP_DEBUG_SKY_PLANE_NONZERO     = 25,
    /* A/B and diagnostic switches of the build and render paths (which kernels trace the camera and the shadow rays, one or two batch
     * lanes, the builders' parameters ...): ONE table per context, key = SWITCH_BASE + cap_debug_switch_index("CAP_..."), the names being
     * the environment variables that fill the table once, at cap_ctx_create (tools set those around a whole process; nothing else in the
     * library reads the environment except CAP_RCCL_LIBRARY).  value: the switch's number (flags: 1 / 0), ~0 = the product's own
     * choice again.  A switch is read by the next cap_bvh_build / cap_render.  Every switch selects between paths that give the same
     * image: they exist for measurements and for tests that exercise a path the product would not take on a small scene. */
    CAP_DEBUG_SWITCH_BASE         = 64
};
int cap_debug_set(CapContext* ctx, uint32_t key, uint64_t value);
int cap_debug_get(CapContext* ctx, uint32_t key, uint64_t* value);
/* Index of a switch by its name ("CAP_NO_WIDE8", "CAP_PRIMARY_WIDE", ...; capsaicin_amd/csrc/cap_kernels.h CapSwitch), -1 if unknown. */
int cap_debug_switch_index(const char* name);
/* The rule behind CAP_DEBUG_MARK_FORM's dense bit, on a host copy of the small-scene record lists: pair_count fan pair records of 20 floats
 * (float 18 = the first triangle's id as bits), single_count unpaired triangles, tri_count triangles in all.  1 if tri_count > 0, there is
 * no unpaired triangle, tri_count == 2 * pair_count and pair j's id is 2j for every j; else 0.  Needs no device. */
int cap_debug_pair_ids_dense(const float* pair_records, uint32_t pair_count, uint32_t single_count, uint32_t tri_count);
/* The head kernels' group walk (CAP_DEBUG_GROUP_WALK) on the host, by the function the kernels run: for a batch of n_slots = groups x m
 * frame slots of cps 64-pixel groups each and `order` = its slots sorted by jitter group (n_slots bytes, a permutation), the frame slot
 * and the 64-pixel group that each chunk index c[k] < cps * n_slots stands for.  m = 1 with the identity order is the slot-major walk.
 * CAP_ERR_INVALID_ARG for a NULL array, m = 0, n_slots > 64 or not a multiple of m, cps * n_slots > 2^26.  Needs no device. */
int cap_debug_head_chunk(uint32_t cps, uint32_t m, const uint8_t* order, uint32_t n_slots, const uint32_t* c, uint64_t count, uint32_t* slot,
                         uint32_t* group64);
/* The address checks every cap_trace_* entry point makes on its device arrays, on `count` <= 4 made-up ranges: array i holds n x stride[i]
 * bytes from base[i], and base[i] must be a multiple of align[i] (a power of two); stride[i] == 0: the caller left array i out.  CAP_OK if
 * every array is aligned, ends inside the address space and shares no byte with another one; else CAP_ERR_INVALID_ARG with the entry
 * points' message in cap_last_error().  Needs no device. */
int cap_debug_query_ranges(uint64_t n, uint32_t count, const uint64_t* base, const uint64_t* stride, const uint32_t* align);
/* The pruning arithmetic of cap_closest_instances (below) for ONE instance transform (12 floats, row-major 3x4), one object-space box
 * (box_lo, box_hi: 3 floats each), one world point (3 floats) and one best squared distance, by the very functions the instance setup
 * and the query kernel run.  Outputs, each may be NULL: world_to_object = the 12 floats of W as the table would store them; g = the
 * proven lower bound on the smallest singular value of the transform's 3x3 part; xw = the world extent Xw of the box under the
 * transform (no |coordinate| the world-record arithmetic meets exceeds it); slack = the absolute part of the bound for this point,
 * 96 * 2^-24 * (|point|_inf + xw); skip = 1 if the walk would skip the box while the best dist2 is best_dist2, else 0.  An inert
 * transform (the rule of cap_instances_set) gives W = 0, g = 0, xw = 0 and skip = 0.  CAP_ERR_INVALID_ARG for a NULL input.  Needs no
 * device. */
int cap_debug_closest_instance_bound(const float* transform, const float* box_lo, const float* box_hi, const float* point, float best_dist2,
                                     float* world_to_object, float* g, float* xw, float* slack, uint32_t* skip);
/* The pruning arithmetic of cap_overlap_instances (below) for ONE instance transform (12 floats, row-major 3x4), the object-space box
 * of its object (object_lo, object_hi), one WORLD-space box (world_lo, world_hi: the instance's stored world box, a top-level node's, or
 * a triangle's world vertex box standing for them), one OBJECT-space box (node_lo, node_hi: a node of the object's tree, or a triangle's
 * vertex box standing for the nodes above it) and one world-space query box (box_lo, box_hi), by the very functions the instance setup
 * and the query kernel run; 3 floats each.  Outputs, each may be NULL: world_to_object, g, xw as cap_debug_closest_instance_bound's;
 * slack = 96 * 2^-24 * (|box|_inf + xw), what the query box is grown by at the top level (there with the table's largest xw) and,
 * divided by g, what its image is grown by inside the instance; image_lo, image_hi = that image, 3 floats each; skip_top = 1 if the
 * walk would skip the world box, skip_node = 1 if it would skip the object-space box, else 0.  An inert transform gives W = 0, g = 0,
 * xw = 0, a zero image and no skip.  CAP_ERR_INVALID_ARG for a NULL input.  Needs no device. */
int cap_debug_overlap_instance_prune(const float* transform, const float* object_lo, const float* object_hi, const float* world_lo, const float* world_hi,
                                     const float* node_lo, const float* node_hi, const float* box_lo, const float* box_hi, float* world_to_object, float* g,
                                     float* xw, float* slack, float* image_lo, float* image_hi, uint32_t* skip_top, uint32_t* skip_node);
/* The bottom-level prune of cap_overlap_triangles_instances (below) for ONE instance transform (12 floats, row-major 3x4), the
 * object-space box of its object (object_lo, object_hi), one OBJECT-space node box (node_lo, node_hi: a node of the object's tree, or a
 * triangle's vertex box standing for the nodes above it) and one WORLD-space query box (query_lo, query_hi: the min and max of a query
 * triangle's vertices), by the very functions the query kernel runs; 3 floats each.  Outputs, each may be NULL: xw as
 * cap_debug_closest_instance_bound's; slack = 96 * 2^-24 * (|query box|_inf + xw), what the query box is grown by inside the instance;
 * world_lo, world_hi = the world box of the node under the transform as the walk computes it, 3 floats each; skip_node = 1 if the walk
 * would skip the node, else 0.  An inert transform gives zeros and no skip.  CAP_ERR_INVALID_ARG for a NULL input.  Needs no device. */
int cap_debug_overlap_world_node(const float* transform, const float* object_lo, const float* object_hi, const float* node_lo, const float* node_hi,
                                 const float* query_lo, const float* query_hi, float* xw, float* slack, float* world_lo, float* world_hi,
                                 uint32_t* skip_node);
/* The bottom-level prune of cap_sweep_instances (below) for ONE instance transform (12 floats, row-major 3x4), the object-space box of
 * its object (object_lo, object_hi), one OBJECT-space node box (node_lo, node_hi: a node of the object's tree, or a triangle's vertex box
 * standing for the nodes above it), one WORLD-space sweep (8 floats, a CapSweepDesc: origin, radius, direction, tmax; the tmax word is
 * not read) and the far bound of the test (the walk's best time so far, or tmax), by the very functions the query kernel runs.  Outputs,
 * each may be NULL: xw as cap_debug_closest_instance_bound's; radius = R = fl(r + 128 * 2^-24 * (|origin|_inf + xw + r)), what the
 * node's world box is grown by; world_lo, world_hi = the world box of the node under the transform as the walk computes it, 3 floats
 * each; entry = the time the ray enters the grown box (0 inside), exit_padded = what it is compared with, fl(fl(min(exit, far) *
 * (1 + 8 * 2^-24)) + 2^-126); skip_node = 1 if the walk would skip the node (entry > exit_padded), else 0.  An inert transform gives
 * zeros and no skip.  CAP_ERR_INVALID_ARG for a NULL input.  Needs no device. */
int cap_debug_sweep_instance_prune(const float* transform, const float* object_lo, const float* object_hi, const float* node_lo, const float* node_hi,
                                   const float* sweep, float far_bound, float* xw, float* radius, float* world_lo, float* world_hi, float* entry,
                                   float* exit_padded, uint32_t* skip_node);
/* Traversal strategy of the trace kernels (same hits either way): AUTO picks EXHAUSTIVE for scenes of at most 64
 * triangles (wave-uniform test of every triangle, no stack) and STACK (LBVH + per-lane LDS stack) otherwise. */
typedef enum CapTraversal
{
    CAP_TRAVERSAL_AUTO       = 0,
    CAP_TRAVERSAL_STACK      = 1,
    CAP_TRAVERSAL_EXHAUSTIVE = 2 /* refused above 4096 triangles */
} CapTraversal;
int cap_set_traversal(CapContext* ctx, uint32_t mode);

/* RaytracingSystem::Run ray passes (raytracing_system.cpp:266-292) for frame_count = frame_begin ..
 * frame_begin + n_frames - 1, each frame's COMBINED added to the accumulation buffer in frame order.
 * num_bounces == SettingsComponent::num_diffuse_bounces (gui_system.h:39).  Asynchronous on the context
 * stream; cap_readback / cap_stats_get / cap_sync wait for it. */
int cap_render(CapContext* ctx, uint32_t frame_begin, uint32_t n_frames, uint32_t num_bounces, uint32_t flags);
int cap_accum_reset(CapContext* ctx);
/* Resume of a long accumulation (SURVEY.md 5 "checkpoint": dump accumulation + sample index): sum_rgba = width*height*4 floats as
 * cap_readback(CAP_BUF_ACCUM_SUM) returned them (running sums in .xyz, frames in .w), frames = how many frames they hold; the next
 * cap_render(frames, n, ..) continues the sum exactly where the dumped one stopped -- the additions are the same, in the same frame
 * order, so the result is bit-identical to an uninterrupted render.  A sharded context takes its own tiles of the image. */
int cap_accum_import(CapContext* ctx, const float* sum_rgba, uint64_t frames);
int cap_sync(CapContext* ctx);

/* dst: width*height*4 floats (host), row 0 = pixel row 0.  Pixels outside this context's shard read 0. */
int cap_readback(CapContext* ctx, CapBufferKind kind, float* dst);

int cap_stats_get(CapContext* ctx, CapStats* out);
int cap_stats_reset(CapContext* ctx);

/* ---- ray queries: TraceRay for rays the caller makes (AO, visibility probes, light baking, picking) ----
 * The traversal the render uses (the compressed 8-wide tree, or the binary tree where that is not used, CAP_NO_WIDE8) on the caller's
 * rays.  Hit rule = DESIGN.md "Intersection contract", the DXR triangle rule with identity transforms: two-sided, closest hit
 * accepted for tmin < t < tmax, minimum t wins, equal t goes to the lower triangle id; (u, v) are the barycentrics that weight v1
 * and v2 (DXR's BuiltInTriangleIntersectionAttributes).  Occlusion is the division-free form tmin * det < T < tmax * det
 * (RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH).  Records are bit-identical to the oracle's brute force over every triangle, whichever
 * builder (cap_set_bvh_build) and tree made them.
 *
 * triangle = the global triangle id, in mesh-table order then primitive order: triangle p of mesh m (the m-th CapMeshDesc of
 * cap_scene_upload) has id sum_{k < m} index_count_k / 3 + p -- not first_index_offset / 3.  The reference's InstanceID() /
 * PrimitiveIndex() (one instance per mesh, tlas_system.cpp:52-55) are (m, p), the pair CAP_BUF_GBUFFER_GEO stores: the caller
 * maps an id back with the prefix sums of the mesh table's triangle counts.
 *
 * Degenerate rays -- a NaN or infinite component of origin or direction, a zero direction, tmax <= tmin or a NaN in either --
 * are not traversed and report a miss (occlusion 0).  tmax = +inf is a ray like any other: every hit beyond tmin counts.
 *
 * Both calls take device pointers on the context's GPU, 16-byte aligned, with ray and output ranges that do not overlap, and are
 * asynchronous on the context stream (like cap_resolve_tiles): ordered after everything enqueued on the context (a cap_render's
 * second batch lane included) and before what follows; cap_sync waits for them.  They use the context's traversal spill area
 * and nothing of the render's state: accumulation, CapStats, queues, post histories and feedback stay as they were.  flags is
 * reserved (0).  n may exceed 2^32: the library splits it into launches.  Errors: CAP_ERR_INVALID_ARG (flags, NULL,
 * misalignment, overlap), CAP_ERR_STATE (before cap_bvh_build).  n = 0 does nothing. */
typedef struct CapRayDesc /* DXR RayDesc layout: 32 B */
{
    float origin[3];
    float tmin;
    float direction[3];
    float tmax;
} CapRayDesc;
typedef struct CapHit /* 16 B; a miss is (tmax, 0, 0, 0xFFFFFFFF) */
{
    float    t;
    float    u;
    float    v;
    uint32_t triangle;
} CapHit;
/* closest hit of each ray: device_hits[i] for device_rays[i] */
int cap_trace_rays(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, CapHit* device_hits, uint32_t flags);
/* 1 if some triangle satisfies the occlusion rule, else 0; one uint32 per ray */
int cap_trace_occlusion(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, uint32_t* device_occluded, uint32_t flags);

/* ---- multi-hit ray queries: the first k hits of each ray (LiDAR returns, thickness, depth complexity; DXR / OptiX any-hit loops) ----
 * A ray's hits are every triangle the closest-hit rule above accepts (tmin < t < tmax, two-sided), sorted by (t, triangle)
 * ascending: equal t goes to the lower id, the order cap_trace_rays' tie rule uses.  device_hits[i * k + j], j < k, is ray i's j-th
 * hit as a CapHit (t, u, v, triangle); slots after its last hit hold the miss record (tmax, 0, 0, 0xFFFFFFFF).  A triangle appears at
 * most once per ray.  With k = 1 every record is exactly what cap_trace_rays returns.  Records are bit-identical to the oracle's
 * brute force, whichever builder and tree made them.
 *
 * device_counts: NULL, or n uint32: the number of ALL hits of ray i, not capped at k (with CAP_MULTI_CONTINUE: of the hits after
 * the cursor).  Counts follow the contract: a ray through an edge or vertex shared by several triangles counts each of them.
 * Asking for counts turns off pruning by the k-th hit, so it costs a full traversal of the interval.  k = 0 counts only:
 * device_hits must be NULL and device_counts given.
 *
 * Paging (CAP_MULTI_CONTINUE): on entry, slot k - 1 of each ray's page is read as a cursor (t_c, g_c); only hits with
 * (t, triangle) > (t_c, g_c) in lexicographic order count, and the next page is written over the old one.  A page that was not
 * full ends in a miss record, whose cursor (tmax, 0xFFFFFFFF) admits nothing: that ray's next page is empty.  Calling again with
 * the same rays and buffer walks every hit exactly once, equal-t hits on either side of a page boundary included.  The cursor
 * slot must hold what the previous call wrote there.
 *
 * Everything else is as for cap_trace_rays: degenerate rays give miss pages and count 0 (with CAP_MULTI_CONTINUE too); device
 * pointers on the context's GPU, asynchronous on the context stream and ordered behind a render's second lane; nothing of the
 * render's state is used; n may exceed 2^32.  Errors: CAP_ERR_STATE before cap_bvh_build and while the trees are stale after
 * cap_scene_update_vertices; CAP_ERR_INVALID_ARG for k > CAP_MULTI_MAX_K, k = 0 with hits given or counts NULL,
 * CAP_MULTI_CONTINUE with k = 0, unknown flags, NULL rays (or hits with k > 0), rays or hits not 16-byte or counts not 4-byte
 * aligned, any overlap between the ray, hit and count ranges, and n * k records beyond the address space.  Nothing is written on
 * an error; n = 0 does nothing. */
#define CAP_MULTI_MAX_K 16
enum
{
    CAP_MULTI_CONTINUE = 1u << 0 /* read slot k - 1 of each page as the cursor and write the next page over it */
};
int cap_trace_rays_multi(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, uint32_t k, CapHit* device_hits, uint32_t* device_counts,
                         uint32_t flags);

/* ---- ray flags and instance masks: DXR TraceRay's RayFlags and InstanceInclusionMask for the three queries above ----
 * The _ex calls are the plain calls with a per-call filter (one CapTraceOptions for all n rays).  A ray's hits under the options are
 * the hits of the plain rule whose triangle passes both filters below; nothing else changes: cap_trace_rays_ex returns the minimum
 * of that set in (t, triangle) order, cap_trace_occlusion_ex whether the occlusion form accepts some triangle that passes,
 * cap_trace_rays_multi_ex the first k of the set, counts of the set and pages over the set (cursor as above).  Records stay
 * bit-identical to the oracle's brute force over the triangles that pass.
 *
 * Facing.  With the contract's det = -d.n, n = e1 x e2 (before the two-sided sign flip), a triangle is front-facing for a ray when
 * det > 0: the ray travels against n and sees v0, v1, v2 counter-clockwise (right-handed).  CAP_RAY_FLAG_CULL_BACK_FACING drops
 * the triangles with det < 0, CAP_RAY_FLAG_CULL_FRONT_FACING those with det > 0; det == 0 is no hit either way.  Both together:
 * CAP_ERR_INVALID_ARG, as in DXR.
 *
 * Masks.  One byte per mesh (the reference has one instance per mesh), 0xFF until cap_scene_set_instance_masks says otherwise.  A
 * triangle of mesh m is a candidate iff masks[m] & instance_mask & 0xFF != 0.  instance_mask = 0 in the options means 0xFF, so a
 * zero-filled struct is the plain call (the one deviation from DXR, the rule CapPostSettings follows).  A mesh whose mask is 0 is
 * invisible to every query, the plain calls included, while the table is installed, as in DXR.  cap_render ignores the masks.
 *
 * CAP_RAY_FLAG_ACCEPT_FIRST_HIT on cap_trace_rays_ex: the record is SOME member of the filtered hit set with its own exact
 * (t, u, v, triangle), and the miss record exactly when the set is empty (the divided test, so hit / miss equals the closest
 * query's, not the occlusion query's).  Which member is unspecified and may differ between runs and trees.  On
 * cap_trace_occlusion_ex the flag is accepted and changes nothing; on cap_trace_rays_multi_ex it is CAP_ERR_INVALID_ARG.
 *
 * options == NULL or all-zero: the call IS the plain call (same validation, same kernels, same bits); so is any call without a
 * cull or first-hit flag while no mask table is installed.  Errors on top of the plain calls': CAP_ERR_INVALID_ARG for unknown flag
 * bits, both cull flags, non-zero reserved words, instance_mask > 0xFF.  Nothing is written on an error. */
enum /* DXR RAY_FLAG_* values */
{
    CAP_RAY_FLAG_ACCEPT_FIRST_HIT  = 0x04, /* RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH */
    CAP_RAY_FLAG_CULL_BACK_FACING  = 0x10, /* RAY_FLAG_CULL_BACK_FACING_TRIANGLES */
    CAP_RAY_FLAG_CULL_FRONT_FACING = 0x20  /* RAY_FLAG_CULL_FRONT_FACING_TRIANGLES */
};
typedef struct CapTraceOptions /* 16 B */
{
    uint32_t ray_flags;     /* CAP_RAY_FLAG_* */
    uint32_t instance_mask; /* InstanceInclusionMask, low 8 bits; 0 means 0xFF (no filtering) */
    uint32_t reserved[2];   /* must be 0 */
} CapTraceOptions;
/* masks: mesh_count host bytes, one per mesh of the uploaded scene, copied before the call returns; NULL restores all 0xFF (and
 * removes the table).  Ordered on the context stream after every query already enqueued and before those that follow.  Does not
 * make the trees stale.  cap_scene_upload resets the masks to 0xFF; cap_bvh_build, cap_bvh_refit and cap_scene_update_vertices
 * keep them.  CAP_ERR_STATE before cap_scene_upload, CAP_ERR_INVALID_ARG when mesh_count is not the uploaded scene's. */
int cap_scene_set_instance_masks(CapContext* ctx, const uint8_t* masks, uint32_t mesh_count);
int cap_trace_rays_ex(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, CapHit* device_hits, const CapTraceOptions* options);
int cap_trace_occlusion_ex(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, uint32_t* device_occluded,
                           const CapTraceOptions* options);
/* multi_flags: cap_trace_rays_multi's flags (CAP_MULTI_CONTINUE) */
int cap_trace_rays_multi_ex(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, uint32_t k, CapHit* device_hits,
                            uint32_t* device_counts, uint32_t multi_flags, const CapTraceOptions* options);

/* ---- closest-point queries: the triangle nearest to a point, and how far away it is (Embree's rtcPointQuery) ----
 * For distance fields, proximity and collision tests against the scene (animated ones included: the trees stay current under
 * cap_bvh_refit), ICP registration, snapping and projecting points onto the scene.  Walks the binary tree of the scene.
 *
 * The per-triangle function is defined on the stored intersection record (v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)), not on the original
 * vertices.  Every operation is one rounded binary32 operation in the order written, there is no fused multiply-add anywhere, division
 * is correctly rounded, and dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z -- so a plain float32 brute force is bit-identical to the
 * kernel.  It is the Voronoi-region cascade (Ericson, Real-Time Collision Detection 5.1.5); the first matching case wins:
 *   ap = p - v0, d1 = dot(e1, ap), d2 = dot(e2, ap).          d1 <= 0 && d2 <= 0:                   v0, (u, v) = (0, 0)
 *   bp = ap - e1, d3 = dot(e1, bp), d4 = dot(e2, bp).         d3 >= 0 && d4 <= d3:                  v1, (1, 0)
 *   vc = d1*d4 - d3*d2.                                       vc <= 0 && d1 >= 0 && d3 <= 0:        edge v0v1, (d1 / (d1 - d3), 0)
 *   cp = ap - e2, d5 = dot(e1, cp), d6 = dot(e2, cp).         d6 >= 0 && d5 <= d6:                  v2, (0, 1)
 *   vb = d5*d2 - d1*d6.                                       vb <= 0 && d2 >= 0 && d6 <= 0:        edge v2v0, (0, d2 / (d2 - d6))
 *   va = d3*d6 - d5*d4.                                       va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0:
 *                                                             edge v1v2, w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), (1 - w, w)
 *   otherwise the face: s = (va + vb) + vc, (vb / s, vc / s).
 * Then, component-wise, m = e1*u + e2*v, delta = ap - m, dist2 = dot(delta, delta), point = v0 + m.  delta is taken from ap rather
 * than from p - point, so that the error scales with the local geometry and not with the absolute coordinates.
 *
 * The answer.  A triangle is a candidate iff it passes the mask filter and dist2 <= r2, r2 = fl(radius * radius).  A NaN dist2 (a
 * zero-area triangle can produce one) fails the comparison and is never an answer.  The record is the candidate minimal in
 * (dist2, triangle) lexicographic order, the tie rule of the ray queries: the answer depends on neither the tree, nor the builder,
 * nor the visiting order.  The miss record is (0, 0, 0, r2, 0, 0, 0xFFFFFFFF, 0).  radius = +inf is a query like any other; radius = 0
 * admits only triangles with computed dist2 == 0.  Degenerate queries -- a non-finite coordinate, a radius that is NaN or negative --
 * are not traversed and give the miss record with dist2 = 0.
 *
 * Conventions are cap_trace_rays_ex's: device pointers on the context's GPU, both 16-byte aligned, ranges that do not overlap;
 * asynchronous on the context stream and ordered behind a render's second lane; n above 2^24 split into launches, n = 0 does nothing;
 * nothing of the render's state is touched; nothing is written on an error.  CAP_ERR_STATE before cap_bvh_build and while the trees
 * are stale after cap_scene_update_vertices.  options: instance_mask and the mesh-mask table act exactly as in the ray queries (a mesh
 * with mask 0 is invisible here too); any ray_flags bit is CAP_ERR_INVALID_ARG (facing and first hit mean nothing for a point), as are
 * non-zero reserved words and instance_mask > 0xFF; NULL or all-zero is the plain call.
 * Not covered: per-point masks.  The sign of the distance: cap_signed_distance below.  Instances and objects: cap_closest_instances
 * below, nearest in world space. */
typedef struct CapPointDesc /* 16 B */
{
    float point[3];
    float radius; /* search radius, >= 0; +inf: unbounded */
} CapPointDesc;
typedef struct CapClosest /* 32 B */
{
    float    point[3]; /* the closest point q */
    float    dist2;    /* squared distance */
    float    u, v;     /* q = v0 + u*e1 + v*e2, the weights of v1 and v2 */
    uint32_t triangle; /* global id, as CapHit's; 0xFFFFFFFF = miss */
    uint32_t feature;  /* CAP_FEATURE_*: where on the triangle q lies */
} CapClosest;
enum
{
    CAP_FEATURE_FACE = 0,
    CAP_FEATURE_EDGE_V0V1 = 1,
    CAP_FEATURE_EDGE_V1V2 = 2,
    CAP_FEATURE_EDGE_V2V0 = 3,
    CAP_FEATURE_V0 = 4,
    CAP_FEATURE_V1 = 5,
    CAP_FEATURE_V2 = 6
};
int cap_closest_points(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out,
                       const CapTraceOptions* options /* may be NULL */);

/* ---- k nearest and in-radius closest-point queries: the SET of triangles near a point (contact generation, robust ICP, density) ----
 * A point's candidates are exactly cap_closest_points': the triangles that pass the mask filter with dist2 <= r2,
 * r2 = fl(radius * radius), by the per-triangle function above on the stored record; a NaN dist2 is never a candidate.  They are sorted
 * by (dist2, triangle) ascending: equal dist2 goes to the lower id.  device_out[i * k + j], j < k, is point i's j-th nearest candidate
 * as a full CapClosest; slots after its last candidate hold the miss record (0, 0, 0, r2, 0, 0, 0xFFFFFFFF, 0).  A triangle appears at
 * most once per point.  With k = 1, no counts and no cursor every record is bit for bit what cap_closest_points returns.  Records
 * are bit-identical to a float32 brute force, whichever builder made the tree.
 *
 * device_counts: NULL, or n uint32: the number of ALL candidates of point i, not capped at k (with CAP_MULTI_CONTINUE: of those above
 * the cursor).  Asking for counts turns off pruning by the k-th distance: the walk is then bounded by the radius alone, so with
 * radius = +inf it is a full traversal of the tree.  k = 0 counts only: device_out must be NULL and device_counts given.
 *
 * Paging (CAP_MULTI_CONTINUE): on entry, slot k - 1 of each point's page is read as a cursor (dist2_c, g_c) -- words 3 and 6 of that
 * record; only candidates with (dist2, triangle) > (dist2_c, g_c) in lexicographic order count, and the next page is written over the
 * old one.  A page that was not full ends in a miss record, whose cursor (r2, 0xFFFFFFFF) admits nothing: that point's next page is
 * empty.  Calling again with the same points and buffer walks every candidate exactly once, equal-dist2 candidates on either side of
 * a page boundary and candidates with dist2 == r2 included.  The cursor slot must hold what the previous call wrote there.
 *
 * Degenerate queries (a non-finite coordinate, a NaN or negative radius) are not traversed: k miss records with dist2 = 0 and count 0,
 * with CAP_MULTI_CONTINUE too.  Everything else is as for cap_closest_points and cap_trace_rays_multi_ex: device pointers on the
 * context's GPU, asynchronous on the context stream and ordered behind a render's second lane; n above 2^24 split into launches;
 * nothing of the render's state is touched.  Errors: CAP_ERR_STATE before cap_bvh_build and while the trees are stale;
 * CAP_ERR_INVALID_ARG for any ray_flags bit, non-zero reserved words, instance_mask > 0xFF, unknown multi flags, k > CAP_MULTI_MAX_K,
 * k = 0 with output given or counts NULL, CAP_MULTI_CONTINUE with k = 0, NULL points (or output with k > 0), points or output not
 * 16-byte or counts not 4-byte aligned, any overlap between the point, output and count ranges, and n * k records beyond the address
 * space.  Nothing is written on an error; n = 0 does nothing.
 * Not covered: a lower bound from the cursor (a later page walks the subtrees the earlier pages exhausted again), and what
 * cap_closest_points leaves out. */
int cap_closest_points_multi(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, uint32_t k, CapClosest* device_out,
                             uint32_t* device_counts, uint32_t multi_flags, const CapTraceOptions* options /* may be NULL */);

/* ---- sphere sweep queries: the first contact of a moving sphere with the scene (character and camera controllers, continuous
 * collision detection, thick-ray picking, clearance along a path) ----
 * For every sweep the first time t in [0, tmax] at which the sphere of radius r centred at c(t) = o + t d touches a triangle of the
 * uploaded scene, and where it touches.  Lengths are in units of d; d is not normalised for the caller.  Walks the binary tree of the
 * scene and stays current under cap_scene_update_vertices + cap_bvh_refit like every other query.
 *
 * The per-triangle function is defined on the stored record (v0, e1, e2) and the computed vertices B1 = fl(v0 + e1), B2 = fl(v0 + e2).
 * Every operation is one rounded binary32 operation in the order written, there is no fused multiply-add anywhere, division and sqrt
 * are correctly rounded, dot and cross are the forms of the closest-point and triangle overlap contracts, and a vector operation is
 * component-wise -- so a plain float32 brute force is bit-identical to the kernel.  r2 = fl(r r), dd = dot(d, d).
 *   (A) Start overlap.  cap_closest_points' cascade at o.  If its dist2 <= r2 the triangle's time is t = 0 and its record is that
 *       cascade's; (B) and (C) are not evaluated.
 *   (B) Candidate times, only if dd != 0 (d = 0, or so small that dd underflows to 0, is a static overlap test: part (A) alone).  A
 *       time counts iff it satisfies the conditions written with it and t > 0 && t <= tmax; every condition is a comparison that a NaN
 *       fails.  The triangle's candidate is the smallest time that counts (none: no contact); it is finite.
 *       root(a, b, c):  disc = b*b - a*c,  t = (-b - sqrt(disc)) / a,  counts iff a > 0.
 *       vertex(m):      root(dd, dot(m, d), dot(m, m) - r2).
 *       edge(m, e):     ee = dot(e, e), me = dot(m, e), de = dot(d, e), md = dot(m, d), mm = dot(m, m),
 *                       t = root(ee*dd - de*de, ee*md - de*me, ee*(mm - r2) - me*me),  s = me + t*de,  counts iff s >= 0 && s <= ee.
 *       With m0 = o - v0, m1 = o - B1, m2 = o - B2 the seven pieces are
 *       plane:    n = cross(e1, e2), nn = dot(n, n), h = dot(n, m0), nd = dot(n, d),
 *                 num = |h| - r*sqrt(nn),  den = (h >= 0 ? -nd : nd),  t = num / den,
 *                 w = (o + t*d) - v0,  a = dot(cross(w, e2), n),  b = dot(cross(e1, w), n),
 *                 counts iff den > 0 && a >= 0 && b >= 0 && a + b <= nn   (the offset plane on o's side, the foot point inside);
 *       edges:    edge(m0, e1), edge(m0, e2), edge(m1, e2 - e1);
 *       vertices: vertex(m0), vertex(m1), vertex(m2).
 *       The candidate is then polished: c is a binary32 point up to an ulp of |o| + t |d| off the line, so for a time that is right to
 *       the last bit the centre lands outside the offset surface as often as inside.  At most three evaluations k = 0, 1, 2 from
 *       t_0 = the candidate: c = o + t_k*d, cap_closest_points' cascade at c gives dist2 and point.  If (C) accepts, t = t_k.  Else,
 *       for k < 2, a Newton step on the distance, lengthened by a nudge of sixteen roundings of the coordinates' size:
 *         dist = sqrt(dist2),  g = c - point,  rate = -dot(g, d),  size = max(|c|_inf, |point|_inf) + r,
 *         t_(k+1) = t_k + (((dist - r) + (16 x 2^-24)*size) * dist) / rate,   counts iff rate > 0 && t_(k+1) <= tmax;
 *       a step that does not count, or a third refusal, leaves the triangle without a contact.  Times only grow.
 *   (C) Verification and record.  c = o + t*d (fl(o + fl(t d)) per component), cap_closest_points' cascade at c.  The candidate is
 *       accepted iff that dist2 <= fl(r2 * (1 + kappa)), kappa = 8 x 2^-24 (1 + kappa is a binary32 number).  The hit's point, u, v
 *       and feature are that cascade's words, bit for bit.
 * So every reported contact is, by the library's own closest-point function, a centre position that touches the triangle: the contact
 * normal is (c - point) and the penetration at a start overlap r - |o - point|.  kappa covers the roundings that scale with r
 * (DESIGN.md "Sphere sweep queries" derives it); those that scale with the coordinates are what the polish is for, and a polished
 * contact penetrates by a few of those roundings.  With exactly representable data the first evaluation accepts and t is the entry
 * time itself.  From an origin many scene sizes away the quadratics of (B) cancel and the candidate is off by about 2^-24 |o|^2 / r:
 * three evaluations may not reach the surface, and such a sweep can miss; start it near the scene.
 *
 * The answer.  Among the triangles that pass the mask filter and have a contact, the one minimal in (t, triangle) lexicographic order,
 * the tie rule of every other query: the answer depends on neither the tree, nor the builder, nor the visiting order.  The miss record
 * is (0, 0, 0, tmax, 0, 0, 0xFFFFFFFF, 0).  Degenerate queries -- a non-finite origin or direction component, a radius or tmax that is
 * NaN or negative -- are not traversed and give the miss record with t = 0.  tmax = +inf is legal; r = 0 is legal (then (C) asks for a computed dist2 of exactly 0: use a small positive radius for a thick ray), has this arithmetic
 * and is not promised equal to cap_trace_rays; r = +inf is a start overlap with every triangle whose cascade is not NaN.  A NaN anywhere
 * in a triangle's evaluation fails its comparisons and the triangle is never an answer; a triangle with two coinciding vertices behaves
 * as in the closest-point contract.
 *
 * Conventions are cap_closest_points': device pointers on the context's GPU, both 16-byte aligned, ranges ("sweeps", "hits") that do
 * not overlap; asynchronous on the context stream and ordered behind a render's second lane; n above 2^24 split into launches, n = 0
 * does nothing; nothing of the render's state is touched; nothing is written on an error.  CAP_ERR_STATE before cap_bvh_build and
 * while the trees are stale.  options: instance_mask and the mesh-mask table act by mesh as for points; any ray_flags bit is
 * CAP_ERR_INVALID_ARG (the sweep is two-sided), as are non-zero reserved words and instance_mask > 0xFF; NULL is the plain call.
 * Not covered: k nearest contacts and paging, other swept shapes, per-query masks, a time of exit, rotation.  cap_sweep_instances
 * (below) is the form over the instance table. */
typedef struct CapSweepDesc /* 32 B, 16-aligned: DXR RayDesc's shape with the radius where tmin is */
{
    float origin[3];
    float radius; /* >= 0 */
    float direction[3];
    float tmax; /* >= 0; +inf: unbounded */
} CapSweepDesc;
typedef struct CapSweepHit /* 32 B: CapClosest's layout with t where dist2 is */
{
    float    point[3]; /* the contact point on the triangle */
    float    t;        /* the time of first contact; tmax on a miss */
    float    u, v;     /* point = v0 + u*e1 + v*e2 */
    uint32_t triangle; /* global id; 0xFFFFFFFF = miss */
    uint32_t feature;  /* CAP_FEATURE_*: where on the triangle the contact lies */
} CapSweepHit;
int cap_sweep_spheres(CapContext* ctx, const CapSweepDesc* device_sweeps, uint64_t n, CapSweepHit* device_out,
                      const CapTraceOptions* options /* may be NULL */);

/* ---- sphere sweep queries over instances: the first contact of a moving sphere with an assembly of placed parts ----
 * cap_sweep_spheres over the instance table of cap_instances_set: for every WORLD-space sweep the first time t in [0, tmax] at which the
 * sphere touches a triangle of an instance, where, and of which instance.  A non-rigid transform does not keep a sphere a sphere, so
 * nothing is evaluated in object space: the answer is defined, and the trees are pruned, in world space.  CapSweepDesc and CapSweepHit
 * are unchanged.
 *
 * Candidates are cap_closest_instances' pairs (i, g) by its rules: instance i is live, g is a triangle of i's object (every triangle
 * of the scene without an object table), and desc[i].mask & mesh_mask[m] & instance_mask != 0, m the mesh of g.
 *
 * The per-pair function is cap_sweep_spheres' -- parts (A), (B) with its polish (the nudge of sixteen roundings, at most three
 * evaluations) and (C) with kappa = 8 x 2^-24, operation by operation as written there -- evaluated on the WORLD RECORD of
 * cap_closest_instances in the place of the stored record: from M = desc[i].transform as the caller gave it and the stored (v0, e1, e2),
 *   v0w_r = fl(dot_c(M_r.xyz, v0) + M_r.w),  e1w_r = dot_c(M_r.xyz, e1),  e2w_r = dot_c(M_r.xyz, e2),
 *   dot_c(a, b) = fl(fl(fl(a.x b.x) + fl(a.y b.y)) + fl(a.z b.z)),
 * no fused multiply-add; the computed vertices are B1 = fl(v0w + e1w) and B2 = fl(v0w + e2w).  The sweep's origin, direction, radius
 * and tmax enter as given.  So a float32 brute force -- the world records, then cap_sweep_spheres' per-triangle function on each --
 * is bit-identical to the kernel.
 *
 * The answer.  Among the candidate pairs that have a contact, the one minimal in (t, instance, triangle) lexicographic order: it
 * depends on neither the trees, nor the builders, nor the visiting order.  The hit's point, u, v and feature are the cascade's words on
 * the winner's world record at c = fl(o + fl(t d)), or at o itself when t = 0; point is in world space; triangle is the scene's global
 * id.  device_instances[j] (may be NULL) is the winner's index in the instance table, 0xFFFFFFFF on a miss and for a degenerate sweep.
 * The miss record (0, 0, 0, tmax, 0, 0, 0xFFFFFFFF, 0) and the degenerate sweeps with their record (t = 0) are cap_sweep_spheres'.
 * Inert instances (below, "Inert instances") contribute nothing.
 *
 * Three identities hold and are tested.  (1) One identity instance (M = I with translation +0) gives cap_sweep_spheres' record bit for
 * bit, with one exception: the world record turns a -0 into +0 -- a vertex coordinate by v0w_r = fl(dot_c(M_r.xyz, v0) + 0), an edge
 * component by dot_c itself, whose products with the zeros of M_r are +0 or -0 and sum to -0 only when all three are -0 -- so a
 * triangle with a vertex coordinate or an edge component -0 enters as if that word were +0, and a word of the record's point (or of
 * u, v) that depends on the sign of such a zero may differ in the sign of a zero, nothing else.  (2) Pure translations, with vertices,
 * translations and sweeps on a common power-of-two grid coarse enough that every v0 + translation is exact, give the answer of the
 * flattened scene with flat id i T + g (T the triangle count).  (3) Scaling every M (translation included), every origin, every radius
 * and every direction by 2^j leaves t, u, v, both ids and the feature unchanged and scales point by 2^j, short of overflow and
 * underflow: no absolute term enters the per-pair function, so the identity is exact.
 *
 * Conventions, errors and their order are cap_sweep_spheres': any ray_flags bit, non-zero reserved words and instance_mask > 0xFF are
 * CAP_ERR_INVALID_ARG; then CAP_ERR_STATE before cap_bvh_build and while the trees are stale, and CAP_ERR_STATE without an instance
 * table, where the other instanced queries have it; then n = 0 does nothing; NULL sweeps or output; the ranges "sweeps" and "hits"
 * (32 bytes each, 16-byte aligned) and, when given, "instances" (4 bytes each, 4-byte aligned), none of which may overlap another.
 * Nothing is written on an error; n above 2^24 is split into launches; nothing of the render's state is touched.  The query is
 * current under cap_scene_update_vertices + cap_bvh_refit, under cap_instances_set again and under cap_objects_set.
 * Not covered: k nearest contacts and paging, other swept shapes, a time of exit, rotation, per-query masks. */
int cap_sweep_instances(CapContext* ctx, const CapSweepDesc* device_sweeps, uint64_t n, CapSweepHit* device_out,
                        uint32_t* device_instances /* may be NULL */, const CapTraceOptions* options /* may be NULL */);

/* ---- box overlap queries: the triangles that meet an axis-aligned box (collision broad phase, voxelisation, selection, clipping) ----
 * For every box the triangles of the uploaded scene that meet the CLOSED box [lo, hi], on the scene's binary tree: the first k of them
 * by triangle id, their number, or both, with cap_closest_points_multi's pages, counts, paging and masks.  Current under
 * cap_scene_update_vertices + cap_bvh_refit like every other query.
 *
 * The predicate is the separating-axis test of a triangle and a box (Akenine-Moller 2001) with all 13 axes, defined on the STORED
 * record (v0, e1, e2) as cap_closest_points' function is.  Every operation is one rounded binary32 operation in the order written, there
 * is no fused multiply-add, dot is the point queries' dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z -- so a plain float32 brute force is
 * bit-identical to the kernel.  Let a = v0, b = fl(v0 + e1), c = fl(v0 + e2).  The triangle meets the box unless one of these separates
 * them (each is a pure comparison, the order of evaluation is free):
 *   1. Box axes, absolute coordinates, exact comparisons: for x, y, z:  min(a_x, b_x, c_x) > hi_x  or  max(a_x, b_x, c_x) < lo_x.
 *   2. The centred frame, component-wise: hl = lo*0.5, hh = hi*0.5, ctr = hl + hh, h = hh - hl (neither overflows for finite input);
 *      P0 = a - ctr, P1 = b - ctr, P2 = c - ctr; edges f0 = e1, f1 = P2 - P1, f2 = P0 - P2.
 *   3. Nine cross axes: for each edge f and each coordinate pair (m, n) in {(y, z), (z, x), (x, y)}:
 *        s_j = f_m*P_j,n - f_n*P_j,m for j = 0, 1, 2 (all three are evaluated),  r = h_m*|f_n| + h_n*|f_m|;
 *        min(s_0, s_1, s_2) > r  or  max(s_0, s_1, s_2) < -r.
 *   4. The triangle's plane: n = (e1_y*e2_z - e1_z*e2_y, e1_z*e2_x - e1_x*e2_z, e1_x*e2_y - e1_y*e2_x), d = dot(n, P0),
 *        r = (h_x*|n_x| + h_y*|n_y|) + h_z*|n_z|;  d > r  or  d < -r.
 * min and max hand a NaN on, and a NaN fails its comparison: an axis with a NaN among its values separates nothing ("min > r" reads
 * "all three > r").  Touching is overlap: a box face coplanar with a triangle, a box that shares only an edge or a corner with it, a
 * point box (lo == hi) on a vertex or in the face all count; one ulp back they do not.  A zero-area triangle is a segment or a point
 * to the axes above and is listed where that meets the box.
 *
 * The answer.  A box's candidates are the triangles that pass the mask filter (the mesh-mask table and instance_mask, exactly as in
 * cap_closest_points) and the predicate, sorted by triangle id ascending.  device_triangles[i * k + j], j < k, is box i's j-th
 * candidate; slots after the last hold 0xFFFFFFFF.  device_counts: NULL, or n uint32: the number of ALL candidates of box i, not capped
 * at k (with CAP_MULTI_CONTINUE: of those above the cursor).  k = 0 counts only: device_triangles must be NULL and device_counts given.
 * The answer depends on neither the tree, nor the builder, nor the visiting order.
 *
 * Paging (CAP_MULTI_CONTINUE): on entry, slot k - 1 of each box's page is read as the cursor g_c; only candidates with id > g_c count
 * and are listed, and the next page is written over the old one.  A page that was not full ends in 0xFFFFFFFF, which admits nothing:
 * that box's next page is empty.  Calling again with the same boxes and buffer walks every candidate exactly once.
 *
 * Degenerate boxes -- a non-finite coordinate, or lo > hi on some axis -- are not traversed: a page of 0xFFFFFFFF and count 0, with
 * CAP_MULTI_CONTINUE too.  lo = -FLT_MAX, hi = FLT_MAX is a legal box and lists everything.  The pad words are not read.
 *
 * Conventions and errors are cap_closest_points_multi's: device pointers on the context's GPU, boxes 16-byte and ids and counts 4-byte
 * aligned, ranges that do not overlap; asynchronous on the context stream and ordered behind a render's second lane; n above 2^24 split
 * into launches, n = 0 does nothing; nothing of the render's state is touched; nothing is written on an error.  CAP_ERR_STATE before
 * cap_bvh_build and while the trees are stale; CAP_ERR_INVALID_ARG for any ray_flags bit, non-zero reserved words,
 * instance_mask > 0xFF, unknown multi flags, k > CAP_MULTI_MAX_K, k = 0 with a page given or counts NULL, CAP_MULTI_CONTINUE with
 * k = 0, NULL boxes (or page with k > 0), misaligned or overlapping ranges, and n * k ids beyond the address space.
 * Not covered: oriented boxes, a lower bound from the cursor (a later page walks the whole box again), per-box masks.  The boxes are in
 * the scene's own space; over instances and objects: cap_overlap_instances below. */
typedef struct CapBoxDesc /* 32 B, 16-byte aligned */
{
    float lo[3];
    float pad0; /* not read */
    float hi[3];
    float pad1; /* not read */
} CapBoxDesc;
int cap_overlap_boxes(CapContext* ctx, const CapBoxDesc* device_boxes, uint64_t n, uint32_t k, uint32_t* device_triangles /* n*k ids */,
                      uint32_t* device_counts /* n or NULL */, uint32_t multi_flags, const CapTraceOptions* options /* may be NULL */);

/* ---- box overlap queries over instances: which triangles of which placed parts meet a world-space box ----
 * cap_overlap_boxes over the instance table of cap_instances_set (and the objects of cap_objects_set), as cap_closest_instances_multi
 * stands to cap_closest_points_multi.  The boxes are axis-aligned in WORLD space.
 *
 * Candidates.  A box's candidates are the pairs (instance i, triangle g) of cap_closest_instances: i is not inert; with an object table
 * g is a triangle of i's object; desc[i].mask & mesh_mask[m] & instance_mask != 0 (m the mesh of g).  The pair is a candidate where its
 * WORLD record meets the box under cap_overlap_boxes' predicate, unchanged.  The world record is cap_closest_instances', built from
 * M = desc[i].transform as the caller gave it, with dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, one rounded binary32 operation per
 * operation written and no fused multiply-add:
 *   v0w_r = fl(dot(M_r.xyz, v0) + M_r.w),  e1w_r = dot(M_r.xyz, e1),  e2w_r = dot(M_r.xyz, e2),   r = x, y, z;
 * the predicate's vertices are a = v0w, b = fl(v0w + e1w), c = fl(v0w + e2w), its e1 and e2 are e1w and e2w.  A NumPy float32 brute force
 * over every (instance, triangle) is bit-identical, whichever builder made the trees.
 *
 * Order and pages.  The pairs sort by (i, g) ascending.  device_triangles[b * k + j] and device_instances[b * k + j], j < k, are box
 * b's j-th pair; slots after the last pair hold 0xFFFFFFFF in both pages.  device_counts: NULL, or n uint32: the number of ALL
 * candidates of the box, not capped at k (with CAP_MULTI_CONTINUE: of those above the cursor).  k = 0 counts only: both pages must be
 * NULL and device_counts given.
 *
 * Paging (CAP_MULTI_CONTINUE): on entry slot k - 1 of both pages is read as the cursor (i_c, g_c); only pairs lexicographically above
 * it count and are listed, and the next pages are written over the old ones.  (0xFFFFFFFF, 0xFFFFFFFF) -- a page that was not full --
 * admits nothing.  device_instances is therefore required whenever k > 0, as in cap_closest_instances_multi.
 *
 * Degenerate boxes are cap_overlap_boxes': not traversed, pages of 0xFFFFFFFF, count 0.  lo = -FLT_MAX, hi = FLT_MAX is legal and
 * lists every live, unmasked pair.
 *
 * Identities (tested on the reference and on the device):
 *   1. One identity instance gives cap_overlap_boxes' ids and counts: 1*x + 0*y + 0*z is exact for finite x -- only the sign of a zero
 *      can change, and no comparison of the predicate sees it.
 *   2. With pure translations, vertices and boxes on a common power-of-two grid (every sum exact) the answer is the flattened scene's
 *      under cap_overlap_boxes, with flat id = i * T + g, T the scene's triangle count.
 *   3. Scaling every M (matrix and translation) and every box by 2^j changes nothing, short of overflow and underflow.
 *
 * Conventions and errors are cap_closest_instances_multi's word for word, with the four ranges "boxes", "triangles", "instances" and
 * "counts": device pointers on the context's GPU, boxes 16-byte and triangles, instances and counts 4-byte aligned, ranges that do not
 * overlap; asynchronous on the context stream; n above 2^24 split into launches with all three outputs advanced per chunk, n = 0 does
 * nothing; nothing is written on an error.  CAP_ERR_STATE without an instance table, before cap_bvh_build and while the trees are
 * stale; CAP_ERR_INVALID_ARG for any ray_flags bit, non-zero reserved words, instance_mask > 0xFF, unknown multi flags,
 * k > CAP_MULTI_MAX_K, k = 0 with a page given or counts NULL, CAP_MULTI_CONTINUE with k = 0, NULL boxes (or either page with k > 0),
 * misaligned or overlapping ranges.
 * Pruning is conservative for every live instance (DESIGN.md "Box overlap queries over instances"; cap_debug_overlap_instance_prune
 * shows its arithmetic).  Not covered: oriented boxes, per-box masks, the wide view, a lower bound inside an instance from the cursor's
 * triangle (an instance below the cursor's is not entered; the cursor's own is walked again). */
int cap_overlap_instances(CapContext* ctx, const CapBoxDesc* device_boxes, uint64_t n, uint32_t k, uint32_t* device_triangles /* n*k */,
                          uint32_t* device_instances /* n*k */, uint32_t* device_counts /* n or NULL */, uint32_t multi_flags,
                          const CapTraceOptions* options /* may be NULL */);

/* ---- triangle overlap queries: the triangles of the scene that meet a given triangle (contact, self-intersection, cutting, clearance) ----
 * cap_overlap_boxes with a triangle for the box: for every query triangle (a, b, c) the triangles of the uploaded scene that meet it,
 * on the scene's binary tree -- the first k of them by triangle id, their number, or both.  Current under cap_scene_update_vertices +
 * cap_bvh_refit like every other query.  A segment (two vertices equal) and a point (all three equal) are legal queries.
 *
 * The predicate is the separating-axis test of two triangles with 17 axes, in the frame of the query's first vertex, defined on the
 * query's vertices as given and on the STORED record (v0, e1, e2) of the scene triangle.  Every operation written is one rounded
 * binary32 operation, there is no fused multiply-add, dot is the point queries' dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z and
 * cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x) -- so a plain float32 brute force is bit-identical to the
 * kernel.  Query vertices A0 = a, A1 = b, A2 = c.  Scene vertices B0 = v0, B1 = fl(v0 + e1), B2 = fl(v0 + e2): the computed vertices
 * of cap_overlap_boxes.  The triangles meet unless one of these separates them (each is a pure comparison, the order of evaluation is
 * free):
 *   1. Coordinate axes, absolute coordinates, exact comparisons: for x, y, z:
 *        min(B0, B1, B2) > max(A0, A1, A2)  or  max(B0, B1, B2) < min(A0, A1, A2).
 *   2. The frame at A0: p_j = A_j - A0 (so p_0 = 0), q_j = B_j - A0; query edges f0 = p1, f1 = p2 - p1, f2 = p0 - p2; scene edges
 *      g0 = e1 (as stored), g1 = q2 - q1, g2 = q0 - q2; normals n = cross(p1, p2), m = cross(e1, e2).
 *   3. Seventeen axes L: n; m; cross(f_i, g_j) for the nine pairs; cross(n, f_i), i = 0, 1, 2; cross(m, g_j), j = 0, 1, 2.  For each,
 *        s_j = dot(L, p_j), t_j = dot(L, q_j) for j = 0, 1, 2 (all six are evaluated);
 *        min(t_0, t_1, t_2) > max(s_0, s_1, s_2)  or  max(t_0, t_1, t_2) < min(s_0, s_1, s_2).
 * min and max hand a NaN on, and a NaN fails its comparison: an axis with a NaN among its six values separates nothing.  A zero axis
 * has s = t = 0 and separates nothing.  Touching is overlap: a shared vertex, a shared edge, a vertex in a face and coplanar contact all
 * count; one ulp back, where the frame is exact, they do not.
 *
 * Completeness.  For two triangles of non-zero area the 17 axes are the complete set in the reals: the facet normals of the Minkowski
 * difference (n, m and the nine cross(f_i, g_j)) and, for the coplanar case, in which all of those are parallel to n, the in-plane
 * edge normals cross(n, f_i) and cross(m, g_j).  Step 1 is what the walk prunes with; in the reals it is implied and costs nothing.
 * Degenerate triangles.  With a zero-area triangle on either side the axes can fail to separate a pair that does not meet (two coplanar
 * segments that do not cross: every cross product of the pair vanishes or lies along the common normal) and such a pair is listed.
 * They never separate a pair that meets.  A point query a = b = c and a segment query against scene triangles of non-zero area are
 * still decided, by m, cross(f, g_j) and cross(m, g_j).
 * The float32 function is the definition: where a product rounds, a contact can be lost or won by an ulp.  It is not symmetric in
 * float32 -- swapping the roles of the two triangles changes the frame, which is the query's.
 *
 * skip: a scene triangle whose global id equals `skip` is no candidate -- applied like the mask, it is neither counted nor listed.
 * 0xFFFFFFFF (no triangle has that id) or any id beyond the scene skips nothing.  A query built from the scene's own triangle g with
 * skip = g lists what touches g, its edge and vertex neighbours included: filtering adjacency is the caller's.
 *
 * Candidates (mask filter and predicate), their order (id ascending), pages, the 0xFFFFFFFF fill, device_counts (all candidates, not
 * capped at k; with CAP_MULTI_CONTINUE: of those above the cursor), k = 0 counts only, the CAP_MULTI_CONTINUE cursor in slot k - 1,
 * masks, conventions, errors and their order are cap_overlap_boxes' word for word, with the three ranges "queries" (48 B per query,
 * 16-byte aligned), "triangles" and "counts" (4-byte aligned).  A query with a non-finite coordinate is not traversed: a page of
 * 0xFFFFFFFF and count 0, with CAP_MULTI_CONTINUE too.  The pad words are not read.
 * Not covered: a node cull finer than the box of the query's vertices; the intersection segment itself; adjacency filtering; exactness
 * for zero-area pairs; per-query masks.  The queries are in the scene's own space; over instances and objects:
 * cap_overlap_triangles_instances below. */
typedef struct CapTriangleDesc /* 48 B, 16-byte aligned */
{
    float    a[3];
    uint32_t skip; /* a scene triangle with this global id is no candidate; 0xFFFFFFFF: none */
    float    b[3];
    uint32_t pad0; /* cap_overlap_triangles: not read.  cap_overlap_triangles_instances: skip_instance -- the pair (skip_instance, skip)
                      is no candidate; with skip = 0xFFFFFFFF nothing is skipped, whatever this word holds */
    float    c[3];
    uint32_t pad1; /* not read */
} CapTriangleDesc;
int cap_overlap_triangles(CapContext* ctx, const CapTriangleDesc* device_queries, uint64_t n, uint32_t k, uint32_t* device_triangles /* n*k ids */,
                          uint32_t* device_counts /* n or NULL */, uint32_t multi_flags, const CapTraceOptions* options /* may be NULL */);

/* ---- triangle overlap queries over instances: which triangles of which placed parts a world-space triangle cuts ----
 * cap_overlap_triangles over the instance table of cap_instances_set (and the objects of cap_objects_set), as cap_overlap_instances
 * stands to cap_overlap_boxes: what a collision pipeline over an assembly asks with the world-space triangles of a moving part.  The
 * query triangles are in WORLD space; the record is the same 48-byte CapTriangleDesc.
 *
 * Candidates.  A query's candidates are the pairs (instance i, triangle g) of cap_overlap_instances, by the same rules: i is not inert;
 * with an object table g is a triangle of i's object; desc[i].mask & mesh_mask[m] & instance_mask != 0 (m the mesh of g).  The pair is
 * a candidate where its WORLD record (v0w, e1w, e2w) meets the query under cap_overlap_triangles' 17-axis predicate, unchanged.  The
 * world record is cap_closest_instances', built from M = desc[i].transform as the caller gave it with
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, one rounded binary32 operation per operation written and no fused multiply-add:
 *   v0w_r = fl(dot(M_r.xyz, v0) + M_r.w),  e1w_r = dot(M_r.xyz, e1),  e2w_r = dot(M_r.xyz, e2),   r = x, y, z;
 * the predicate's scene vertices are B0 = v0w, B1 = fl(v0w + e1w), B2 = fl(v0w + e2w), its g0 is e1w as computed and its
 * m = cross(e1w, e2w).  A NumPy float32 brute force over every (query, instance, triangle) is bit-identical, whichever builder made
 * the trees.
 *
 * The skip pair.  This call reads the pad0 word as skip_instance: a pair with i == skip_instance and g == skip is no candidate --
 * applied like the mask, it is neither counted nor listed.  A skip of 0xFFFFFFFF skips nothing, whatever pad0 holds, so zeroed pads
 * with the default skip stay harmless.  pad1 is not read.  A query built from the world record of triangle g of instance i with the
 * skip pair (i, g) lists what touches that placed triangle in the rest of the assembly and in its own instance: self-contact of an
 * instance against the assembly.  Skipping a whole instance per query is not covered; per call the instance masks do it.
 *
 * Order, pages, counts and paging are cap_overlap_instances' word for word.  The pairs sort by (i, g) ascending.
 * device_triangles[q * k + j] and device_instances[q * k + j], j < k, are query q's j-th pair; slots after the last pair hold
 * 0xFFFFFFFF in both pages.  device_counts: NULL, or n uint32: the number of ALL candidates of the query, not capped at k (with
 * CAP_MULTI_CONTINUE: of those above the cursor).  k = 0 counts only: both pages must be NULL and device_counts given.  With
 * CAP_MULTI_CONTINUE slot k - 1 of both pages is read on entry as the cursor (i_c, g_c); only pairs lexicographically above it count
 * and are listed, and the next pages are written over the old ones.  (0xFFFFFFFF, 0xFFFFFFFF) -- a page that was not full -- admits
 * nothing.  device_instances is therefore required whenever k > 0.
 *
 * A query with a non-finite coordinate is not traversed: pages of 0xFFFFFFFF and count 0, with CAP_MULTI_CONTINUE too.
 *
 * Identities (tested on the reference and on the device):
 *   1. One identity instance gives cap_overlap_triangles' ids and counts (1*x + 0*y + 0*z is exact for finite x; only the sign of a
 *      zero can change, and no comparison of the predicate sees it); there skip_instance = 0.
 *   2. With pure translations, vertices and queries on a common power-of-two grid (every sum exact) the answer is the flattened
 *      scene's under cap_overlap_triangles, with flat id = i * T + g, T the scene's triangle count.
 *   3. Scaling every M (matrix and translation) and every query by 2^j changes nothing, short of overflow and underflow.
 *
 * Conventions, errors and their order are cap_overlap_instances' word for word, with the four ranges "queries" (48 B per query,
 * 16-byte aligned), "triangles", "instances" and "counts" (4-byte aligned): device pointers on the context's GPU, ranges that do not
 * overlap; asynchronous on the context stream; n above 2^24 split into launches with all three outputs advanced per chunk, n = 0 does
 * nothing; nothing is written on an error.  CAP_ERR_STATE without an instance table, before cap_bvh_build and while the trees are
 * stale; CAP_ERR_INVALID_ARG for any ray_flags bit, non-zero reserved words, instance_mask > 0xFF, unknown multi flags,
 * k > CAP_MULTI_MAX_K, k = 0 with a page given or counts NULL, CAP_MULTI_CONTINUE with k = 0, NULL queries (or either page with
 * k > 0), misaligned or overlapping ranges.
 * Pruning is conservative for every live instance: the walk tests the world box of every node of the object's tree against the box of
 * the query's vertices -- not the object-space image of that box, which the triangle predicate does not justify (DESIGN.md "Triangle
 * overlap queries over instances"; cap_debug_overlap_world_node shows the arithmetic).  Not covered: a finer node cull; per-query
 * masks and whole-instance skip; the intersection segment; a lower bound inside an instance from the cursor's triangle (an instance
 * below the cursor's is not entered; the cursor's own is walked again). */
int cap_overlap_triangles_instances(CapContext* ctx, const CapTriangleDesc* device_queries, uint64_t n, uint32_t k, uint32_t* device_triangles /* n*k */,
                                    uint32_t* device_instances /* n*k */, uint32_t* device_counts /* n or NULL */, uint32_t multi_flags,
                                    const CapTraceOptions* options /* may be NULL */);

/* ---- instanced ray queries: N transformed instances of the uploaded scene, or of objects of it, under a device-built top-level tree ----
 * The uploaded scene and the trees cap_bvh_build makes of it are read as OBJECT space; cap_instances_set installs a table of N
 * instances of it, each with an object-to-world transform and an 8-bit mask, and builds a top-level tree (TLAS) over the instances'
 * world boxes on the device.  cap_trace_instances / cap_trace_instances_occlusion walk TLAS -> ray into object space -> the binary
 * tree of the scene.  Nothing else changes: the plain cap_trace_rays* calls keep tracing the object-space scene, cap_render ignores
 * the table (as it ignores the mesh masks).
 *
 * Objects (cap_objects_set, below).  Without an object table an instance shows the whole scene.  With one, the scene is a container
 * of OBJECTS -- contiguous mesh ranges, hence contiguous ranges of global triangle ids -- each with a binary tree of its own (a
 * bottom-level structure in DXR's terms), and every instance shows ONE object (cap_instances_set_ex's object_index; plain
 * cap_instances_set shows object 0).  Everything below holds with "scene" read as "the instance's object": the hit set of an instance
 * holds triangles of its object only, its world box is the image of the object's bounds, and the walk below it visits the object's
 * tree alone.  `triangle` stays the scene's global id, mesh masks stay per mesh of the scene.
 *
 * World-to-object.  Per instance the library computes W = fl32(inverse(M)) once, the inverse of the affine map taken in double and
 * each of its twelve entries rounded once to binary32.  W as stored is part of the contract (cap_instances_readback returns it);
 * everything below is defined from W, not from M.
 * Object-space ray (the DXR rule: the direction is not normalised, so t means the same on both sides), row r of W:
 *   o'_r = dot(W_r.xyz, o) + W_r.w      d'_r = dot(W_r.xyz, d)      dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))
 * with one rounded add; tmin and tmax unchanged.  An object-space ray that is degenerate by the queries' rule (a non-finite
 * component, zero direction) has no hit in that instance.
 * Hit set of a ray: the pairs (instance i, triangle g) with i not inert, g passing the closest (cap_trace_instances) or occlusion
 * (cap_trace_instances_occlusion) triangle test against ray's object-space ray in instance i, and the filters.  The closest record
 * is the minimum in (t, i, g) lexicographic order: the existing tie rule with the instance in front, so the answer depends on
 * neither tree nor on the visiting order.  (u, v) are object-space barycentrics, `triangle` the global triangle id of the scene.
 * Filters (CapTraceOptions): facing is decided in object space from det's sign exactly as in cap_trace_rays_ex and is NOT affected
 * by the instance transform, a mirroring one included (the DXR rule).  A triangle of mesh m in instance i is a candidate iff
 * desc[i].mask & mesh_mask[m] & instance_mask != 0 (instance_mask = 0 means 0xFF; mesh masks are 0xFF unless
 * cap_scene_set_instance_masks set them).  The masks are for visibility groups.  They can also stand in for objects -- meshes with
 * masks 1 << k, each instance given the bit of what it shows -- and that is still the right tool for switching PARTS of an object on
 * and off per instance (at most eight, sharing one tree); for different objects in different places use cap_objects_set: under the
 * mask trick every instance has the scene's box and its walk tests every object's triangles before the mask rejects them.
 * CAP_RAY_FLAG_ACCEPT_FIRST_HIT on cap_trace_instances returns some
 * member of the set, a miss exactly when it is empty.
 * Inert instances.  An instance whose transform has a non-finite entry, is singular, whose inverse does not fit binary32, or whose
 * condition number kappa = ||W^-1||_inf * ||W||_inf (3x3 parts, row-sum norms, W as stored) exceeds CAP_INSTANCE_MAX_CONDITION is
 * INERT: never hit, counted in CapInstancesInfo::inert, not an error; decided on the device, the same for host and device
 * descriptors.  Its read-back W is all zero and its box empty (lo = +inf, hi = -inf).  The bound is the domain in which the
 * top-level boxes are proven conservative for the rounded object-space ray (DESIGN.md "Instances"); any transform with a 2-norm
 * condition number up to CAP_INSTANCE_MAX_CONDITION / 3 is inside it. */
#define CAP_INSTANCE_MAX_CONDITION 4096.0
#define CAP_INSTANCE_MAX_COUNT (1u << 24) /* DXR's limit */
typedef struct CapInstanceDesc /* 64 B */
{
    float    transform[12]; /* object-to-world, row-major 3x4 (rows of the rotation / scale part, translation in column 3) */
    uint32_t mask;          /* InstanceMask, low 8 bits; 0 = never hit, as in DXR */
    uint32_t reserved[3];   /* must be 0 */
} CapInstanceDesc;
enum
{
    CAP_INSTANCES_DEVICE = 1u << 0 /* descs is a device pointer on the context's GPU, read on the context stream; never copied to the host */
};
typedef struct CapInstancesInfo
{
    uint32_t count, inert, tlas_nodes, tlas_depth;
    double   ms; /* host time of the call; includes the wait for the device only when the call waits (see below) */
} CapInstancesInfo;
/* Installs (or, called again, replaces) the table and builds the TLAS: the whole cost of a rigid-motion frame.  count = 0 removes
 * the table; count <= CAP_INSTANCE_MAX_COUNT.  Needs a built tree: CAP_ERR_STATE before cap_bvh_build and while the trees are stale
 * after cap_scene_update_vertices.  Host descriptors are copied before the call returns (the call waits for the stream) and are
 * checked: non-zero reserved words are CAP_ERR_INVALID_ARG.  Device descriptors (4-byte aligned) are copied on the stream; the call
 * is asynchronous unless `out` is given (the inert count is read back).  cap_scene_upload and cap_objects_set drop the table;
 * cap_bvh_build and cap_bvh_refit keep the descriptors and rebuild world boxes and TLAS from the new bounds by the same routine;
 * cap_scene_set_instance_masks does not touch it. */
int cap_instances_set(CapContext* ctx, const CapInstanceDesc* descs, uint32_t count, uint32_t flags, CapInstancesInfo* out /* may be NULL */);
/* cap_instances_set with an object per instance.  object_index lives where descs lives -- `count` host words, or with
 * CAP_INSTANCES_DEVICE a 4-byte aligned device pointer -- and is copied like the descriptors; NULL means all 0, and
 * cap_instances_set is this call with NULL.  Without an object table every index must be 0 (the whole scene); with one it selects
 * the object.  Host indices are checked: one >= the number of objects (>= 1 without a table) is CAP_ERR_INVALID_ARG with nothing
 * installed.  Device indices are not read on the host: an out-of-range one makes the instance INERT (counted, never hit, empty box). */
int cap_instances_set_ex(CapContext* ctx, const CapInstanceDesc* descs, const uint32_t* object_index /* may be NULL */, uint32_t count,
                         uint32_t flags, CapInstancesInfo* out /* may be NULL */);
/* host arrays, either may be NULL: W (12 floats per instance, row-major 3x4) and the padded world box (lo.xyz, hi.xyz) */
int cap_instances_readback(CapContext* ctx, float* world_to_object, float* world_boxes);
/* cap_trace_rays_ex / cap_trace_occlusion_ex in every convention (device pointers, 16-byte alignment of rays and hits, no overlap,
 * asynchronous on the context stream, n above 2^24 split into launches, nothing written on an error); CAP_ERR_STATE without a
 * table.  device_instances[i] (4-byte aligned, may be NULL) is the table index of ray i's hit, 0xFFFFFFFF on a miss. */
int cap_trace_instances(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, CapHit* device_hits, uint32_t* device_instances,
                        const CapTraceOptions* options /* may be NULL */);
int cap_trace_instances_occlusion(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, uint32_t* device_occluded,
                                  const CapTraceOptions* options /* may be NULL */);
/* Multi-hit over the instances: cap_trace_rays_multi_ex's pages, counts and paging over cap_trace_instances' hit set.
 * Hit set of a ray: exactly cap_trace_instances' -- the pairs (instance i, triangle g) with i not inert, g passing the closest
 * triangle test against the ray's object-space ray in instance i, and the filters of `options` (facing in object space;
 * desc[i].mask & mesh_mask[m] & instance_mask != 0).  With an object table g ranges over the instance's object only.  Sorted by
 * (t, i, g) ascending, the order cap_trace_instances' tie rule defines; a pair appears at most once.
 * Pages: device_hits[r * k + j] and device_instances[r * k + j], j < k, are ray r's j-th pair: the CapHit holds t, object-space
 * (u, v) and the scene's global triangle id, device_instances the table index.  Slots after the last pair hold the miss record
 * (tmax, 0, 0, 0xFFFFFFFF) and instance 0xFFFFFFFF.  With k = 1 record and instance are bit-identical to what cap_trace_instances
 * writes for the same options without CAP_RAY_FLAG_ACCEPT_FIRST_HIT.  Records depend on neither tree nor on the visiting order.
 * device_counts: NULL, or n uint32: the number of ALL pairs of the set, not capped at k (with CAP_MULTI_CONTINUE: of the pairs above
 * the cursor).  Asking for counts turns off pruning by the k-th hit.  k = 0 counts only: device_hits and device_instances must be
 * NULL and device_counts given.
 * Paging (CAP_MULTI_CONTINUE): on entry, slot k - 1 of each ray's hit page and of its instance page is read as the cursor
 * (t_c, i_c, g_c); only pairs with (t, i, g) > (t_c, i_c, g_c) in lexicographic order count, and the next page is written over the
 * old one.  A short page ends in the miss record, whose cursor (tmax, 0xFFFFFFFF, 0xFFFFFFFF) admits nothing.  Calling again with the
 * same rays and buffers walks every pair exactly once, equal-t pairs of coinciding or abutting instances on either side of a page
 * boundary included (a loop over cap_trace_instances with tmin = t loses those: the interval is open).  Both cursor slots must hold
 * what the previous call wrote there.
 * Everything else is as for cap_trace_rays_multi_ex and cap_trace_instances: device pointers on the context's GPU; rays and hits
 * 16-byte, instances and counts 4-byte aligned; no overlap between any two of the four ranges; asynchronous on the context stream,
 * ordered behind a render's second lane; n above 2^24 split into launches, n = 0 does nothing; degenerate rays give miss pages and
 * count 0 (with CAP_MULTI_CONTINUE too); nothing of the render's state is touched.  Errors: CAP_ERR_STATE without an instance table,
 * before cap_bvh_build and while the trees are stale; CAP_ERR_INVALID_ARG for k > CAP_MULTI_MAX_K, k = 0 with hits or instances given
 * or counts NULL, k > 0 with hits or instances NULL, CAP_MULTI_CONTINUE with k = 0, unknown multi flags,
 * CAP_RAY_FLAG_ACCEPT_FIRST_HIT, both cull flags, unknown ray flags, non-zero reserved words, instance_mask > 0xFF, misalignment,
 * overlap, and n * k records beyond the address space.  Nothing is written on an error. */
int cap_trace_instances_multi(CapContext* ctx, const CapRayDesc* device_rays, uint64_t n, uint32_t k, CapHit* device_hits,
                              uint32_t* device_instances, uint32_t* device_counts, uint32_t multi_flags,
                              const CapTraceOptions* options /* may be NULL */);

/* ---- closest-point queries over instances: the nearest (instance, triangle) to a point, in WORLD space ----
 * cap_closest_points over the instance table of cap_instances_set(_ex): proximity and collision tests, ICP, snapping and distance
 * fields against scenes built from instances, where a rigid-motion frame costs one cap_instances_set and no rebuild.  "Nearest" is
 * defined where the caller means it, in world space, on the instance's TRANSFORMED triangle -- an affine transform that is not rigid
 * does not preserve nearest, so the object-space answer would be a different one.  Any live instance works: rotation, non-uniform
 * scale, shear, mirror.
 *
 * World record.  For instance i and triangle g take M = desc[i].transform exactly as the caller gave it (binary32, row-major 3x4; NOT
 * the stored inverse W the ray queries are defined from) and the stored intersection record (v0, e1, e2) of g.  Per row r of M:
 *   v0w_r = fl(dot_c(M_r.xyz, v0) + M_r.w)     e1w_r = dot_c(M_r.xyz, e1)     e2w_r = dot_c(M_r.xyz, e2)
 *   dot_c(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 * dot_c is the POINT queries' dot product: every operation one rounded binary32 operation in the order written, and -- unlike the
 * instanced ray transform -- no fused multiply-add anywhere in this query, so that a vectorised float32 brute force is bit-identical.
 * Per-triangle function: cap_closest_points' Voronoi cascade, unchanged, applied to (v0w, e1w, e2w) and the world point p; it gives
 * dist2, u, v, feature and point = v0w + m.
 *
 * Candidates.  A pair (i, g) is a candidate iff instance i is not inert; with an object table, g is a triangle of i's object;
 * desc[i].mask & mesh_mask[m] & instance_mask != 0 for g's mesh m (the instanced ray rule; instance_mask = 0 means 0xFF);
 * and dist2 <= r2, r2 = fl(radius * radius).  A NaN dist2 is never a candidate.
 * Answer: the candidate minimal in (dist2, i, g) lexicographic order; it depends on neither tree nor on the visiting order.
 * device_out[j] is a CapClosest with point = the world-space closest point, dist2 = the world-space squared distance, (u, v) = the
 * barycentric weights (they address the object-space triangle as well), triangle = the scene's global triangle id, feature as in
 * cap_closest_points.  device_instances[j] (may be NULL) is the table index, 0xFFFFFFFF on a miss.  The miss record is exactly
 * cap_closest_points': (0, 0, 0, r2, 0, 0, 0xFFFFFFFF, 0); degenerate points (a non-finite coordinate, a NaN or negative radius) are
 * not traversed and give the miss record with dist2 = 0.
 *
 * Identities (each one is tested):
 *   1. one identity instance, no negative zero in the scene: the records are bit-identical to cap_closest_points';
 *   2. translations and vertices on a common power-of-two grid (every sum exact): the records equal cap_closest_points' over the
 *      flattened scene, flat id = i * T + g for T triangles;
 *   3. M (linear part and translation), and the point and radius, all scaled by 2^k: dist2 scales by 4^k and point by 2^k; u, v, feature
 *      and the winner are unchanged, absent under- and overflow.
 *
 * Conventions are cap_closest_points' and cap_trace_instances': device pointers on the context's GPU, points and output 16-byte
 * aligned, instances 4-byte aligned, no overlap between any two of the three ranges; asynchronous on the context stream and ordered
 * behind a render's second lane; n above 2^24 split into launches, n = 0 does nothing; nothing is written on an error; nothing of the
 * render's state is touched.  CAP_ERR_STATE before cap_bvh_build, while the trees are stale after cap_scene_update_vertices, and
 * without an instance table.  CAP_ERR_INVALID_ARG for any ray_flags bit, non-zero reserved words, instance_mask > 0xFF, NULL points or
 * output, misalignment, overlap.
 * Pruning never decides: the top-level boxes and the objects' trees are pruned with a bound that is proven conservative for every
 * live instance (DESIGN.md "Closest-point queries over instances"; cap_debug_closest_instance_bound shows its arithmetic).
 * Not covered: per-point masks, the wide view.  The k nearest, counts and paging: cap_closest_instances_multi below.  The sign of the
 * distance: cap_signed_distance_instances further below. */
int cap_closest_instances(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out,
                          uint32_t* device_instances /* may be NULL */, const CapTraceOptions* options /* may be NULL */);

/* ---- k nearest and in-radius closest-point queries over instances: the SET of (instance, triangle) pairs near a point ----
 * cap_closest_points_multi's pages, counts and paging over cap_closest_instances' candidates: contact generation against rigidly
 * moving parts, robust ICP, "how many triangles of which instances lie within r", without flattening the scene.
 * Candidates of a point: exactly cap_closest_instances' -- the pairs (instance i, triangle g) with i not inert; with an object table,
 * g a triangle of i's object; desc[i].mask & mesh_mask[m] & instance_mask != 0 for g's mesh m; and dist2 <= r2 = fl(radius * radius),
 * dist2 from the unchanged cascade on the world record built from M = desc[i].transform with dot_c, no fused multiply-add.  A NaN
 * dist2 is never a candidate.  Sorted by (dist2, i, g) ascending, the order cap_closest_instances' tie rule defines; a pair appears at
 * most once.
 * Pages: device_out[j * k + s] and device_instances[j * k + s], s < k, are point j's s-th pair: a full world-space CapClosest as
 * cap_closest_instances writes it, and the table index.  Slots after the last pair hold the miss record
 * (0, 0, 0, r2, 0, 0, 0xFFFFFFFF, 0) and instance 0xFFFFFFFF.  With k = 1, no counts and no cursor, record and instance are bit for
 * bit cap_closest_instances' (the call runs its kernel).  Records are bit-identical to a float32 brute force, whichever builder made
 * the trees.
 * device_counts: NULL, or n uint32: the number of ALL candidate pairs of point j, not capped at k (with CAP_MULTI_CONTINUE: of the
 * pairs above the cursor).  Asking for counts turns off pruning by the k-th distance: the walk is then bounded by the radius alone.
 * k = 0 counts only: device_out and device_instances must be NULL and device_counts given.
 * Paging (CAP_MULTI_CONTINUE): on entry, slot k - 1 of each point's record page and of its instance page is read as the cursor
 * (dist2_c, i_c, g_c) -- words 3 and 6 of the record, and the instance; only pairs with (dist2, i, g) > (dist2_c, i_c, g_c) in
 * lexicographic order count, and the next pages are written over both arrays.  A short page ends in the miss record, whose cursor
 * (r2, 0xFFFFFFFF, 0xFFFFFFFF) admits nothing.  Calling again with the same points and buffers walks every pair exactly once,
 * equal-dist2 pairs of coinciding instances on either side of a page boundary and pairs with dist2 == r2 included.  Both cursor slots
 * must hold what the previous call wrote there; device_instances is therefore required whenever k > 0, as in
 * cap_trace_instances_multi.
 * Degenerate points (a non-finite coordinate, a NaN or negative radius) are not traversed: k miss records with dist2 = 0, instance
 * 0xFFFFFFFF and count 0, with CAP_MULTI_CONTINUE too.
 * Everything else is as for cap_closest_instances and cap_trace_instances_multi: device pointers on the context's GPU; points and
 * output 16-byte, instances and counts 4-byte aligned; no overlap between any two of the four ranges; asynchronous on the context
 * stream, ordered behind a render's second lane; n above 2^24 split into launches with all three output pointers advanced per chunk,
 * n = 0 does nothing; nothing of the render's state is touched.  Errors: CAP_ERR_STATE without an instance table, before
 * cap_bvh_build and while the trees are stale; CAP_ERR_INVALID_ARG for any ray_flags bit, non-zero reserved words, instance_mask >
 * 0xFF, unknown multi flags, k > CAP_MULTI_MAX_K, k = 0 with output or instances given or counts NULL, k > 0 with output or instances
 * NULL, CAP_MULTI_CONTINUE with k = 0, NULL points, misalignment, overlap, and n * k records beyond the address space.  Nothing is
 * written on an error.
 * Pruning never decides: the bound of cap_closest_instances with the k-th distance in the place of the best (DESIGN.md "Multi
 * closest-point queries over instances").
 * Not covered: a lower bound from the cursor (later pages walk the exhausted subtrees and instances again), per-point masks, the sign
 * of the distance, the wide view. */
int cap_closest_instances_multi(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, uint32_t k, CapClosest* device_out,
                                uint32_t* device_instances, uint32_t* device_counts, uint32_t multi_flags,
                                const CapTraceOptions* options /* may be NULL */);

/* ---- signed distance: the pseudonormal table and cap_signed_distance ----
 * cap_closest_points with a sign: negative inside a closed mesh.  The sign is that of dot(delta, N), N the angle-weighted pseudonormal
 * (Baerentzen & Aanaes 2005) of the FEATURE the record reports -- the face, edge or vertex the closest point lies on -- not the face
 * normal of the returned triangle: in an edge or vertex region the (dist2, lowest id) tie rule may return a face the point lies behind
 * (DESIGN.md "Signed distance" has counts).  The library builds the table because only it holds the mesh's connectivity across
 * duplicated vertices on the device, and keeps it current under cap_bvh_refit.
 *
 * The table (cap_pseudonormals_build) is made from the scene's ORIGINAL vertices, not the stored (v0, e1, e2) records, in binary64:
 *   weld      two vertices are one iff their three binary32 coordinates are equal after mapping -0 to +0, across the whole scene and
 *             all its meshes (OBJ material splits and triangle soups duplicate vertices); a non-finite coordinate welds to nothing;
 *   degenerate  a triangle with a non-finite corner, two corners of one weld id, or (v1 - v0) x (v2 - v0) == 0 in binary64 takes part
 *             in nothing -- no half-edge, no sum, no statistic but its own counter -- and its seven entries are +0;
 *   face      Nf = normalize((v1 - v0) x (v2 - v0)), on the side of the n = e1 x e2 the ray queries decide facing from: a front-facing
 *             hit comes from the positive side;
 *   edge      between weld ids (a, b), undirected: the sum of Nf over the live triangles on it;
 *   vertex    the sum of angle x Nf over the live corners at it, angle = atan2(|a x b|, a . b) of the two edges leaving the corner.
 * The sums are not normalised (only the sign is used); they run in ascending (triangle, corner) order and each component is rounded
 * ONCE to binary32 on store, so the same triangle list gives the same bits however its vertices are indexed or split over meshes.
 * cap_pseudonormals_readback copies the table out: 7 x 3 floats per triangle by global id, the entries indexed by CAP_FEATURE_*
 * (FACE, EDGE_V0V1, EDGE_V1V2, EDGE_V2V0, V0, V1, V2).  CapPseudonormalsInfo counts what the weld found; the sign means inside /
 * outside only for a mesh with closed == 1 (every edge on exactly two triangles that traverse it in opposite directions).  The table
 * and the query are defined for any mesh.
 *
 * cap_pseudonormals_build needs a built tree that is not stale (CAP_ERR_STATE); 3 x triangles >= 2^32 is CAP_ERR_UNSUPPORTED.  It
 * waits for the device once (the statistics).  out may be NULL.  cap_pseudonormals_drop frees the table (CAP_OK without one).
 * cap_pseudonormals_readback is CAP_ERR_STATE without a table or while the trees are stale.
 * Life cycle: cap_scene_upload drops the table; cap_scene_update_vertices makes it stale together with the trees; cap_bvh_build and
 * cap_bvh_refit rebuild it by the same routine when one exists -- the weld included, because moved vertices may weld differently;
 * cap_scene_set_instance_masks, objects and instances do not touch it.  It always covers every triangle, whatever the masks.
 * Memory: 84 B per triangle for the table, plus about 150 B per triangle of build scratch that is freed when the build returns.
 *
 * cap_signed_distance.  device_out[i] is bit for bit cap_closest_points' record: candidates, tie rule, masks, miss record and
 * degenerate points are unchanged.  For a record (g, feature): d = dot(delta, N[g][feature]), delta the record's own
 * fl(ap - fl(fl(e1*u) + fl(e2*v))) of the per-triangle function above, N the stored binary32 entry, dot the queries' unfused
 * (a.x*b.x + a.y*b.y) + a.z*b.z; device_signed[i] = -sqrt(dist2) if d < 0, else +sqrt(dist2), sqrt the correctly rounded binary32
 * square root.  d == 0 takes the positive sign (dist2 == 0 gives +0.0).  A miss or a degenerate point gives +inf.  So a float32
 * computation on the read-back table and the record's (u, v) is bit-identical.
 * Conventions are cap_closest_points' plus: device_signed is required and 4-byte aligned, no two of the three ranges overlap, and
 * CAP_ERR_STATE also without a table.  Nothing is written on an error; n above 2^24 is split into launches.
 * Not covered: the k-nearest forms.  The sign over instances: cap_signed_distance_instances below.  A sign for meshes that are not
 * closed: cap_winding_numbers further below. */
typedef struct CapPseudonormalsInfo
{
    uint32_t vertices;             /* welded positions of the live triangles */
    uint32_t edges;                /* undirected edges between them */
    uint32_t boundary_edges;       /* ... with one triangle */
    uint32_t nonmanifold_edges;    /* ... with more than two */
    uint32_t inconsistent_edges;   /* ... with exactly two that traverse it in the same direction */
    uint32_t degenerate_triangles;
    uint32_t closed;               /* 1 iff the three edge defect counts are 0 and at least one triangle is live */
    uint32_t reserved;
    double   ms;                   /* wall time of the build */
} CapPseudonormalsInfo;
int cap_pseudonormals_build(CapContext* ctx, CapPseudonormalsInfo* out /* may be NULL */);
int cap_pseudonormals_drop(CapContext* ctx);
int cap_pseudonormals_readback(CapContext* ctx, float* host_normals /* 21 floats per triangle */);
int cap_signed_distance(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out, float* device_signed,
                        const CapTraceOptions* options /* may be NULL */);

/* ---- signed distance over instances: cap_closest_instances with a sign, taken in object space ----
 * "How deep inside which part": penetration depth and contact generation against rigidly moving parts, distance fields over scenes
 * built from instances and animated by one cap_instances_set per frame.  The DISTANCE is the world one; the SIGN is read in the
 * instance's object space, where the pseudonormal table lives.  For a closed mesh, inside and outside are invariant under any
 * invertible affine map, a mirror included: a world point lies inside instance i exactly when its object-space image lies inside i's
 * object.  So no table per instance, no transformed normals and no rule for which transforms are "rigid enough" are needed.
 *
 * Records.  device_out[j] and device_instances[j] (may be NULL) are bit for bit cap_closest_instances' answer: candidates, tie rule
 * (dist2, i, g), masks, objects, miss record and degenerate points are all unchanged.
 * Object-space point.  For a point p whose record is a hit in instance i, with W the stored world-to-object matrix as
 * cap_instances_readback returns it, per row r:
 *   p'_r = fl(fl(fl(fl(W_r0*p.x) + fl(W_r1*p.y)) + fl(W_r2*p.z)) + W_r3)
 * every operation one rounded binary32 operation in the order written, no fused multiply-add.
 * Sign record.  cap_signed_distance's winner for the point (p', radius = +inf) over instance i's candidates alone: the triangles of i's
 * object (the whole scene without an object table) with desc[i].mask & mesh_mask[m] & instance_mask != 0 for the triangle's mesh m.
 * The per-triangle function is cap_closest_points' cascade, unchanged, on the stored object-space record (v0, e1, e2); the sign record
 * is the candidate minimal in (dist2', g'); a NaN dist2' is never a candidate.  d = dot_c(delta', N[g'][feature']): delta' that
 * record's own delta, N the stored binary32 table entry, dot_c the point queries' unfused dot.  The point's own radius does not bound
 * this walk, and the world winner's triangle is always among its candidates.  (g', feature') need not be the world record's (g,
 * feature): a transform that is not a similarity does not preserve nearest.
 * Signed value.  device_signed[j] = -sqrt(dist2) if d < 0 and dist2 != 0, else +sqrt(dist2): dist2 the WORLD record's, sqrt the
 * correctly rounded binary32 square root.  dist2 == 0 gives +0.0 whatever the object-space walk says.  A miss or a degenerate point
 * gives +inf.  If p' is degenerate by the points' own rule (a coordinate overflowed or is NaN), or no candidate has a dist2' that is
 * not NaN, the sign is positive.  A float32 computation from the read-back W, the read-back table and the scene's triangles is
 * therefore bit-identical.
 * What the sign means: inside or outside only where the instance's VISIBLE triangles -- its object's, under the masks -- form a
 * closed, consistently wound surface.  The table welds across the whole scene: objects that touch in object space share edges there
 * and stop being closed, each for itself, so keep the objects of one scene apart (CapPseudonormalsInfo.closed reports the scene).  A
 * mirrored instance of an outward-wound object is negative inside as well: facing, as everywhere in this ABI, is an object-space
 * notion.
 * Identity (tested): with one identity instance and no negative zero in the scene, records and signed values are bit-identical to
 * cap_signed_distance's, for every radius.
 * Conventions are cap_closest_instances' plus: device_signed is required and 4-byte aligned; no two of the four ranges (points,
 * output, signed, and instances unless NULL) overlap.  CAP_ERR_STATE without an instance table, without a pseudonormal table, before
 * cap_bvh_build and while the trees are stale.  CAP_ERR_INVALID_ARG exactly where cap_closest_instances has it, and for a NULL
 * device_signed.  Nothing is written on an error.  n above 2^24 is split into launches with all three output pointers advanced; n = 0
 * does nothing.  Asynchronous on the context stream; nothing of the render's state is touched.
 * Pruning never decides: the world walk is cap_closest_instances', the object-space walk cap_closest_points' with the scene's slack
 * (DESIGN.md "Signed distance over instances").
 * Not covered: the sign of the k-nearest forms. */
int cap_signed_distance_instances(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out,
                                  uint32_t* device_instances /* may be NULL */, float* device_signed,
                                  const CapTraceOptions* options /* may be NULL */);

/* ---- winding numbers: the dipole table and cap_winding_numbers ----
 * The generalised winding number (Jacobson et al. 2013) w(q) = (1 / 4 pi) sum_t Omega_t(q), Omega_t the signed solid angle triangle t
 * subtends at q: 1 inside and 0 outside a closed mesh wound outwards (the side the ray queries call front), 5/6 at the centre of a
 * cube with one face removed, and degrading smoothly with holes, duplicated triangles and self-intersections.  w >= 1/2 is the usual
 * robust inside test for voxelisation, point classification and distance-field baking where cap_signed_distance's sign does not apply
 * (CapPseudonormalsInfo.closed == 0).  The exact sum costs O(T) per point; the walk answers in O(log T) by replacing far subtrees with
 * their first-order dipole (Barill et al. 2018).
 *
 * The table (cap_winding_build) hangs a dipole on every child of the scene's binary tree: one 64-byte record per inner node, indexed as
 * cap_bvh_readback's nodes, 8 floats per child slot (slot 0, then slot 1):
 *   words 0..2  p~, the area-weighted centroid of the child's subtree
 *   word  3     r, the radius of a ball about the stored p~ that covers the child's stored box
 *   words 4..6  N = sum of 1/2 (v1 - v0) x (v2 - v0) over the subtree
 *   word  7     the child's code exactly as the tree holds it for traversal (words 14 and 15 of the node): a node index, or the leaf
 *               code ~(first | (count - 1) << 27) of a range of the leaf order
 * so the query reads one record per node step and never the box nodes.  A child's subtree is what lies below that code: the range of
 * a leaf code, both slots of a node index.  From the scene's ORIGINAL vertices, in binary64:
 *   triangle    n_t = 1/2 (v1 - v0) x (v2 - v0), a_t = |n_t| = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z), c_t = ((v0 + v1) + v2) / 3;
 *   degenerate  a triangle with a non-finite corner or n_t == 0 contributes nothing and is counted in CapWindingInfo;
 *   sums        N = sum n_t, A = sum a_t, M = sum a_t c_t; a leaf code sums its triangles in leaf order starting from 0, a node index
 *               adds slot 0 + slot 1 -- one fixed order, so the same tree and vertices give the same bytes on every run;
 *   p~          M / A, or the centre 1/2 (lo + hi) of the child's stored box when A == 0; p~ and N are rounded once to binary32;
 *   r           the distance from the STORED p~ to the farthest corner of the child's stored (padded) box,
 *               sqrt((dx*dx + dy*dy) + dz*dz) with d_k = max(|lo_k - p~_k|, |hi_k - p~_k|), rounded to binary32 and stepped one ulp up.
 * Every inner node has a record, also the nodes below a leaf code, which no walk reaches.  A tree whose root is a leaf (one triangle)
 * has no records.  cap_winding_readback copies the table out, 16 floats per inner node.  CapWindingInfo: the inner nodes, the
 * degenerate triangles, the total area A, N and p~ of the whole tree (p~ the centre of the scene bounds when A == 0), the wall time.
 *
 * Life cycle, cap_pseudonormals_*'s rule for rule: cap_winding_build needs a built tree that is not stale (CAP_ERR_STATE) and waits for
 * the device once; out may be NULL.  cap_winding_drop frees the table (CAP_OK without one).  cap_winding_readback is CAP_ERR_STATE
 * without a table or while the trees are stale.  cap_scene_upload drops the table; cap_scene_update_vertices makes it stale together
 * with the trees; cap_bvh_build and cap_bvh_refit rebuild it by the same routine when one exists; cap_scene_set_instance_masks, objects
 * and instances do not touch it.  It always covers every triangle, whatever the masks.  Memory: 64 B per inner node, plus about 180 B
 * per triangle of build scratch that is freed when the build returns.
 *
 * cap_winding_numbers.  One walk per point q = device_points[i].point (the radius is not read), depth-first from the root with a
 * binary64 accumulator.  At a node the two children are decided, all in binary32, every operation one rounded operation in the order
 * written, no fused multiply-add, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z:
 *   d = fl(p~ - q), d2 = dot(d, d), lim = fl(beta * r); the child is FAR iff d2 > fl(lim * lim).
 * A far child adds the term fl(dot(N, d) / fl(fl(k4 * d2) * sqrt(d2))), k4 = fl(4 pi) = 12.566371f, and counts in visits[0].  The far
 * terms of a node are added first, slot 0 then slot 1; then the children that are not far are entered, slot 0's subtree before slot
 * 1's.  A leaf code adds the exact term of each of its triangles in leaf order and adds their number to visits[1].  The exact term is
 * Van Oosterom & Strackee's on the stored intersection record (v0, e1, e2, n = fl(e1 x e2)) of the ray queries:
 *   a = fl(v0 - q), b = fl(a + e1), c = fl(a + e2), la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), lc = sqrt(dot(c, c)),
 *   det = dot(a, n), den = (((la*lb)*lc + dot(a, b)*lc) + dot(b, c)*la) + dot(c, a)*lb,
 *   term = fl(atan2f(det, den) * k2), k2 = fl(1 / (2 pi)) = 0.15915494f.
 * A term that is NaN (a record with a non-finite word) adds nothing.  Each term is widened to binary64 and added; device_winding[i] is
 * the accumulator rounded once to binary32.  The far / near decisions -- and so device_visits -- are reproducible bit for bit by a
 * float32 restatement on the read-back tree and table; the value is reproducible run to run and depends on the device's atan2f, sqrt
 * and division only within their rounding.  A root that is a leaf is summed exactly.
 * beta must be finite and >= 1, or +inf (anything else, NaN included: CAP_ERR_INVALID_ARG).  Larger is more exact and slower; 2 keeps
 * the error near 0.05 on closed test meshes, ample for the 1/2 threshold and not a precision claim.  +inf makes every comparison
 * false: the exact sum over all triangles.  A point with a non-finite coordinate gets a quiet NaN and visits (0, 0).  An empty scene
 * gives 0.0.
 * Conventions are the point queries': device pointers on the context's GPU -- device_points 16-byte aligned, device_winding (4 B per
 * point) and device_visits (8 B per point; may be NULL) 4-byte aligned --, no two ranges overlap; nothing is written on an error; n
 * above 2^24 is split into launches, n = 0 does nothing; asynchronous on the context stream; nothing of the render's state is touched.
 * CAP_ERR_STATE without a table, before cap_bvh_build and while the trees are stale.  There is no CapTraceOptions: the moments cover
 * all triangles, so a mesh mask cannot be honoured.
 * Not covered: masks, second- and third-order moments, a per-point beta, a wave-cooperative walk.  Instances and objects:
 * cap_winding_instances below. */
typedef struct CapWindingInfo
{
    uint32_t inner_nodes;          /* records in the table: triangles - 1, or 0 */
    uint32_t degenerate_triangles;
    double   total_area;           /* A of the whole tree */
    float    root_n[3];            /* N of the whole tree: 0 for a closed mesh, up to rounding */
    float    root_p[3];            /* p~ of the whole tree */
    double   ms;                   /* wall time of the build */
} CapWindingInfo;
int cap_winding_build(CapContext* ctx, CapWindingInfo* out /* may be NULL */);
int cap_winding_drop(CapContext* ctx);
int cap_winding_readback(CapContext* ctx, float* host_table /* 16 floats per inner node */);
int cap_winding_numbers(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, float beta, float* device_winding,
                        uint32_t* device_visits /* may be NULL: 2 per point */);

/* ---- winding numbers over instances: world dipoles and cap_winding_instances ----
 * The generalised winding number of the scene the instance table describes, flattened into world space: with M_i = desc[i].transform,
 * L_i its linear part and s_i = sign(det L_i),
 *   w(q) = sum_i s_i / (4 pi) sum_{t in object(i)} Omega(M_i t, q),
 * Omega the signed solid angle of the WORLD-space triangle.  s_i makes a mirrored instance of an outward-wound closed mesh read 1
 * inside: facing, as everywhere in this ABI, is an object-space notion.  Solid angle is not affine-invariant, so this is not
 * w_object(W q) except for similarity transforms and closed meshes; it is the true winding number of the flattened scene, the robust
 * inside test for assemblies of parts that weld into each other, are open, or are placed many times.
 * An instance contributes iff it is not inert, desc.mask & 0xFF != 0 and det L_i is a finite number other than 0.  A mask of 0
 * switches an instance off, as for rays; nothing else of the masks is honoured and there is no CapTraceOptions, for cap_winding_numbers'
 * reason: the moments cover every triangle.
 *
 * Derived tables.  Three tables hang off the dipole table of cap_winding_build, the instance table and the object table; all are
 * built in binary64 and rounded once per word, in one fixed order, so the same state gives the same bytes:
 *   per instance   12 floats: L row-major (9), |det L|, sigma, s.  sigma = sqrt(||L||_1 ||L||_inf) rounded UP to binary32, an upper
 *                  bound of ||L||_2 and exactly 1 for the identity.  s = +1 or -1, 0 for an instance that does not contribute.
 *   top level      8 floats per entry of the top-level tree, in the tree's own layout (level 0 = the instances in the tree's order,
 *                  padded to an even count; entry j of a level above = entries 2 j and 2 j + 1 of the level below): words 0..2 p~_w,
 *                  word 3 r, words 4..6 N_w, word 7 the instance index at level 0 and 0xFFFFFFFF above.  Level 0, from the root sums
 *                  (N, A, M) of the instance's object: N_w = s cof(L) N (the area vector transforms exactly under an affine map),
 *                  p~_w = M_i (M / A), weight A |det L|^(2/3) (exact for similarities; any positive weight keeps p~_w inside the
 *                  subtree).  A level above adds (N_w, weight, weight p~_w) of entry 2 j and entry 2 j + 1, in that order.  p~_w =
 *                  the weighted sum over the weight, or the centre of the entry's stored world box when the weight is 0; r follows
 *                  the scene table's rule on the entry's stored world box: the distance from the STORED p~_w to its farthest corner,
 *                  stepped one ulp up.  An entry without a contributing instance below it is EMPTY: r = -1 and zeros.
 *   forest         with an object table: the dipole table of every object's tree, 16 floats per forest node, by the rules of
 *                  cap_winding_build on the object's triangles; word 7 holds the child code in the forest's numbering.  Without an
 *                  object table the one object is the scene and its table is cap_winding_build's.  A one-triangle object has no
 *                  records.
 * They are derived state: cap_instances_set(_ex), cap_objects_set, cap_bvh_build, cap_bvh_refit and cap_winding_build only mark them
 * dirty, and the first cap_winding_instances or cap_winding_instances_readback that finds them dirty rebuilds them on the context
 * stream ahead of its own work, without a host wait (cap_instances_set alone leaves the forest's table as it is).  A context that never
 * calls either has none.  cap_winding_drop and cap_scene_upload free them.  The scene table's bytes are never touched.
 * Memory: 48 B per instance, 88 B per top-level entry, with an object table 64 B per forest node and 56 B per object, plus about 180 B
 * per triangle of the largest object of build scratch, which is kept until cap_winding_drop.
 * cap_winding_instances_readback copies them out (each pointer may be NULL): host_top 8 floats per top-level entry, host_inst 12
 * floats per instance, host_forest 16 floats per forest node.  cap_winding_instances_info never builds anything: `built` says whether
 * current tables exist, and only then are contributing, forest_records and the root words filled.
 *
 * cap_winding_instances.  One walk per point q, a binary64 accumulator, all decisions in binary32, every operation one rounded
 * operation in the order written, no fused multiply-add, dot as cap_winding_numbers'.
 * Top level: the implicit tree from its root.  At a node the two entries are decided, slot 0 then slot 1: an empty entry is skipped;
 * otherwise cap_winding_numbers' far rule and far term on the world dipole (p~_w, r, N_w) and q, unchanged, counted in visits[0].
 * The far terms of a node are added first; then the entries that are neither empty nor far are entered, slot 0's subtree first.  An
 * entry of level 0 that is entered is an instance i, counted in visits[1]:
 *   p'_r = fl(fl(fl(fl(W_r0*q.x) + fl(W_r1*q.y)) + fl(W_r2*q.z)) + W_r3), W the stored world-to-object matrix (cap_instances_readback);
 *   if p' is degenerate by the points' own rule (a coordinate that is not finite) the instance adds nothing and is not counted.
 * Then cap_winding_numbers' walk of the object's tree from the object's root over the object's table, with, for an object-space
 * difference d', d_w = (dot(L_0, d'), dot(L_1, d'), dot(L_2, d')), L_r the rows of the stored L:
 *   far rule    d' = fl(p~ - p'), d2 = dot(d_w, d_w), lim = fl(beta * fl(sigma * r)); FAR iff d2 > fl(lim * lim);
 *   far term    fl(fl(|det L| * dot(N, d')) / fl(fl(k4 * d2) * sqrt(d2))), counted in visits[2] (the world area vector is cof(L) N,
 *               and the cofactor cancels against L d');
 *   exact term  a' = fl(v0 - p'), b' = fl(a' + e1), c' = fl(a' + e2); a, b, c their images under d_w; la, lb, lc, den from a, b, c as
 *               in cap_winding_numbers; det = fl(|det L| * dot(a', n)), which is s det_w; term = fl(atan2f(det, den) * k2); a leaf
 *               adds its number of triangles to visits[3].
 * A NaN term adds nothing.  device_winding[j] is the accumulator rounded once.  A point with a non-finite coordinate gets a quiet NaN
 * and visits (0, 0, 0, 0); a table without a contributing instance, or an empty scene, gives 0.0.  The decisions -- and so
 * device_visits -- are reproducible bit for bit by a float32 restatement on the read-backs.
 * Identity (tested): with one identity instance of a scene without negative zero, beta = +inf gives cap_winding_numbers' bits; at a
 * finite beta so does every point whose visits[0] is 0, and visits[2], visits[3] are then cap_winding_numbers' pair.
 * beta: finite and >= 1, or +inf (the exact sum); anything else is CAP_ERR_INVALID_ARG.  The error at beta = 2 is of the size of
 * cap_winding_numbers' (DESIGN.md "Winding numbers over instances").
 * Conventions are cap_winding_numbers': device_points 16-byte aligned, device_winding (4 B per point) and device_visits (16 B per
 * point; may be NULL) 4-byte aligned, no two ranges overlap, nothing is written on an error, n above 2^24 is split into launches, n = 0
 * does nothing, asynchronous on the context stream.  CAP_ERR_STATE without an instance table, without a winding table, before
 * cap_bvh_build and while the trees are stale.
 * Not covered: mesh masks and a per-call inclusion mask, higher moments, a per-point beta. */
typedef struct CapWindingInstancesInfo /* 160 B */
{
    uint32_t instances;         /* of the installed table */
    uint32_t contributing;
    uint32_t levels;            /* of the top-level tree */
    uint32_t entries;           /* of all levels, padding included: host_top holds 8 floats for each */
    uint32_t forest_records;    /* 0 without an object table */
    uint32_t built;             /* 1: derived tables exist and are current */
    uint32_t level_entries[25]; /* entries per level, padding included: level l starts at the sum of the levels below */
    uint32_t reserved;
    double   total_weight;      /* of the whole table */
    float    root_n[3];         /* N_w of the whole table */
    float    root_p[3];         /* p~_w of the whole table */
} CapWindingInstancesInfo;
int cap_winding_instances(CapContext* ctx, const CapPointDesc* device_points, uint64_t n, float beta, float* device_winding,
                          uint32_t* device_visits /* may be NULL: 4 per point */);
int cap_winding_instances_info(CapContext* ctx, CapWindingInstancesInfo* out);
int cap_winding_instances_readback(CapContext* ctx, float* host_top /* 8 floats per top-level entry */,
                                   float* host_inst /* 12 floats per instance */,
                                   float* host_forest /* 16 floats per forest node; each may be NULL */);

/* ---- objects: per-mesh-range bottom-level trees for the instanced queries ----
 * An object is the mesh range [first_mesh, first_mesh + mesh_count) of the uploaded scene: mesh_count >= 1, at least one triangle,
 * inside the mesh table.  Ranges are pairwise disjoint, in any order, and need not cover the scene; anything else, or count >
 * CAP_OBJECT_MAX_COUNT, is CAP_ERR_INVALID_ARG with nothing changed.  Needs a built tree that is not stale (CAP_ERR_STATE), as
 * cap_instances_set.  count = 0 removes the table: instances are instances of the whole scene again.
 * cap_objects_set builds one binary tree per object from the current vertices, each with the builder cap_bvh_build would take for a
 * scene of the object's triangle count under the context's cap_set_bvh_build mode (the AUTO thresholds included); the host builder
 * CAP_BVH_BUILD_SAH is mapped to CAP_BVH_BUILD_SAH_DEVICE.  CapObjectInfo::builder says which one built an object.  A one-triangle
 * object has no node.  An object tree deeper than 64 is CAP_ERR_UNSUPPORTED (the scene tree's rule), as is a forest position that does
 * not fit the traversal-leaf code; the table is then dropped.
 * Life cycle.  cap_scene_upload drops the object table and the instance table.  cap_objects_set -- a new table or count = 0 -- drops
 * the INSTANCE table, because object indices change meaning: call cap_instances_set(_ex) again.  cap_bvh_build and cap_bvh_refit
 * rebuild every object's tree from the current vertices by the same routine (not an in-place refit: the cost is one build per object)
 * and then the instances' world boxes and TLAS.  The call waits for the device once, to read the trees' depths and bounds.
 * Memory: the forest holds 64 B per covered triangle (intersection records) and 64 B per node (triangles - 1 per object) beside the
 * scene's own trees, plus build scratch of about 100 B per triangle of the largest object.
 * cap_render, the plain queries and the flat multi-hit queries (cap_trace_rays_multi*) do not read the table. */
#define CAP_OBJECT_MAX_COUNT 4096u
typedef struct CapObjectRange
{
    uint32_t first_mesh, mesh_count;
} CapObjectRange;
typedef struct CapObjectInfo /* 48 B */
{
    uint32_t first_triangle, triangle_count, node_count, max_depth;
    float    bounds_lo[3], bounds_hi[3]; /* exact min / max of the object's vertices, as CapBvhInfo's */
    uint32_t builder;                    /* the CAP_BVH_BUILD_* that built it (never AUTO or SAH) */
    uint32_t reserved;
} CapObjectInfo;
typedef struct CapObjectsInfo
{
    uint32_t count, triangles, nodes, max_depth; /* objects, covered triangles, forest nodes, largest depth */
    double   ms;                                 /* host time of the call, the wait for the device included */
} CapObjectsInfo;
int cap_objects_set(CapContext* ctx, const CapObjectRange* ranges /* host */, uint32_t count, CapObjectsInfo* out /* may be NULL */);
/* the first min(capacity, count) entries into `out` (host; may be NULL when capacity is 0), the table's count into *count_out (may be
 * NULL); 0 objects without a table */
int cap_objects_info(CapContext* ctx, CapObjectInfo* out, uint32_t capacity, uint32_t* count_out);
/* the forest as cap_bvh_readback gives the scene's tree: 16 floats per forest node (object k's nodes follow object k - 1's, child codes
 * in the forest's numbering) and the scene's triangle id of every forest record; each may be NULL.  CAP_ERR_STATE without a table. */
int cap_objects_readback(CapContext* ctx, float* host_nodes, uint32_t* host_leaf_triangles);

/* ---- multi-GPU tile exchange (one gather of tile radiance at frame end) ---- */
/* floats in this context's tile-ordered radiance buffer: max_tiles_per_shard * 64 * 4 (same on every shard) */
int cap_tile_buffer_floats(CapContext* ctx, size_t* out_floats);
/* writes ACCUM_MEAN of the local tiles, tile order, into a DEVICE buffer of cap_tile_buffer_floats floats */
int cap_resolve_tiles(CapContext* ctx, float* device_dst);
/* device_src: shard_count tile buffers back to back (the gather result); device_image: width*height*4 floats */
int cap_assemble_tiles(CapContext* ctx, const float* device_src, uint32_t shard_count, float* device_image);

/* ---- the exchange itself: ONE gather of tile radiance to rank 0 per frame, over RCCL (xGMI) ----
 * The reference is single-GPU (dx12.cpp:13-25, 196-234); this is the north star's "frames shard by screen tile across the GPUs of
 * one node with a single RCCL gather of tile radiance at frame end".  Each context renders the shard cap_set_shard gave it
 * (shard index == rank, shard count == ranks).  RCCL is loaded on first use (dlopen "librccl.so.1", or CAP_RCCL_LIBRARY); a copy
 * the process already has loaded is shared.  cap_comm_gather_frame* resolve the tiles (as cap_resolve_tiles), gather them to rank
 * 0 with ncclGather on the contexts' streams and assemble the row-major image there (as cap_assemble_tiles): asynchronous,
 * ordered behind the render on each stream. */
#define CAP_COMM_ID_BYTES 128
/* one process per GPU: rank 0 makes the id, the host program carries it to the other ranks (file, MPI, a key-value store) */
int cap_comm_unique_id(uint8_t* id_128_bytes);
int cap_comm_init_rank(CapContext* ctx, const uint8_t* id_128_bytes, uint32_t rank, uint32_t nranks); /* collective */
int cap_comm_gather_frame(CapContext* ctx);                                                            /* collective */
/* one process driving n GPUs: ctxs[i] renders shard i of n; contexts on pairwise distinct devices get an RCCL communicator
 * (ncclCommInitAll), contexts that all share one device exchange by device copies */
int cap_comm_init_all(CapContext* const* ctxs, uint32_t n);
int cap_comm_gather_frame_all(CapContext* const* ctxs, uint32_t n);
/* rank 0 after a gather: the assembled frame, width*height*4 floats (mean radiance; .w = frames), on the device / on the host */
int cap_comm_image(CapContext* ctx, float** device_image);
int cap_comm_readback(CapContext* ctx, float* dst);
int cap_comm_info(CapContext* ctx, uint32_t* rank, uint32_t* size, uint32_t* uses_rccl);
int cap_comm_destroy(CapContext* ctx); /* also done by cap_ctx_destroy */
/* Error path: gives the communicator up WITHOUT waiting for the stream (ncclCommAbort) -- for a rank whose peers failed before
 * entering a collective this rank has already queued, where cap_comm_destroy's stream synchronisation would never return.  The
 * communicator's asynchronous error state is polled once per frame by cap_comm_gather_frame* (ncclCommGetAsyncError). */
int cap_comm_abort(CapContext* ctx);

/* ---- reconstruction chain ----
 * The passes RaytracingSystem::Run records after the ray passes (raytracing_system.cpp:294-317):
 * SpatialGather (cpp:1541-1604) -> IntegrateTemporally (cpp:1283-1342) -> Denoise = BlurDisocclusion + 2|4 a-trous blurs
 * (cpp:1437-1538) -> CombineIllumination (cpp:1400-1435) -> ApplyTAA (cpp:1344-1398), full-resolution configuration.
 * Settings = the SettingsComponent fields those passes read (gui_system.h:20-37, defaults in comments). */
typedef struct CapPostSettings
{
    int32_t gather;                    /* true  */
    int32_t denoise;                   /* true  */
    int32_t eaw5;                      /* true  */
    float   eaw_normal_sigma;          /* 128   */
    float   eaw_depth_sigma;           /* 3     */
    float   eaw_luma_sigma;            /* 3     */
    float   gather_normal_sigma;       /* 64    */
    float   gather_depth_sigma;        /* 2     */
    float   gather_luma_sigma;         /* 3     */
    float   temporal_upscale_feedback; /* 0.975 */
    float   taa_feedback;              /* 0.9   */
    int32_t lowres_indirect;           /* false: RaytracingOptions::lowres_indirect, UPSCALE2X in Gather and Accumulate
                                          (spatial_gather.hlsl:36-46, temporal_accumulation.hlsl:228-235, 307-313) */
    /* Every field from here on reads 0 as the reference's default, so that a caller who fills the struct positionally up to
     * lowres_indirect (the round-1 form) -- or memsets it and sets what it knows -- runs the reference's default configuration. */
    int32_t disable_variance;          /* false: NOT RaytracingOptions::use_variance (raytracing_system.h:25, default true): the
                                          USE_VARIANCE define of eaw_blur.hlsl:68,114,127,162 (raytracing_system.cpp:669-673).  Set:
                                          no luma edge-stopping and no a-trous kernel weights in Blur, variance channel 0 */
    int32_t fast_weights;              /* false.  Not a reference option: evaluates the edge-stopping weights with the hardware's
                                          v_exp_f32 / v_log_f32 / v_rcp_f32 instead of the arithmetic contract's polynomials and IEEE
                                          divisions, and (round 5) the VALUES of IntegrateTemporally and TAA with the same instructions
                                          and the centre tap of their bicubic resamples -- what those two passes DECIDE (reprojection,
                                          disocclusion test, static / moving) stays the exact arithmetic on the same G-buffer, so both
                                          modes reset and blend at the same pixels.  The exact mode (0) is bit-identical to the oracle; this one is held to a stated
                                          tolerance against it over a multi-frame sequence (tests/test_post_gpu.py), per colour channel
                                          with e = |fast - exact| / (|exact| + 1e-3): median e <= 2e-5, 99 % of the channels
                                          e <= 4e-3, every channel e <= 3e-2 (TAA's variance clipping amplifies in flat regions).
                                          That distribution holds for RENDERED frames.  On arbitrary planes no fixed number can hold
                                          (a 2^-16 relative change of the colour inputs moves the exact chain by more than that
                                          median); there the mode is held, frame by frame, to four times the exact chain's own response
                                          to such a change: median, 99th percentile and maximum of e each at most 4 x those of the
                                          exact chain on perturbed colours (tests/test_post_planes_fast_gpu.py; DESIGN.md has the
                                          measured ratios).  TAA's neighbourhood box counts among what decides and is the exact code */
    int32_t output;                    /* 0: SettingsComponent::output (gui_system.h:11-17, 38), passed to CombineIllumination as
                                          `type` (raytracing_system.cpp:1415; combine_illumination.hlsl:26-40): CAP_OUTPUT_COMBINED
                                          indirect * albedo + direct, CAP_OUTPUT_DIRECT, CAP_OUTPUT_INDIRECT (the denoised indirect
                                          term, w = 1), CAP_OUTPUT_VARIANCE (its variance channel: indirect.www after the last blur) */
} CapPostSettings;
enum
{
    CAP_OUTPUT_COMBINED = 0, /* kCombined */
    CAP_OUTPUT_DIRECT   = 1, /* kDirect   */
    CAP_OUTPUT_INDIRECT = 2, /* kIndirect */
    CAP_OUTPUT_VARIANCE = 3  /* kVariance */
};
/* The reference's default configuration (gui_system.h:20-40, raytracing_system.h:22-27): gather, denoise, eaw5 on; sigmas 128 / 3 / 3
 * and 64 / 2 / 3; feedbacks 0.975 / 0.9; every later field 0. */
void cap_post_settings_default(CapPostSettings* out);
/* Runs the chain on the planes of the last frame rendered with CAP_RENDER_AOV (frame_count = that frame's index; the
 * camera is the one set for it; prev_camera = the previous frame's, CameraComponent/prev_camera of
 * temporal_accumulation.hlsl:10-11) and keeps the histories for the next call.  Needs an unsharded context: the stencils read
 * across tile borders.  Asynchronous on the context stream.  The result (current_frame_output(), cpp:320-324) is read with
 * cap_post_readback. */
int cap_post_frame(CapContext* ctx, const CapPostSettings* settings, uint32_t frame_count, const CapCameraData* prev_camera);
/* Sharded contexts: the chain runs on ONE rank on the gathered ray-pass outputs (the note on the post-process chain in the
 * multi-GPU design: 5x5 .. 7x7 neighbourhoods with strides up to 14 px cross every tile border).  Per frame:
 *   every rank   cap_render(.., CAP_RENDER_AOV); cap_resolve_aov_tiles(ctx, buf)            buf: cap_aov_tile_buffer_floats floats
 *   one gather of the rank buffers to the root (rank-major, like cap_resolve_tiles / cap_assemble_tiles)
 *   root         cap_post_frame_gathered(ctx, settings, frame_count, prev_camera, gathered, shard_count)
 * The buffer holds the four planes the chain reads (indirect, direct, albedo, normal/depth of the AOV frame), plane-major, each
 * in tile order.  The root's context must have the same resolution, camera and shard_count; its own render outputs are not
 * used (with settings.lowres_indirect every rank renders with CAP_RENDER_LOWRES_INDIRECT and frame_count selects the 2x2
 * interleave offset, as in cap_post_frame). */
int cap_aov_tile_buffer_floats(CapContext* ctx, size_t* out_floats);
int cap_resolve_aov_tiles(CapContext* ctx, float* device_dst);
int cap_post_frame_gathered(CapContext* ctx, const CapPostSettings* settings, uint32_t frame_count, const CapCameraData* prev_camera,
                            const float* device_gathered, uint32_t shard_count);
/* CAP_RENDER_GBUFFER_FEEDBACK on sharded contexts: the next frame's indirect pass reads the chain's output and the normal/depth
 * image of this frame (rt_indirect.hlsl:116-145), which only the root has.  After the chain of frame f the root exports the two
 * images (cap_feedback_buffer_floats floats: width*height*4 each, output first), ONE broadcast carries them to the other ranks,
 * and those import them before cap_render(f + 1, .., CAP_RENDER_GBUFFER_FEEDBACK).  Frame 0 needs nothing (cleared histories
 * everywhere).
 * Layout of the buffer (a contract between builds: ranks exchange it): plane 0 = the chain's output of frame f,
 * current_frame_output() (RGBA as cap_post_readback returns it); plane 1 = frame f's normal/depth image as the CHAIN keeps it for
 * the next frame -- the DECODED unit normal in .xyz (OctDecode of gbuffer_normal_depth.xy) and the raw depth in .w -- not the
 * oct-encoded G-buffer plane of CAP_BUF_NORMAL_DEPTH (that was its content until round 3).  The indirect pass's feedback branch and
 * Accumulate read only .w; both planes are written and read by cap_feedback_export / _import only, as a pair
 * (tests/test_post_gpu.py::test_gbuffer_feedback_on_shards round-trips them across every frame of a sequence). */
int cap_feedback_buffer_floats(CapContext* ctx, size_t* out_floats);
int cap_feedback_export(CapContext* ctx, float* device_dst);
int cap_feedback_import(CapContext* ctx, const float* device_src, uint32_t frame_count);
/* zero-fills the histories (a new sequence; also implied by cap_set_resolution) */
int cap_post_reset(CapContext* ctx);
/* dst: width*height*4 floats (host) */
int cap_post_readback(CapContext* ctx, float* dst);

#ifdef __cplusplus
}
#endif
#endif /* CAPSAICIN_HIP_H */
