// cap_kernels.h — host-callable launchers of the gfx950 kernels, one section per translation unit.
#pragma once

#include "cap_device.h"

#include <cstdio>
#include <vector>

namespace cap
{
// A/B and diagnostic switches: ONE table per context (round 6; 26 getenv() calls with function-local statics before), filled from the
// environment once at cap_ctx_create and settable per context with cap_debug_set(ctx, CAP_DEBUG_SWITCH_BASE + index, value), so that a
// test or a tool flips a path without a child process.  -1 = not set: the product's own choice.  The names are the environment
// variables' (kSwitchNames, context.hip); the launchers read the table through LaunchCfg.
enum CapSwitch : uint32_t
{
    SW_NO_WIDE8 = 0,      // binary-tree kernels instead of the compressed 8-wide view
    SW_LANE1_PRIORITY,    // stream priority of the second lane
    SW_PLOC_RADIUS,       // clustering search window
    SW_SAHDEV_LEAF,       // sah_device: segments of at most this many triangles go to the clustering
    SW_WIDE_HOST_COLLAPSE,
    SW_TRACE_LAUNCHES,    // name every launch on stderr and drain the stream after it
    SW_NO_TWO_LANES,
    SW_LANE_SPLIT_MIN,
    SW_BLOCKS_PER_CU,
    SW_NO_CAMERA_CULL,
    SW_NO_ALBEDO_IN_W,
    SW_NO_INLINE_NEE,
    SW_NO_INLINE_PROBE,
    SW_NO_WAVE_RING,
    SW_ANY_REFILL,        // 0 never, 1 always: the lane-refill any-hit kernel
    SW_PRIMARY_WIDE,      // 0 never, 1 whenever allowed: camera rays through k_trace_closest8
    SW_NO_PACKET,
    SW_NO_ANY_PROBE,
    SW_ANY_PROBE,
    SW_ANY_BLOCKS,
    SW_NO_PRIMARY_FUSE,
    SW_W8_REFILL,
    SW_W8_GRID,
    SW_AUTO_SAH_TRIANGLES,  // AUTO builds with surface-area splits from this many triangles on
    SW_NO_NEE_PAIR_CULL,    // EXT model: next-event rays test every fan pair (read by the next cap_bvh_build / cap_materials_upload)
    SW_RAYGEN_KERNEL,       // dense scenes: the camera rays' identity queue written out by k_raygen_identity instead of generated in the trace kernel
    SW_NO_PLANE_CODE,       // small-scene path under albedo_in_w: bounce 0 writes the constant direct plane as before (ShadeArgs::code_in_color off)
    SW_SAMPLE_TABLE,        // small-scene path, reference model: 0 never, 1 whenever the kernels have the form: direction-sample terms from the batch's table (ShadeArgs::sample_terms)
    SW_NO_CAMERA_TABLE,     // small-scene path, reference model: bounce 0 stays a launch of its own (no camera-vertex table, no bounce-0 head in bounce 1's launch)
    SW_NO_GRAY_ENTRIES,     // small-scene path, sample-table kernels, untextured scene: the extension queue keeps its 48-byte entries (three throughput words)
    SW_NO_GROUP_WALK,       // head kernels: bounce 0's chunk indices walk the identity queue slot-major (no bands of jitter groups, cap_device.h head_chunk)
    SW_NO_TABLE_REUSE,      // every batch rebuilds its camera-vertex table, whether or not its inputs changed (ctx_render.hip CameraTableKey)
    SW_NO_SKY_PLANE,        // small-scene path, head form with 32-byte entries: the sky term stays three float atomics on the colour plane (no ShadeArgs::planes.sky)
    SW_COUNT
};
struct SwitchTable
{
    int64_t v[SW_COUNT];
    bool    on(CapSwitch k) const { return v[k] > 0; }              // presence flags: set and not 0
    int64_t get(CapSwitch k, int64_t dflt) const { return v[k] >= 0 ? v[k] : dflt; }
};

struct LaunchCfg
{
    hipStream_t stream;
    uint32_t    grid_blocks;    // persistent grid size for queue kernels
    uint32_t    stack_entries;  // 32 or 64 (per-lane LDS traversal stack)
    uint32_t    cu_count = 0;   // compute units (0: unknown) -- persistent kernels with a static chunk assignment clamp their grid
                                // to what is resident at once, see resident_grid() below
    uint32_t    any_no_probe = 0;  // launch_trace_any: the producer already probed (ShadeArgs::inline_probe): plain per-chunk kernel
    const SwitchTable* sw = nullptr;  // the context's A/B switches (null: every switch at the product's choice)
    bool    sw_on(CapSwitch k) const { return sw && sw->on(k); }
    int64_t sw_get(CapSwitch k, int64_t dflt) const { return sw ? sw->get(k, dflt) : dflt; }
};

// Kernels that deal their chunks out statically (wave w takes slots w, w + W, ...): a workgroup that is not resident from the start
// runs its whole share after the others have finished.  Their grids are therefore clamped to what the runtime says fits at once
// (measured on the 262 k-triangle scene: 5 workgroups per CU requested with 32-KB stacks, 4 resident, closest hit 11.3 ms; 24-KB
// stacks, 5 resident, 7.9 ms).  One answer per kernel instantiation, asked once.
template <auto K>
uint32_t resident_grid(const LaunchCfg& cfg, uint32_t want)
{
    static int per_cu = -1;
    if (per_cu < 0)
    {
        int n = 0;
        per_cu = (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, K, (int)kBlock, 0) == hipSuccess && n > 0) ? n : 0;
        if (cfg.sw_on(SW_TRACE_LAUNCHES)) fprintf(stderr, "[cap] resident workgroups per CU: %d\n", per_cu);
    }
    if (!cfg.cu_count || !per_cu) return want;
    const uint32_t cap = cfg.cu_count * (uint32_t)per_cu;
    return want < cap ? want : cap;
}
// the persistent grid of a queue kernel: one workgroup per kBlock entries, at most cfg.grid_blocks
inline uint32_t queue_grid(const LaunchCfg& cfg, uint32_t max_count)
{
    uint32_t g = (max_count + kBlock - 1) / kBlock;
    if (g > cfg.grid_blocks) g = cfg.grid_blocks;
    return g ? g : 1;
}

// ---- trace ----
// Primary visibility (rt_primary_visibility.hlsl:35-49): generates camera rays for frame slots [0, n_slots) of
// the batch and writes hit records (u, v, asfloat(global triangle id | ~0u), t) at index slot * Ppad + pl.
// work: kQueueClasses zeroed chunk-grab counters (kCounterStride apart) for the persistent wide-tree variant, or NULL
void launch_trace_primary(const LaunchCfg& cfg, const BvhDev& bvh, const CameraDev& cam, const ScreenDev& screen,
                          const FrameConst* frames, uint32_t n_slots, float4* hits, uint32_t* work);
// Camera rays written as a ray queue whose entry i belongs to path i (= slot * Ppad + local pixel): q.org_tmin / q.dir_tmax hold
// n_slots * Ppad entries, q.count the 64 sub-queue counters (set by the kernel), q.class_capacity = ceil(n_slots * Ppad / 64) rounded
// up to a multiple of 64.  launch_trace_closest8 on it writes hits[i] exactly where launch_trace_primary would have.
void launch_raygen_identity(const LaunchCfg& cfg, const CameraDev& cam, const ScreenDev& screen, const FrameConst* frames, uint32_t n_slots,
                            const RayQueue& q);
// Closest hit for the extension-ray queue (rt_indirect.hlsl:173).
void launch_trace_closest(const LaunchCfg& cfg, const BvhDev& bvh, const RayQueue& q, uint32_t max_count, float4* hits);
// The same on the compressed 8-wide view of the tree (trace8.hip; needs bvh.wide8_ok).  work: kQueueClasses zeroed chunk-grab counters.
void launch_trace_closest8(const LaunchCfg& cfg, const BvhDev& bvh, const RayQueue& q, uint32_t max_count, float4* hits, uint32_t* work);
void launch_trace_closest8_camera(const LaunchCfg& cfg, const BvhDev& bvh, const RayQueue& q, uint32_t max_count, float4* hits, uint32_t* work,
                                  const CameraDev& cam, const ScreenDev& screen, const FrameConst* frames, uint32_t n_slots);
// Any hit for the shadow-ray queue (lighting.h:48-61); unoccluded rays add contrib to target[plane index].
// guard: 8 x uint64 {-, malformed path ids seen by shade, by trace_any, last offender, appends beyond a class's capacity, -, -, -}
// work: kQueueClasses zeroed chunk-grab counters for this launch (exhaustive path; may be NULL for the LBVH kernels)
void launch_trace_any(const LaunchCfg& cfg, const BvhDev& bvh, const ShadowQueue& q, uint32_t max_count, float4* target,
                      uint32_t pixels_padded, uint32_t n_slots, uint64_t* guard, uint32_t* work, bool mostly_unoccluded,
                      const FrameConst* frames, float4* code_plane = nullptr);
// code_plane (ShadeArgs::code_in_color, bounce 0 of the small-scene path): target holds nothing yet.  An unoccluded ray stores its
// contribution there instead of adding it, and marks the path's word code_plane[plane index].w (code -> code + kCodeLit).
// Only the two small-scene kernels of the reference model have the form (stack_entries == 0, !mostly_unoccluded).  Any other kernel
// would ignore code_plane and ADD to a `direct` nobody has written, unmarked and without an error: launch_trace_any asserts the
// condition, and the only caller that passes a plane derives it from code_in_color, whose own condition (ctx_render.hip plan_render) implies it.

// The same for the reference model's shadow rays on the wide view with lane refill (trace8.hip): dense scenes, where a traversal step's
// round trip ends in HBM.  Needs bvh.wide8_ok and the zeroed grab counters `work`.
void launch_trace_any8_refill(const LaunchCfg& cfg, const BvhDev& bvh, const ShadowQueue& q, uint32_t max_count, float4* target, uint32_t pixels_padded,
                              uint32_t n_slots, uint64_t* guard, uint32_t* work, const FrameConst* frames);

// Ray queries of caller-supplied rays (cap_trace_rays / cap_trace_occlusion): rays = CapRayDesc records as float4 pairs, out = CapHit
// records (float4) or one uint32 per ray.  work: [0] the wide kernels' chunk counter, [kCounterStride] the number of rays they passed
// to the binary tree in `defer` (zeroed per launch).  safe: origin components beyond it go to the binary tree (query.hip).
struct QueryArgs
{
    const float4* rays;
    uint32_t      n;
    void*         out;
    uint32_t*     work;
    uint32_t*     defer;
    float         safe;
};
constexpr float kQuerySafeScale = 4.0f;  // safe = this x max(scene extent, largest |coordinate|): see query.hip
bool query8_stack_matches();  // the wide query kernels' pair stack is the one the host checks the tree's depth against
struct RayFilter;  // ray flags and instance masks (below); NULL = the plain kernels
void launch_query8(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, bool any, const RayFilter* f = nullptr, bool first_hit = false);
// binary tree, per lane: every ray of q (deferred = false), or the q.work[kCounterStride] rays listed in q.defer
void launch_query_binary(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, bool any, bool deferred);
// Multi-hit queries (cap_trace_rays_multi, query.hip): q as above with q.out = k CapHit records per ray (NULL when k = 0); counts = n
// hit counts or NULL (then the k-th hit prunes); resume: slot k - 1 of each page is the cursor (CAP_MULTI_CONTINUE).  The kernels'
// list capacity is multi_bucket(k) >= k.
struct MultiArgs
{
    QueryArgs q;
    uint32_t  k;
    uint32_t* counts;
    uint32_t  resume;
};
constexpr uint32_t kMultiMaxK = 16;
uint32_t multi_bucket(uint32_t k);
void     launch_query8_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, const RayFilter* f = nullptr);
void     launch_query_binary_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, bool deferred, const RayFilter* f = nullptr);

// Ray flags and instance masks of the _ex queries (query.hip k_query_*_f): the face cull as tri_test_cull's two words, and the instance
// mask as one byte per GLOBAL triangle id (its mesh's mask; NULL while no table is
// installed, cap_scene_set_instance_masks) tested against `mask`.  Wave-uniform: kernel arguments, SGPRs.
struct RayFilter
{
    uint32_t       cull_and, cull_xor;
    uint32_t       mask;      // InstanceInclusionMask, 1..0xFF
    const uint8_t* tri_mask;  // NULL: no mask test
};
// launch_query_binary under a filter (query.hip k_query_binary_f; first_hit: closest only, the lane retires at its first accepted hit)
void launch_query_binary_filtered(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, const RayFilter& f, bool any, bool first_hit, bool deferred);

// Closest-point queries (cap_closest_points, point_query.hip): points = CapPointDesc records (float4: point, radius), out = CapClosest
// records (two float4 per point).  slack: the absolute part of the pruning bound, kClosestSlackScale x the largest coordinate magnitude
// of the scene bounds (DESIGN.md "Closest-point queries").  depth: the tree's max_depth, which picks the stack size.  f NULL: no mask table.
struct ClosestArgs
{
    const float4* points;
    uint32_t      n;
    float4*       out;
    float         slack;
};
constexpr float kClosestSlackScale = 1.0f / 262144.0f;  // 64 x 2^-24: the proof needs 52
void launch_closest_points(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestArgs& a, const RayFilter* f, uint32_t depth);
// cap_signed_distance (point_query.hip k_closest_points<.., true>): launch_closest_points, and signed_out[i] = the distance to the record's
// closest point, negative where the record's delta points against the pseudonormal normals[21 triangle + 3 feature] (+inf without a record)
struct SignedArgs
{
    const float* normals;
    float*       signed_out;
};
void launch_signed_distance(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestArgs& a, const SignedArgs& s, const RayFilter* f, uint32_t depth);
// Sphere sweep queries (cap_sweep_spheres, sweep.hip k_sweep_spheres): sweeps = CapSweepDesc records (two float4: origin, radius;
// direction, tmax), out = CapSweepHit records (two float4 per sweep).  mag: the largest coordinate magnitude of the scene bounds, which
// with the sweep's own origin and radius makes the absolute part of its prune radius (DESIGN.md "Sphere sweep queries").  depth and f
// as launch_closest_points'.
struct SweepArgs
{
    const float4* sweeps;
    uint32_t      n;
    float4*       out;
    float         mag;
};
constexpr float kSweepAccept     = 1.0f + 8.0f * 5.9604644775390625e-8f;  // 1 + kappa of the contract's part (C): kappa = 8 x 2^-24
constexpr float kSweepNudge      = 16.0f * 5.9604644775390625e-8f;        // what a refused candidate's step is lengthened by, x the coordinates' size
constexpr float kSweepSlackScale = 1.0f / 131072.0f;                      // 128 x 2^-24: the prune argument needs 58
void launch_sweep_spheres(const LaunchCfg& cfg, const BvhDev& bvh, const SweepArgs& a, const RayFilter* f, uint32_t depth);
// The k nearest and in-radius form (cap_closest_points_multi, point_query.hip k_closest_points_multi): a.out = pages of k CapClosest
// records per point (NULL when k = 0); counts = n candidate counts or NULL (then the k-th distance prunes); resume: slot k - 1 of each
// page is the cursor (CAP_MULTI_CONTINUE).  The list capacity is multi_bucket(k) >= k.
struct ClosestMultiArgs
{
    ClosestArgs a;
    uint32_t    k;
    uint32_t*   counts;
    uint32_t    resume;
};
void launch_closest_points_multi(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestMultiArgs& m, const RayFilter* f, uint32_t depth);
// Over the instance table (cap_closest_instances, point_query.hip k_closest_inst): nearest in world space, on the instance's transformed
// triangle.  a as above (a.slack is not read: the slack is per point and instance, cap_near.h); inst_out may be NULL.  descs: the
// CapInstanceDesc records as the caller gave them (4 float4 each; the contract's world record is built from M, not from W), near and
// xw_max: InstanceBuildArgs::near and misc + 7.  bvh, tl, f and depth as launch_query_instances'; bvh.tris_by_id the scene's records.
struct TlasDev;
struct ClosestInstArgs
{
    ClosestArgs     a;
    uint32_t*       inst_out;
    const float4*   descs;
    const float2*   near;
    const uint32_t* xw_max;
};
void launch_closest_instances(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestInstArgs& a, const TlasDev& tl, const RayFilter& f, uint32_t depth);
// cap_signed_distance_instances (point_query.hip k_closest_inst<.., true>): launch_closest_instances, and s.signed_out[j] = the world
// distance of the record, negative where the flat signed query at p' = W p over the winning instance's candidates says so (s.normals: the
// scene's pseudonormal table).  a.a.slack is READ here: the scene's flat slack (kClosestSlackScale), which bounds the object-space walk.
void launch_signed_distance_instances(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestInstArgs& a, const SignedArgs& s, const TlasDev& tl,
                                      const RayFilter& f, uint32_t depth);
// The k nearest and in-radius form over the instance table (cap_closest_instances_multi, point_query.hip k_closest_inst_multi): ia.a.out
// = pages of k CapClosest records per point and ia.inst_out = pages of k instances (both NULL when k = 0); counts, resume and the list
// capacity as ClosestMultiArgs' -- the cursor is slot k - 1 of both pages.
struct ClosestInstMultiArgs
{
    ClosestInstArgs ia;
    uint32_t        k;
    uint32_t*       counts;
    uint32_t        resume;
};
void launch_closest_instances_multi(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestInstMultiArgs& m, const TlasDev& tl, const RayFilter& f,
                                    uint32_t depth);

// Sphere sweeps over the instance table (cap_sweep_instances, sweep.hip k_sweep_inst; a = SweepArgs above): the sweeps are in world space, a.out as above and inst_out the
// instance of each record (may be NULL).  a.mag is not read: the prune radius is per sweep and instance (cap_near.h
// sweep_prune_radius).  descs, near and xw_max as ClosestInstArgs'; bvh, tl, f and depth as launch_closest_instances'.
struct SweepInstArgs
{
    SweepArgs       a;
    uint32_t*       inst_out;
    const float4*   descs;
    const float2*   near;
    const uint32_t* xw_max;
};
void launch_sweep_instances(const LaunchCfg& cfg, const BvhDev& bvh, const SweepInstArgs& a, const TlasDev& tl, const RayFilter& f, uint32_t depth);

// Box overlap queries (cap_overlap_boxes, overlap.hip k_overlap_boxes): boxes = CapBoxDesc records (two float4: lo, hi; the w words are
// not read), out = pages of k triangle ids per box (NULL when k = 0), counts = n candidate counts or NULL, resume: slot k - 1 of each
// page is the cursor (CAP_MULTI_CONTINUE).  slack: what the query box is grown by before it is compared with the node boxes,
// kClosestSlackScale x the largest coordinate magnitude of the scene bounds (DESIGN.md "Box overlap queries").  depth and f as
// launch_closest_points'; the list capacity is multi_bucket(k) >= k.
struct OverlapArgs
{
    const float4* boxes;
    uint32_t      n;
    uint32_t*     out;
    uint32_t      k;
    uint32_t*     counts;
    uint32_t      resume;
    float         slack;
};
void launch_overlap_boxes(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapArgs& a, const RayFilter* f, uint32_t depth);
// Triangle overlap queries (cap_overlap_triangles, overlap.hip k_overlap_triangles): queries = CapTriangleDesc records (three float4: (a,
// skip bits) (b, -) (c, -)); out, k, counts, resume, slack, depth and f as OverlapArgs' -- the walk is the box query's against the box
// of the query's three vertices.
struct OverlapTriArgs
{
    const float4* queries;
    uint32_t      n;
    uint32_t*     out;
    uint32_t      k;
    uint32_t*     counts;
    uint32_t      resume;
    float         slack;
};
void launch_overlap_triangles(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapTriArgs& a, const RayFilter* f, uint32_t depth);
// Over the instance table (cap_overlap_instances, overlap.hip k_overlap_inst): the boxes are in world space, a.out = pages of k triangle
// ids and inst_out = pages of k instances (both NULL when k = 0) -- the cursor is slot k - 1 of both.  a.slack is not read: the slack is
// per box and instance (cap_near.h overlap_slack).  descs, near and xw_max as ClosestInstArgs'; bvh, tl, f and depth as
// launch_closest_instances'.
struct OverlapInstArgs
{
    OverlapArgs     a;
    uint32_t*       inst_out;
    const float4*   descs;
    const float2*   near;
    const uint32_t* xw_max;
};
void launch_overlap_instances(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapInstArgs& a, const TlasDev& tl, const RayFilter& f, uint32_t depth);
// Triangle overlap queries over the instance table (cap_overlap_triangles_instances, overlap.hip k_overlap_tri_inst): the queries are in
// world space and their second w word is the skip pair's instance; a.out and inst_out are the two pages of OverlapInstArgs, a.slack is
// not read (the slack is per query and instance).  The rest as OverlapInstArgs'.
struct OverlapTriInstArgs
{
    OverlapTriArgs  a;
    uint32_t*       inst_out;
    const float4*   descs;
    const float2*   near;
    const uint32_t* xw_max;
};
void launch_overlap_triangles_instances(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapTriInstArgs& a, const TlasDev& tl, const RayFilter& f,
                                        uint32_t depth);

// ---- instances (instance.hip): cap_instances_set, cap_trace_instances* ----
// The table on the device.  rec: 4 float4 per instance = the three rows of W (world to object, row r = (W_r0, W_r1, W_r2, W_r3)) and
// (asfloat(mask), asfloat(root of the object's tree), asfloat(object index), -); an inert instance has W = 0 and mask 0.  box: 2 float4 per instance = (lo.xyz, k) (hi.xyz, asfloat(index)),
// k >= 0 the per-ray inflation factor of tlas_slab (instance.hip), k < 0 for an inert instance or a padding entry.
// tlas: the top-level tree, an implicit binary tree over the instances in Morton order.  Level 0 holds the instances' box records in
// that order, level l + 1 entry j the union of level l entries 2 j and 2 j + 1; every level is padded to an even number of entries with
// k < 0 records, level l starts at entry level_off[l], the last level (`top`) has one entry.
// objects: what an instance can show -- the objects of cap_objects_set, or one entry, the scene, without an object table.
struct InstObject
{
    double   blo[3], bhi[3];  // the object-space box every reported hit point lies in (the object's bounds + the build's padding)
    int32_t  root;            // root of the object's tree as BvhDev::root, in the pools the query is given
    uint32_t reserved;
};
struct InstanceBuildArgs
{
    const float*      descs;  // CapInstanceDesc records, 16 words each (device)
    uint32_t          n;
    const InstObject* objects;       // (device)
    uint32_t          n_objects;
    const uint32_t*   object_index;  // per instance (device); NULL: all 0.  An index >= n_objects makes the instance inert
    float4*      rec;
    float4*      box;
    float4*      tlas;
    float2*      near;  // per instance (g, Xw): the distance prune of cap_closest_instances (cap_near.h); (0, 0) for an inert instance
    uint32_t*    keys[2];
    uint32_t*    vals[2];
    uint32_t*    hist;
    uint32_t*    scan;
    uint32_t*    misc;  // 8 words: 6 ordered-uint bounds of the live boxes' centres, the inert count, the largest Xw as float bits
};
constexpr uint32_t kTlasMaxLevels = 25;  // n <= 2^24: levels 0 .. 24
// level_off[0 .. top] and the total number of entries for n instances; returns top
uint32_t tlas_layout(uint32_t n, uint32_t level_off[kTlasMaxLevels], uint32_t* total);
void     launch_instances_build(hipStream_t stream, const InstanceBuildArgs& a);
struct TlasDev
{
    const float4*   rec;
    const float4*   tlas;
    const uint32_t* level_off;  // device copy of tlas_layout's table
    uint32_t        top;
};
// mode 0: closest, 1: first accepted hit, 2: occlusion.  q.out as the other queries'; inst_out (closest / first only) may be NULL.
// f.tri_mask NULL: no per-mesh masks.  Always a binary tree below an instance (DESIGN.md "Instances"): bvh.nodes / bvh.tris are the
// pools the instance records' roots refer to -- the scene's tree, or the forest of an object table -- and depth the largest
// max_depth of the trees in them.
void launch_query_instances(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, const TlasDev& tl, const RayFilter& f, int mode, uint32_t* inst_out,
                            uint32_t depth);
// Multi-hit over the instances (cap_trace_instances_multi, instance.hip k_query_inst_multi): m as launch_query_binary_multi's, pages of
// m.k records per ray in m.q.out and of m.k instance indices in inst_out (both NULL when m.k = 0); with m.resume slot k - 1 of both
// is the cursor (t, instance, triangle).  bvh.tris_by_id must be the scene's records whichever pools bvh.nodes / bvh.tris are.
void launch_query_instances_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, const TlasDev& tl, const RayFilter& f, uint32_t* inst_out,
                                  uint32_t depth);
// An object's tree as a builder left it at its place in the forest (cap_objects_set): nodes = the object's n_tris - 1 nodes, tris its
// n_tris leaf-order records, both numbered from 0 with triangle ids local to the object.  Adds node_base to inner child references,
// rec_base to leaf references and first_triangle to the records' id words, in place.
struct ForestRelocArgs
{
    float4*  nodes;
    float4*  tris;
    uint32_t n_tris, node_base, rec_base, first_triangle;
};
void launch_forest_relocate(hipStream_t stream, const ForestRelocArgs& a);

// ---- shade ----
struct ShadeArgs
{
    SceneDev          scene;
    CameraDev         cam;
    ScreenDev         screen;
    const FrameConst* frames;
    // One word, two readers that never meet: the stand-alone shade stage of the tree path reads `hits`; the fused small-scene kernels take
    // their hit from registers and read `sample_terms` (see below).  Sharing it keeps the kernel arguments of every kernel as they were.
    union
    {
        const float4* hits;
        const float4* sample_terms;
    };
    RayQueue          in;       // unused for the first bounce (identity queue)
    RayQueue          out;
    ShadowQueue       shadow;
    Planes            planes;
    uint32_t          n_slots;     // frame slots in this batch
    uint32_t          bounce;
    uint32_t          num_bounces;
    uint32_t          max_count;   // upper bound of the input queue length
    uint32_t          aov_slot;    // frame slot whose AOVs are kept, or ~0u
    uint64_t*         shaded_counter;
    uint32_t*         work;        // fused kernels: kQueueClasses chunk-grab counters of this launch (zeroed), kCounterStride apart
    // Eighty bytes, two readers that never meet (like hits / sample_terms above: the kernel arguments of every kernel stay as they were):
    // the feedback variants read `fb`, the head kernels -- reference model without feedback -- read `walk`, the order in which bounce 0's
    // chunk indices visit the batch's (frame slot, 64-pixel group) pairs (cap_device.h head_chunk; set per batch by render_batch)
    union
    {
        FeedbackDev   fb;
        HeadWalk      walk;
    };
    // untextured scene, reference shading, accumulate-only render (nobody but the resolve reads the planes): the first vertex's albedo
    // is one of four constants, so the albedo plane is not used and direct.w carries a code instead of 1 (cap_shade.h shade_vertex)
    uint32_t          albedo_in_w;
    // EXT model on the small-scene path: the next-event shadow ray is tested inside the fused kernel (same exhaustive loop as the
    // any-hit kernel's) and the path carries its gathered radiance in the extension queue (RayQueue::acc); the colour plane is
    // written once, when the path ends, the direct plane once at bounce 0 -- no shadow queue, no any-hit launch, no scattered
    // read-modify-write.  The sums are the same additions in the same (bounce) order.
    uint32_t          inline_nee;
    // Reference model on the small-scene path: the fused kernel tests every shadow ray it generates against ONE fan pair -- the one
    // farthest along the batch's first light direction, which occludes most of them -- and only queues the survivors for the any-hit
    // kernel (which then tests every pair, without a probe of its own).  Occlusion is an OR over the pairs: same result.
    // The shadow rays the probe answered are rays of the statistics, not entries: the launch adds their number to word 2 of its
    // classes' counter lines (flush_stats).
    uint32_t          inline_probe;
    // ... and from bounce 1 on the survivors are traced by the wave that found them (k_trace_shade's per-wave ring): the only
    // any-hit launch left on the small-scene path is bounce 0's
    uint32_t          wave_ring;
    uint32_t          cull_camera_pairs;  // bounce 0 of the small-scene path: the camera basis is orthonormal, so a tile may skip the pairs off its screen area
    // albedo_in_w on the small-scene path (reference model): the code sits in color.w, which every later writer of the colour plane carries
    // through, and bounce 0 writes no direct plane at all: zeros and the sky constant are what the code already says.  The bounce-0
    // any-hit launch stores the contribution of an unoccluded ray into `direct` and turns the code c into c + 4, "direct holds a value";
    // the resolve loads `direct` only there.  An entry of `direct` an earlier batch left is never read: the word that says whether to
    // read it is rewritten by every batch's bounce 0.  Set by the host only where every kernel involved has the form: the fused
    // kernel of bounce 0 (trace_shade_has_code_form), the small-scene any-hit kernels (launch_trace_any's code_plane) and the resolve.
    uint32_t          code_in_color;
    // sample_terms (above; fused small-scene launches only, where it is always set): this bounce's block [frame slot][4096] of the batch's
    // table of direction-sample terms (launch_sample_terms), or null: the sample travels in the queue entries and every vertex computes
    // its own terms.  All launches of a batch take the same form (launch_trace_shade); the last bounce samples nothing and reads
    // nothing through it.
};
static_assert(sizeof(HeadWalk) <= sizeof(FeedbackDev), "ShadeArgs::walk must not grow the kernel arguments");
// The first vertex's code (direct.w under albedo_in_w, color.w under code_in_color).  Three places must agree on it: shade_vertex
// (the plane's word, and under CODE the spare word of a bounce-0 shadow entry), store_first_direct (+ kCodeLit) and the resolves.
constexpr float kCodePadding = 0.f, kCodeSky = 1.f, kCodeKd = 2.f, kCodeBlack = 3.f;
constexpr float kCodeLit = 4.f;  // code_in_color: added where the bounce-0 any-hit launch stored a contribution into `direct`
// Pixels the bounce-0 kernel grows every fan pair's screen bounds by (small_scene.hip stage_camera_pairs).  The host's gate for
// cull_camera_pairs (ctx_render.hip) allows a camera basis to move a projected point by an eighth of it.
constexpr float kCameraCullPad = 2.0f;
// feedback: vertices of bounce >= 1 that the previous frame saw take its shaded colour and end the path (rt_indirect.hlsl:116-145;
// reference shading model only)
void launch_shade(const LaunchCfg& cfg, const ShadeArgs& args, bool ext, bool feedback = false);
// tree path, bounce 0: camera-ray packet walk + shading in one kernel (args.work = bounce 0's grab counters); false if the
// configuration does not take the packet walk -- then launch_trace_primary + launch_shade do the same in two kernels
bool launch_primary_shade(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, float4* hits, bool ext);
// small-scene path: exhaustive closest hit fused with the shading of the vertex found (bounce 0 generates the camera rays)
// returns how the launched kernel builds the closest-hit candidate mask (CAP_DEBUG_MARK_FORM's form)
// camera_head: args.bounce == 1 and the launch does bounce 0 as well, as the head of every chunk of bounce 0's identity queue, from the
// batch's table of camera vertices: args.in.org_tmin / dir_tmax = the table's two planes (launch_camera_vertices), args.in.thr_pid =
// bounce 0's block of the sample table, args.in.count = bounce 0's counter lines; args.frames[s].pad1 = slot s's jitter group.  Needs
// sample_terms, inline_probe and wave_ring, and a batch whose colour plane carries the code (code_in_color).  Its bounce-0 shadow rays go
// through the wave rings: no any-hit launch follows bounce 0.
// gray: the extension queues args.in (not under camera_head, where it is the table) and args.out hold 32-byte entries (RayQueue) and
// thr_pid is neither read nor written.  Needs sample_terms and trace_shade_has_gray_form(); every launch of a batch or none.
// sky_plane: a path that escapes at bounce >= 1 stores its throughput into args.planes.sky and adds nothing to the colour plane; the
// head launch zeroes the plane for the whole batch and launch_resolve(.., sky_plane) adds the term.  Needs gray, the batch's first
// launch to be the camera_head one and code_in_color (whose albedo_in_w frees the word of Planes that carries the plane); every launch
// of a batch and its resolve, or none.
uint32_t launch_trace_shade(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, bool ext, bool feedback = false, bool camera_head = false,
                            bool gray = false, bool sky_plane = false);
// whether the reference model's bounce 0 of this scene has the form ShadeArgs::code_in_color asks for (the kernel of tame records in LDS)
bool trace_shade_has_code_form(const BvhDev& bvh, const SceneDev& scene);
// ... and the form ShadeArgs::sample_terms asks for (the lean kernels)
bool trace_shade_has_table_form(const BvhDev& bvh, const SceneDev& scene);
// ... and 32-byte extension entries (launch_trace_shade's gray): the table kernels on a scene without textures
bool trace_shade_has_gray_form(const BvhDev& bvh, const SceneDev& scene);
// The premise of that form on a 48-byte queue: out_device[0] += entries of q, up to its class counts, whose three throughput words are not
// bitwise equal; out_device[1] += entries looked at.
void launch_gray_selftest(hipStream_t stream, const RayQueue& q, unsigned long long* out_device);
// The batch's table of direction-sample terms: table[(b * n_slots + s) * 4096 + ((y mod 64) << 6 | x mod 64)] = (ca, cb, cos_theta, 0) of
// hemisphere_terms() of the blue-noise sample of count = frames[s].frame_count * 25 + b, for b < num_bounces (the bounces that sample).
void launch_sample_terms(hipStream_t stream, const float2* bluenoise, const FrameConst* frames, uint32_t n_slots, uint32_t num_bounces, float4* table);
// out_device[0] += entries of such a table that differ from the per-vertex evaluation in any bit, out_device[1] += entries compared
void launch_sample_terms_selftest(hipStream_t stream, const float2* bluenoise, const FrameConst* frames, uint32_t n_slots, uint32_t num_bounces,
                                  const float4* table, unsigned long long* out_device);

// The batch's table of camera vertices (small_scene.hip k_camera_vertices): one entry per (jitter group, padded pixel), rows = groups;
// args.frames[g].pad2 = the first slot of group g.  selftest_out != null: rows = the batch's slots, nothing is written, every slot's own
// bounce-0 vertex is compared with the entry of its group (args.frames[s].pad1): out[0] += mismatches, out[1] += entries compared.
void launch_camera_vertices(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, uint32_t rows, float4* tab_p, float4* tab_n,
                            unsigned long long* selftest_out = nullptr);

// ---- accumulate / exchange ----
// accum[pl] += sum over slots (in slot order) of color*albedo + direct; .w counts frames.
// sky_plane (with code_in_color): color.xyz + planes.sky * (0.7, 0.7, 0.85) stands for color.xyz (launch_trace_shade's sky_plane)
void launch_resolve(const LaunchCfg& cfg, const Planes& planes, uint32_t n_slots, uint32_t pixels_padded, float4* accum,
                    bool albedo_in_w = false, float kd_untextured = 0.0f, bool code_in_color = false, bool sky_plane = false);
// out_device[0] += the words of sky[0 .. n) that are not +0 (CAP_DEBUG_SKY_PLANE_NONZERO)
void launch_sky_nonzero(hipStream_t stream, const float* sky, size_t n, unsigned long long* out_device);
// plane_kind: 0 copy, 1 combined (color*albedo+direct from the three planes at slot offset), 2 mean (xyz / w)
void launch_untile(const LaunchCfg& cfg, const ScreenDev& screen, const float4* src, const float4* albedo, const float4* direct,
                   int plane_kind, float4* image);
// the inverse of launch_untile(.., 0, ..): a row-major image into this shard's tile order (cap_accum_import)
void launch_tile(const LaunchCfg& cfg, const ScreenDev& screen, const float4* image, float4* dst);
// s0 may be null (its image is produced elsewhere)
void launch_untile4(const LaunchCfg& cfg, const ScreenDev& screen, const float4* s0, const float4* s1, const float4* s2, const float4* s3,
                    float4* d0, float4* d1, float4* d2, float4* d3);
void launch_tiles_mean(const LaunchCfg& cfg, const float4* accum, uint32_t pixels_padded, float4* dst);
// shard_stride: float4 elements between two shards' buffers (0: pixels_padded, i.e. back to back)
void launch_assemble(const LaunchCfg& cfg, const ScreenDev& screen, const float4* gathered, uint32_t shard_count, float4* image,
                     size_t shard_stride = 0);
void launch_geo_aov(const LaunchCfg& cfg, const SceneDev& scene, const float4* hits_slot, uint32_t pixels_padded, float4* aov_geo);

// ---- LBVH build (bvh.hip) ----
struct BvhBuildArgs
{
    // inputs: GeometryStorage layout on the device
    const float*    positions;
    const float*    normals;
    const float*    texcoords;
    const uint32_t* indices;
    const uint4*    tri_ids;        // (instance, primitive, texture index, -) per global triangle
    const uint4*    mesh_offsets;   // per mesh: (first_vertex_offset, first_index_offset, -, -)
    uint32_t        tri_count;
    // outputs
    float4*         shade_tris;     // kShadeRec per triangle, global order
    float4*         tris_sorted;    // 4 per triangle, leaf order
    float4*         nodes;          // 4 per internal node
    uint32_t*       leaf_tri;       // global triangle id per leaf
    // scratch
    float4*         tri_raw;        // 4 per triangle, global order
    float4*         tri_box;        // 2 per triangle (lo, hi), global order
    uint32_t*       keys[2];
    uint32_t*       vals[2];
    uint32_t*       hist;           // radix histogram scratch: 256 * blocks
    uint32_t*       parent;         // [2*tri_count] parents of internal nodes then leaves, (parent << 1) | slot
    uint32_t*       flags;          // [tri_count] refit arrival counters
    uint32_t*       bounds;         // 6 orderable-uint encoded floats
    uint32_t*       max_depth;      // 2: the tree's depth; 1 if any triangle's stored normals are not tame (SceneDev::shade_tame)
};
size_t bvh_radix_blocks(uint32_t n);
void   launch_bvh_build(hipStream_t stream, const BvhBuildArgs& a);
int    launch_bvh_sort(hipStream_t stream, const BvhBuildArgs& a);  // setup + Morton order only: a.keys[r] / a.vals[r] sorted, returns r
// the build's radix sort alone (also the instance table's, instance.hip): n (key, value) pairs sorted by key, stable; the result is
// keys[r] / vals[r] for the returned r.  hist: 256 * bvh_radix_blocks(n) words, scan: bvh_radix_scan_words(n) words of scratch.
size_t bvh_radix_scan_words(uint32_t n);
int    launch_radix_sort_pairs(hipStream_t stream, uint32_t* const keys[2], uint32_t* const vals[2], uint32_t n, uint32_t* hist, uint32_t* scan);
size_t bvh_scan_scratch_words(uint32_t total);
void   launch_exclusive_scan_u32(hipStream_t stream, uint32_t* v, uint32_t total, uint32_t* scratch);  // exclusive scan of v[0 .. total) in place
// Agglomerative build with a surface-area distance over the Morton order (ploc.hip); same outputs as launch_bvh_build,
// incl. the subtree counts in a.keys[1].  boxes: 4 * tri_count float4; ints: 3 * tri_count + 4 words.  Returns 0 on success.
struct PlocScratch
{
    float4*   boxes;
    uint32_t* ints;
};
int    launch_bvh_build_ploc(hipStream_t stream, const BvhBuildArgs& a, const PlocScratch& s, uint32_t radius);
// Binned surface-area splits from the root down to segments of <= `leaf` triangles, the clustering inside those (ploc.hip,
// "sah_device"); same outputs and the same PlocScratch, plus bvh_sah_device_scratch_words(n) words of its own.
size_t bvh_sah_device_scratch_words(uint32_t n);
int    launch_bvh_build_sah_device(hipStream_t stream, const BvhBuildArgs& a, const PlocScratch& s, uint32_t* scratch, uint32_t radius, uint32_t leaf);
// Host-built tree (sah_builder.cpp): setup = triangle records, boxes and scene bounds only; finish = after `nodes` and
// `leaf_tri` have been uploaded: intersection records into leaf order + the wide view.
void launch_bvh_setup(hipStream_t stream, const BvhBuildArgs& a);
void launch_bvh_finish_host(hipStream_t stream, const BvhBuildArgs& a);

// Compressed 8-wide view (wide_builder.cpp builds the nodes on the host): intersection records into its leaf order.
void     launch_gather_wide(hipStream_t stream, const uint32_t* tri_src, const float4* tris_sorted, uint32_t n, float4* tris8);
// Device-side collapse of the device-built binary tree (needs BvhBuildArgs::keys[1] = the subtree counts launch_bvh_build leaves
// there).  task: capacity words of scratch; cnt: 2 * capacity; alloc: 2 words; nodes8: capacity * kWideNodeStride words; tri_src: n_tris words.
struct WideCollapseArgs
{
    const float4*   bnodes;
    const uint32_t* count;
    uint32_t        n_tris, capacity;
    double          pad;
    uint32_t *      task, *alloc, *nodes8, *tri_src;
    uint32_t*       cnt;  // 2 * capacity + 2 * (capacity / 1024 + 2) words: per node of the level being written, (inner children, triangles) -> their bases; the scan's tile sums behind
    uint32_t        begin, end;
};
// level_begin (may be null): the first node of every level, then the node count -- level l = [level_begin[l], level_begin[l + 1])
int      launch_wide_collapse(hipStream_t stream, WideCollapseArgs a, uint32_t* node_count, uint32_t* depth, uint32_t* top_nodes,
                          std::vector<uint32_t>* level_begin = nullptr);
// ---- pseudonormal table (pseudonormal.hip, cap_pseudonormals_build): the sign of cap_signed_distance ----
// table: 21 floats per triangle by global id, seven entries of three indexed by CAP_FEATURE_*.  Everything else is build scratch, C = 3 x
// tri_count words each unless said; stats: 8 words = vertices, edges, boundary, non-manifold and inconsistent edges, degenerate triangles.
struct PseudonormalArgs
{
    const float*    positions;
    const uint32_t* indices;
    const uint4*    tri_ids;
    const uint4*    mesh_offsets;
    uint32_t        tri_count;
    float*          table;
    uint32_t *      kx, *ky, *kz;  // the corners' position bits; then (dead mark, lower, higher weld id) of the half-edges
    uint32_t*       keys[2];
    uint32_t*       vals[2];
    uint32_t*       weld;          // weld id per corner
    uint32_t*       flag;          // run starts, then their exclusive scan
    uint32_t*       hist;          // 256 * bvh_radix_blocks(C)
    uint32_t*       scan;          // pseudonormal_scan_words(C)
    double*         nf;            // the face normal, 3 per triangle
    double*         ang;           // the corner angles, 3 per triangle
    uint32_t*       stats;
};
size_t pseudonormal_scan_words(uint32_t corners);
void   launch_pseudonormals_build(hipStream_t stream, const PseudonormalArgs& a);

// ---- winding numbers (winding.hip): the dipole table of cap_winding_build and the walk of cap_winding_numbers ----
// table: 4 float4 per inner node of the binary tree, per child slot (p~.xyz, r) (N.xyz, asfloat(traversal child code)): the record of
// include/capsaicin_hip.h ("winding numbers").  Everything else is build scratch: tri_sums 7 doubles per triangle in leaf order
// (n_t, a_t, a_t c_t), sums 14 doubles per inner node (a slot's N, A, M), parent and flags one word per inner node, stats 2 words
// (degenerate triangles, -), root 7 doubles (the whole tree's N, A, M).
struct WindingBuildArgs
{
    const float*    positions;
    const uint32_t* indices;
    const uint4*    tri_ids;
    const uint4*    mesh_offsets;
    uint32_t        tri_count;
    const float4*   nodes;
    const uint32_t* leaf_tri;
    float4*         table;
    double*         tri_sums;
    double*         sums;
    uint32_t*       parent;
    uint32_t*       flags;
    uint32_t*       stats;
    double*         root;
    // An object's tree in the forest (cap_winding_instances; zeros and NULL for the scene's tree): nodes, table, sums, parent and flags
    // point at the object's own first node and are indexed from 0, while the child codes the nodes hold are the forest's -- node_base
    // and rec_base are what k_forest_relocate added to them.  The forest keeps no leaf_tri: rec_ids = the object's leaf-order records,
    // whose word 12 is the global triangle id.
    uint32_t        node_base, rec_base;
    const float4*   rec_ids;
};
void launch_winding_build(hipStream_t stream, const WindingBuildArgs& a);
// points = CapPointDesc records (the radius is not read), out = one float per point, visits = 2 words per point (far terms, exact
// triangles) or NULL.  bvh.tris are the leaf-order records, bvh.root / tri_count the scene's; depth: the tree's max_depth.
struct WindingArgs
{
    const float4* points;
    uint32_t      n;
    const float4* table;
    float         beta;
    float*        out;
    uint32_t*     visits;
};
void launch_winding_numbers(const LaunchCfg& cfg, const BvhDev& bvh, const WindingArgs& a, uint32_t depth);
// The derived tables of cap_winding_instances (winding.hip; include/capsaicin_hip.h "winding numbers over instances"), all on one stream:
//   inst      3 float4 per instance: L row-major (9 words), |det L|, sigma, s = +1 / -1, or 0 for an instance that does not contribute
//   top       2 float4 per TLAS entry, in the layout of `tlas`: (p~_w, r) (N_w, word 7); r = -1 marks an empty entry
//   top_sums  7 doubles per TLAS entry (N_w, weight, weight p~_w): level 0 from the objects' root sums, a level above = entry 2 j + entry 2 j + 1
//   obj_root  7 doubles per object (N, A, M of the whole object: WindingBuildArgs::root of its build)
//   count     1 word: the contributing instances
struct WindingInstBuildArgs
{
    const float4*   descs;  // CapInstanceDesc records
    const float4*   rec;    // the instance records of k_instance_setup: word 12 the live mask, word 14 the object
    const float4*   tlas;
    uint32_t        n;
    const double*   obj_root;
    float4*         inst;
    float4*         top;
    double*         top_sums;
    uint32_t*       count;
};
void launch_winding_instances_build(hipStream_t stream, const WindingInstBuildArgs& a);
// cap_winding_instances (k_winding_inst): a = the points, beta and outputs as WindingArgs' with visits = 4 words per point, a.table the
// dipole table of the pools bvh.nodes / bvh.tris refer to (the scene's, or the forest's); depth: the deepest tree below an instance.
struct WindingInstArgs
{
    WindingArgs   a;
    const float4* inst;
    const float4* top;
};
void launch_winding_instances(const LaunchCfg& cfg, const BvhDev& bvh, const WindingInstArgs& a, const TlasDev& tl, uint32_t depth);

// ---- refit of the kept trees to moved vertices (refit.hip, cap_bvh_refit) ----
// binary tree: triangle setup (bounds reset first), parent links from the nodes, the build's climb (bvh.hip k_refit) in leaf order
void   launch_bvh_refit_climb(hipStream_t stream, const BvhBuildArgs& a);  // (bvh.hip) the climb alone
void   launch_refit_binary(hipStream_t stream, const BvhBuildArgs& a);
// expected node visits of the binary tree, 1 + sum(inner child box area) / root box area, into *out (device); nothing for n_tris < 2.
// scratch: tree_visits_scratch() doubles.  A fixed reduction order: the same boxes give the same bits.
size_t tree_visits_scratch();
void   launch_tree_visits(hipStream_t stream, const float4* nodes, uint32_t n_tris, double* scratch, double* out);
// 8-wide view, level by level from the deepest (after the binary refit and the gather of tris8): boxes = 6 floats per wide node
struct WideRefitArgs
{
    uint32_t*     nodes8;
    const float4* tris8;
    const float4* tri_box;
    float*        boxes;
    double        pad;           // kWidePad * max(extent, |coordinate|) of the NEW scene bounds
    uint32_t      one_triangle;  // the one-triangle scene (host collapse: its child box is the padded scene box)
    uint32_t      begin, end;
};
void launch_refit_wide(hipStream_t stream, WideRefitArgs a, const std::vector<uint32_t>& level_begin);
uint32_t wide8_stack_pairs();  // (g_base, g_mask) entries a lane of the wide kernels can hold: the tree's depth - 1 must fit

// ---- reconstruction chain (post.hip): Gather -> Accumulate -> BlurDisocclusion -> Blur -> Combine -> TAA ----
struct PostSettingsDev  // SettingsComponent subset, gui_system.h:20-37
{
    int   gather, denoise, eaw5;
    float eaw_normal_sigma, eaw_depth_sigma, eaw_luma_sigma;
    float gather_normal_sigma, gather_depth_sigma, gather_luma_sigma;
    float temporal_upscale_feedback, taa_feedback;
    int   lowres_indirect;  // UPSCALE2X: `indirect` is the (W/2, H/2) image of this frame's interleave offset
    int   use_variance;     // USE_VARIANCE of eaw_blur.hlsl
    int   fast_weights;     // hardware exp / log / rcp in the edge-stopping weights (toleranced mode)
    int   output;           // SettingsComponent::output = CombineIllumination's `type` (combine_illumination.hlsl:26-40): 0..3
};
struct PostChainArgs
{
    PostSettingsDev settings;
    uint32_t        width, height, frame_count;
    CameraDev       camera, prev_camera;
    // this frame's ray-pass outputs, row-major W*H ...
    const float4 *indirect, *direct, *albedo, *normal_depth;
    // ... or, on an unsharded context (cap_post_frame), straight from the render's tile-ordered planes: `tiled` = the screen's tile
    // columns (0 = row-major inputs as above).  Then `tiled_indirect` / `tiled_normal_depth` are untiled by the chain's first
    // kernel -- which decodes the normals on the way, so `normal_depth` is not needed row-major at all -- and Combine reads
    // `direct` / `albedo` in tile order: three image round trips less per frame.
    uint32_t      tiled;
    const float4 *tiled_indirect, *tiled_normal_depth;
    float4*       indirect_rowmajor;  // where the untiled indirect plane goes (the chain's `indirect` when tiled)
    ScreenDev     screen;
    // persistent state (raytracing_system.cpp:262-317)
    float4 *indirect_history[2], *moments_history[2], *combined_history[2], *prev_normal_depth;
    // scratch
    float4 *indirect_temp, *temp[2], *normals;  // normals: decoded (n.xyz, depth) of this frame
    // called on the host before pass p's launches, p = 0..4: Spatial gather, Temporal upscale, EAW, Combine illumination, TAA,
    // and with p = 5 after the last launch (per-pass timestamps like the reference's AllocateTimestampQueryPair); may be null
    void (*mark)(void* user, int pass);
    void* mark_user;
};
// The frame's output is combined_history[frame_count % 2] (raytracing_system.cpp:320-324).
void launch_post_chain(hipStream_t stream, const PostChainArgs& a);
// post.hip's unscaled IEEE division against the compiler's, on the device: out[0] mismatches of log2 over every normal float,
// out[1] over 2^30 operand pairs of the range it is used on (both must be 0; cap_debug_get(CAP_DEBUG_SELFTEST_DIV))
void launch_div_selftest(hipStream_t stream, unsigned long long* out_device);
// cap_shade.h's unscaled square roots and divisions of the small-scene shading against the compiler's: out[0] mismatches, out[1]
// comparisons made; which = 0 the unary forms over every float of their ranges, 1 = ortho_vector's pair over 2^31 candidates
void launch_shade_forms_selftest(hipStream_t stream, unsigned long long* out_device, uint32_t which);
// out[(y, x)] = full[(2y + oy, 2x + ox)]: the half-resolution indirect image of LOWRES_INDIRECT (rt_indirect.hlsl:53-59, :176)
void launch_decimate2x(hipStream_t stream, const float4* full, uint32_t width, uint32_t height, uint32_t ox, uint32_t oy, float4* out);
}  // namespace cap
