// cap_context.h — what the host units behind include/capsaicin_hip.h share (context.hip, ctx_render.hip, ctx_scene.hip, ctx_bvh.hip,
// ctx_query.hip, ctx_post.hip, ctx_comm.hip): the context and its buffers, the error reporting, and the helpers more than one unit calls.  Private to
// csrc/: nothing here is part of the ABI.
#pragma once

#include <array>
#include <string>
#include <utility>
#include <vector>

#include "../../include/capsaicin_hip.h"

#include "cap_kernels.h"

namespace cap
{
// sets cap_last_error() and returns `code` (context.hip, with the thread's message)
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                         \
    do                                                                                                        \
    {                                                                                                         \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(CAP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                                \
    } while (0)

template <typename T>
struct DevBuf
{
    T*     p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o)
        {
            release();
            p = o.p, n = o.n, o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr, n = 0;
    }
    hipError_t ensure(size_t count)
    {
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
};

enum StageId
{
    ST_PRIMARY,
    ST_CLOSEST,
    ST_ANY,
    ST_SHADE,
    ST_RESOLVE,
    ST_POST,
    ST_COUNT,
    ST_DIRECT,      // "RT Direct lighting": second label of the bounce-0 shading / shadow-ray spans
    ST_POST_PASS0,  // .. ST_POST_PASS0 + 4: "Spatial gather", "Temporal upscale", "EAW", "Combine illumination", "TAA"
    ST_NONE = -1
};

struct TimedSpan
{
    hipEvent_t a, b;
    int        stage;
    int        also = ST_NONE;  // a span may count under a second label
};

// guard block of a context (ShadeArgs::shaded_counter): {-, malformed path ids seen by shade, by trace_any, last offender, appends
// beyond a class's capacity, -, -, -}
constexpr size_t kGuardWords = 8;

// The counter block of a batch of `bounces` bounces (Lane::counters), in 32-bit words.  A queue has kQueueClasses x kCounterStride
// words; per bounce and class one 64-bit word counts both queues, low half = extension entries, high half = shadow entries (one atomic
// serves both), words 2 and 3 the probed shadow rays and the shaded vertices.  Three sections of one queue per bounce -- the queue
// counters, the chunk-grab counters of the fused launch, those of the any-hit launch -- and behind them the camera rays' identity queue.
// Only the first section is copied to the host (sync_and_collect).
struct CounterLayout
{
    uint32_t bounces;
    static constexpr size_t per_queue() { return (size_t)kQueueClasses * kCounterStride; }
    size_t    section() const { return (size_t)(bounces + 1) * per_queue(); }
    size_t    total() const { return 3 * section() + per_queue(); }
    uint32_t* ext(uint32_t* base, uint32_t b) const { return base + b * per_queue(); }
    uint32_t* shadow(uint32_t* base, uint32_t b) const { return base + 1 + b * per_queue(); }
    uint32_t* work_shade(uint32_t* base, uint32_t b) const { return base + section() + b * per_queue(); }
    uint32_t* work_any(uint32_t* base, uint32_t b) const { return base + 2 * section() + b * per_queue(); }
    uint32_t* identity(uint32_t* base) const { return base + 3 * section(); }
};

// what sync_and_collect must know of a batch to sum its counters
struct BatchCounted
{
    uint32_t num_bounces;
    bool     shadow_queued;  // false: the batch's shadow rays were traced where they were generated, and never were queue entries
};
}  // namespace cap

using namespace cap;

struct CapContext
{
    int         device = 0;
    hipStream_t stream = nullptr;
    bool        own_stream = false;
    int         cu_count = 256;

    // scene (GeometryStorage layout, asset_load_system.h:16-27)
    DevBuf<float>    positions, normals, texcoords;
    DevBuf<uint32_t> indices;
    DevBuf<uint4>    tri_ids;
    DevBuf<uint4>    mesh_offsets;
    DevBuf<uint32_t> mesh_texture;
    uint32_t         vertex_count = 0, index_count = 0, mesh_count = 0, tri_count = 0;
    bool             scene_ready = false;

    std::vector<DevBuf<uint8_t>> texture_data;
    std::vector<TextureDev>      texture_host;
    DevBuf<TextureDev>           textures;
    bool                         textures_dirty = true;
    DevBuf<float2>               bluenoise;
    bool                         bluenoise_ready = false;
    std::vector<CapMaterial>     materials_host;
    DevBuf<CapMaterial>          materials;
    // EXT: host copies needed to build the light table, the table itself, the B/A blue-noise channels
    std::vector<float>           positions_host;
    std::vector<uint32_t>        indices_host;
    std::vector<CapMeshDesc>     meshes_host;
    DevBuf<uint32_t>             light_tris;
    DevBuf<float>                light_cdf;
    DevBuf<float2>               bluenoise_ba;
    uint32_t                     light_count = 0;
    float                        light_area  = 0.0f;
    bool                         materials_ready = false;

    // BVH
    DevBuf<float4>   shade_tris, tris_sorted, nodes, tri_raw, tri_box;
    DevBuf<float4>   nodes8, tris8;           // compressed 8-wide view (cap_wide.h) and its intersection records
    DevBuf<uint32_t> wide_src;                // leaf-order index per wide-order record
    DevBuf<uint32_t> wide_task, wide_alloc, wide_cnt;   // device collapse: binary node per wide node, allocation counters, per-level bases
    uint32_t         wide8_depth = 0, wide8_top = 0, wide8_nodes = 0;
    float            wide8_ms = 0.f;
    DevBuf<uint32_t> query_work, query_defer; // cap_trace_rays / cap_trace_occlusion: chunk and hand-over counters, rays handed to the binary tree
    DevBuf<uint8_t>  tri_mask;                // cap_scene_set_instance_masks: each triangle's mesh mask, by global triangle id
    bool             tri_mask_on = false;     // a mask table is installed (some mask differs from 0xFF)
    // instance table and top-level tree (cap_instances_set, instance.hip); inst_count = 0: no table
    DevBuf<float4>   inst_desc, inst_rec, inst_box, inst_tlas;
    DevBuf<uint32_t> inst_keys[2], inst_vals[2], inst_hist, inst_scan, inst_misc, inst_level_off;
    uint32_t         inst_count = 0, inst_top = 0, inst_nodes = 0;
    DevBuf<float2>   inst_near;               // each instance's (g, Xw) for cap_closest_instances (cap_near.h)
    DevBuf<uint32_t> inst_obj;                // each instance's object index (cap_instances_set_ex)
    bool             inst_obj_on = false;     // ... given with the installed table (false: every instance shows object 0)
    InstObject       scene_object_host{};     // the scene as the one object of a context without an object table ...
    DevBuf<InstObject> scene_object;          // ... and its device copy (instances_rebuild)
    // object table and forest (cap_objects_set, instance.hip); obj_count = 0: no table.  Object k's tree: nodes
    // [obj_node_base[k], + triangle_count - 1) of forest_nodes, records [obj_rec_base[k], + triangle_count) of forest_tris.
    std::vector<CapObjectInfo> obj_info;
    std::vector<uint32_t>      obj_node_base, obj_rec_base;
    uint32_t                   obj_count = 0, obj_max_depth = 0;
    DevBuf<float4>             forest_nodes, forest_tris;
    DevBuf<InstObject>         obj_table;     // per object: padded box and root (k_instance_setup)
    DevBuf<float4>             obj_tri_raw, obj_tri_box;  // build scratch of the largest object (the builders' tri_raw / tri_box / leaf_tri)
    DevBuf<uint32_t>           obj_leaf_tri, obj_misc;    // obj_misc: 8 words per object, 6 bounds + depth
    DevBuf<float4>   fan_pairs, fan_singles;  // exhaustive path: fan-pair records (5 float4) and the unpaired triangles (4 float4)
    uint32_t         fan_pair_count = 0, fan_single_count = 0;
    DevBuf<float4>   fan_pairs_nee;           // the pair records again, potential occluders of next-event rays first (update_nee_pairs)
    uint32_t         fan_pair_nee_count = 0;
    std::vector<float>    fan_pairs_host;     // 20 floats per pair (+ padding records), as uploaded
    std::vector<uint32_t> light_tris_host;    // global ids of the emissive triangles (cap_materials_upload)
    DevBuf<uint32_t> leaf_tri, keys0, keys1, vals0, vals1, hist, parent, flags, bvh_misc;  // bvh_misc: 6 bounds + depth + 1 if a triangle's stored normals are not tame (SceneDev::shade_tame)
    DevBuf<float4>   ploc_boxes;  // CAP_BVH_BUILD_PLOC scratch (ploc.hip)
    DevBuf<uint32_t> ploc_ints;
    DevBuf<uint32_t> sahdev_words;  // CAP_BVH_BUILD_SAH_DEVICE scratch (ploc.hip)
    CapBvhInfo       bvh_info{};
    bool             shade_tame = false;  // SceneDev::shade_tame of the shading records as cap_bvh_build / cap_bvh_refit last wrote them
    bool             bvh_ready = false;
    // pseudonormal table of cap_signed_distance (cap_pseudonormals_build, pseudonormal.hip): 21 floats per triangle by global id
    DevBuf<float>        pn_table;
    bool                 pn_ready = false;  // a table exists (stale while bvh_stale; cap_bvh_build / cap_bvh_refit rebuild it)
    CapPseudonormalsInfo pn_info{};
    // dipole table of cap_winding_numbers (cap_winding_build, winding.hip): 4 float4 per inner node of the binary tree
    DevBuf<float4>       wn_table;
    bool                 wn_ready = false;  // a table exists (stale while bvh_stale; cap_bvh_build / cap_bvh_refit rebuild it)
    CapWindingInfo       wn_info{};
    DevBuf<double>       wn_root;           // N, A, M of the whole tree as the build summed them (WindingBuildArgs::root)
    // derived tables of cap_winding_instances (winding.hip), built on the stream ahead of the first query that finds them dirty and
    // freed by cap_winding_drop: per-instance (L, |det L|, sigma, s), the top-level dipoles and their binary64 sums, the forest's dipole
    // table with the objects' root sums, and the build scratch of the largest object (kept: nothing waits for the build to end)
    DevBuf<float4>       wi_inst, wi_top, wi_forest;
    DevBuf<double>       wi_top_sums, wi_obj_root, wi_reals;
    DevBuf<uint32_t>     wi_words, wi_count;
    bool                 wi_dirty = true, wi_forest_dirty = true;  // set wherever the instances, the objects, the trees or the table change
    bool                 wi_built = false;  // the derived tables exist (current unless dirty)
    // vertex updates and refit (cap_scene_update_vertices, cap_bvh_refit, refit.hip)
    bool                  bvh_stale = false;             // vertices changed since the trees were last brought up to date
    bool                  positions_host_stale = false;  // positions_host lags a device-side update (read back only when needed)
    bool                  visits_built_known = false;    // refit_visits_built holds the metric of the last build's boxes
    double                refit_visits_built = 0.0;
    std::vector<uint32_t> wide_levels;                   // level l of the 8-wide view = nodes [wide_levels[l], wide_levels[l + 1])
    DevBuf<float>         wide_boxes;                    // refit scratch: each wide node's box (6 floats)
    DevBuf<double>        refit_sums;                    // refit scratch: partial sums of the tree metric, then its two values

    // camera / screen
    CapCameraData camera{}, prev_camera{};
    bool          camera_ready = false, prev_camera_ready = false;
    ScreenDev     screen{};
    uint64_t      max_batch_paths = 0;
    SwitchTable   sw{};                    // A/B switches: environment at creation, then cap_debug_set(CAP_DEBUG_SWITCH_BASE + i)
    uint32_t      debug_capacity_div = 1;  // cap_debug_set(CAP_DEBUG_QUEUE_CAPACITY_DIV): tests of the append guard only
    uint32_t      debug_wide_depth_limit = 0;  // cap_debug_set(CAP_DEBUG_WIDE_DEPTH_LIMIT): pretend the wide kernels' stacks end here
    bool          debug_fail_lane = false;     // cap_debug_set(CAP_DEBUG_FAIL_LANE1): the second working set "cannot be allocated"
    // The smallest second working set (paths = slots x padded pixels) whose allocation has failed since the last call that can free
    // memory: cap_render does not try that size or a larger one again (every call repeated ~28 GB of hipMalloc / hipFree).
    uint64_t      lane1_failed_paths = 0;
    uint32_t      lane1_failed_bounces = 0, lane1_retry_tick = 0;
    uint32_t      lanes_last_render = 0;       // cap_debug_get(CAP_DEBUG_LANES_USED)
    uint32_t      last_class_capacity = 0;     // sub-queue capacity of the last cap_render batch (CAP_DEBUG_QUEUE_CANARY_*)
    uint32_t      tri_ids_dense = 0;           // pair_ids_dense() of the uploaded fan records (BvhDev::tri_ids_dense)
    uint32_t      last_mark_form = 0;          // launch_trace_shade()'s answer for bounce >= 1 of the last cap_render (CAP_DEBUG_MARK_FORM)
    uint32_t      last_sample_table = 0;       // 1: the last cap_render's fused launches took the sample-table form (CAP_DEBUG_SAMPLE_TABLE)
    struct LastTerms                           // the table the last batch of the last cap_render built (CAP_DEBUG_SELFTEST_SAMPLE_TABLE)
    {
        const FrameConst* frames = nullptr;    // its frame constants (a slot of frames_ring: intact until kFrameRing calls later)
        uint32_t          n_slots = 0, num_bounces = 0, lane = 0;
    } last_terms;
    uint32_t      last_camera_table = 0;       // 1: the last batch of the last cap_render ran bounce 0 from the camera-vertex table (CAP_DEBUG_CAMERA_TABLE)
    struct LastCamera                          // that table (CAP_DEBUG_SELFTEST_CAMERA_TABLE): the batch's frame constants, slots, groups and lane
    {
        const FrameConst* frames = nullptr;
        uint32_t          n_slots = 0, n_groups = 0, lane = 0;
    } last_camera;
    uint32_t      last_group_walk = 0;         // slots per jitter group if the last batch's head kernel took the group walk, 0: slot-major (CAP_DEBUG_GROUP_WALK)
    uint32_t      last_camera_reused = 0;      // 1: the last batch of the last cap_render found its lane's camera-vertex table built (CAP_DEBUG_CAMERA_TABLE_REUSED)
    // Everything a lane's camera-vertex table was built from (ctx_render.hip render_batch compares it bit for bit before it builds): what
    // camera_vertex() and stage_camera_pairs() read -- camera, screen and shard, each group's jitter, the switches behind
    // cull_camera_pairs, the scene's records by their generation and counts -- and where the table lies.  valid == false: build.
    struct CameraTableKey
    {
        bool          valid = false;
        CameraDev     cam{};
        ScreenDev     screen{};
        uint32_t      n_groups = 0, lane = 0, cull_camera_pairs = 0, tri_count = 0, fan_pair_count = 0, fan_single_count = 0, tri_ids_dense = 0;
        uint32_t      kd_untextured = 0;       // its bits
        uint32_t      jitter[kMaxFrameSlots][2] = {};  // (jitter_x, jitter_y) bits of each group's first slot, in group order
        const float4* table = nullptr;         // Lane::camera's buffer and size: a regrown buffer is another table
        size_t        table_n = 0;
        const void*   records[4] = {};         // shade_tris, tris_by_id, fan_pairs, fan_singles
        uint64_t      scene_generation = 0;
    } camera_key[2];                           // per lane
    uint64_t      scene_generation = 0;        // bumped by every entry point that can change a record the table's builder reads
    uint32_t      last_gray_entries = 0;       // 1: the last cap_render's fused launches used 32-byte extension entries (CAP_DEBUG_GRAY_ENTRIES)
    struct LastQueues                          // what the last batch of a 48-byte render left in the extension queues (CAP_DEBUG_SELFTEST_GRAY)
    {
        uint32_t num_bounces = 0, first_writer = 0, class_capacity = 0, lane = 0;  // first_writer: the first bounce that appended to a queue
        bool     valid = false;
    } last_queues;
    struct LastSky                             // the sky-plane form of the last cap_render (CAP_DEBUG_SKY_PLANE) and its last batch's plane (.._NONZERO)
    {
        uint32_t form = 0, n_slots = 0, lane = 0;
    } last_sky;
    uint32_t      last_cull_camera_pairs = 0;  // ShadeArgs::cull_camera_pairs of the last cap_render batch (CAP_DEBUG_CAMERA_CULL)
    uint32_t      traversal_mode  = CAP_TRAVERSAL_AUTO;
    uint32_t      bvh_build_mode  = CAP_BVH_BUILD_AUTO;

    // wavefront state
    DevBuf<float4>     aov_geo, aov_nd, accum, image_tmp;
    DevBuf<uint64_t>   shaded_counter;
    // A batch working set of cap_render: queues, planes, counters and a slice of traversal-stack spill, and the stream its batches
    // run on.  There are two ("two lanes"), for batches in flight beside each other: lane[0] on the context's `stream`, lane[1] on
    // `stream2` (both sized by ensure_lane).  Lane 0's spill area is the one cap_bvh_build allocates and every ray query uses.  The
    // LAST batch of a call always runs on lane 0, so everything that reads a finished frame's planes finds them there (aov_planes).
    struct Lane
    {
        hipStream_t      stream = nullptr;  // not owned: the context's `stream` (lane 0) or `stream2` (lane 1)
        DevBuf<float4>   hits, q_org[2], q_dir[2], q_thr[2], s_org, s_dir, s_con, pl_color, pl_direct, pl_albedo;
        DevBuf<float>    pl_sky;       // [frame slot][Ppad] the sky plane (Planes::sky), if the form is on; zeroed by every batch's head launch
        DevBuf<float4>   camera;       // camera vertices, two planes [jitter group][Ppad] (launch_camera_vertices), if the form is on; kept from batch to batch (camera_key)
        DevBuf<float4>   terms;        // per batch: direction-sample terms [sampling bounce][slot][4096] (ShadeArgs::sample_terms), if the form is on
        DevBuf<uint32_t> counters;     // per batch: CounterLayout
        DevBuf<uint32_t> stack_spill;  // traversal-stack entries beyond the LDS part, per thread of the persistent grid
    } lane[2];
    hipStream_t stream2 = nullptr;
    hipEvent_t  lane_ev[2] = {nullptr, nullptr}, fork_ev = nullptr, join_ev = nullptr;
    // per-frame constants of a cap_render call: a ring of device buffers fed from pinned staging, so that a call need not wait
    // for the previous one (which may still be reading its own slot)
    static constexpr int kFrameRing = 4;
    DevBuf<FrameConst> frames_ring[kFrameRing];
    FrameConst*        frames_pinned[kFrameRing] = {nullptr, nullptr, nullptr, nullptr};
    size_t             frames_pinned_n[kFrameRing] = {0, 0, 0, 0};
    hipEvent_t         frames_event[kFrameRing] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t           frames_next = 0;
    uint32_t           last_slots = 0;     // frame slots of the last batch rendered (AOV readback)
    bool               aov_valid = false;
    bool               aov_lowres = false;  // the AOV frame was rendered with CAP_RENDER_LOWRES_INDIRECT
    uint32_t           aov_frame  = 0;      // its frame_count (selects the 2x2 interleave offset)
    uint64_t           frames_accumulated = 0;

    // reconstruction chain (row-major W*H images)
    DevBuf<float4> post_in[4];  // indirect, direct, albedo, normal_depth of the frame
    DevBuf<float4> post_ihist[2], post_mhist[2], post_chist[2], post_prev_nd, post_itemp, post_temp[2], post_normals;
    uint32_t       post_w = 0, post_h = 0;
    int            post_last_dst = -1;

    // multi-GPU frame exchange (cap_comm_*): RCCL communicator, or `comm_local` when the shards of one process share a device
    void*           comm = nullptr;  // ncclComm_t
    uint32_t        comm_rank = 0, comm_size = 0;
    bool            comm_local = false;
    DevBuf<float>   comm_send, comm_gathered, comm_image;
    hipEvent_t      comm_event = nullptr;

    // statistics
    CapStats               stats{};
    std::vector<TimedSpan> spans;
    std::vector<std::array<hipEvent_t, 6>> post_marks;  // pass-boundary events of every cap_post_frame since the last sync
    std::vector<hipEvent_t> event_pool;
    std::vector<uint32_t*> pinned_pool;
    std::vector<std::pair<uint32_t*, BatchCounted>> pending;  // (pinned copy of the counters' first section, what it counted) per batch, read at sync
    uint64_t*              pinned_shaded = nullptr;
};

namespace cap
{
// The AOV frame's tile-ordered planes (what CAP_RENDER_AOV leaves for read-backs and the reconstruction chain): the last frame slot
// of the last batch.  The LAST batch of a cap_render call always runs on lane 0 (its lane is (n_batches - 1 - batch) & 1), so
// they are lane 0's planes whichever lanes the call used.
struct AovPlanes
{
    const float4 *color, *direct, *albedo;
};

// context.hip
int        sync_and_collect(CapContext* c);
hipEvent_t get_event(CapContext* c);
CameraDev  camera_dev(const CapCameraData& cd);
SceneDev   scene_dev(const CapContext* c);
BvhDev     bvh_dev(const CapContext* c, const CapContext::Lane& lane);
AovPlanes  aov_planes(const CapContext* c);
int        trace_launch(const CapContext* c, const char* fmt, ...);
void       launch_texture_footprints(hipStream_t stream, const uint32_t* src, uint4* dst, uint32_t width, uint32_t height);  // k_texture_footprints
// ctx_render.hip: cap_render and everything only it calls; it crosses the boundary through the ABI header alone, and takes from
// context.hip the helpers above, CounterLayout and the `pending` records it leaves for sync_and_collect
// ctx_scene.hip
bool pair_ids_dense(const float* pairs, uint32_t pair_count, uint32_t single_count, uint32_t tri_count);
int  upload_fan_records(CapContext* c);
int  update_nee_pairs(CapContext* c);
int  ensure_positions_host(CapContext* c);
int  upload_light_table(CapContext* c);
// ctx_query.hip
int query_state(CapContext* c, const char* what);  // CAP_ERR_STATE unless the trees are built and up to date
// ctx_bvh.hip
int  winding_instances_ensure(CapContext* c, const char* what);  // enqueues the build of cap_winding_instances' derived tables if they are dirty
void winding_instances_release(CapContext* c);                   // frees them (the stream must be idle)
}  // namespace cap
