// ctx_query.hip — the ray-query entry points (cap_trace_*) over the launchers of query.hip (scene trees; binary tree: kernels.hip
// k_query_binary) and instance.hip (instance table), and the closest-point queries (cap_closest_points, cap_signed_distance, cap_closest_points_multi, cap_closest_instances, cap_closest_instances_multi, cap_signed_distance_instances; point_query.hip), cap_sweep_spheres and cap_sweep_instances (sweep.hip), cap_overlap_boxes, cap_overlap_instances, cap_overlap_triangles and cap_overlap_triangles_instances (overlap.hip) and cap_winding_numbers and cap_winding_instances (winding.hip).  Every entry point checks in this order and touches the device only after the last
// check: ctx, flags, filter, k rules, state, n == 0 (CAP_OK), NULL pointers, ranges (query_ranges.h).
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "cap_context.h"
#include "query_ranges.h"

int cap::query_state(CapContext* c, const char* what)
{
    if (!c->bvh_ready) return fail(CAP_ERR_STATE, "%s: call cap_bvh_build first", what);
    if (c->bvh_stale) return fail(CAP_ERR_STATE, "%s: vertices changed; call cap_bvh_refit or cap_bvh_build", what);
    return CAP_OK;
}

namespace
{
static_assert(sizeof(CapRayDesc) == 2 * sizeof(float4) && sizeof(CapHit) == sizeof(float4), "query records are the kernels' float4 records");
static_assert(CAP_MULTI_MAX_K == kMultiMaxK, "the header's page limit is the kernels' largest bucket");

constexpr uint64_t kQueryRaysPerLaunch = 1ull << 24;  // rays per launch: 32-bit ray indices and chunk counters, a 64-MB hand-over list

// What every query launch shares: the tree view, the launch configuration, the wide view's hand-over bound and the launch tracer.
struct QueryRun
{
    CapContext* c;
    const char* what;
    BvhDev      bvh;
    LaunchCfg   cfg;
    float       safe;
    float       slack;  // closest-point queries: the absolute part of the pruning bound
    float       mag;    // sphere sweeps: the largest coordinate magnitude of the scene bounds, rounded up
    uint64_t    per;    // rays per launch
    TlasDev     tl;     // instanced queries (use_instance_pools): the top-level tree ...
    uint32_t    depth;  // ... and the depth of the deepest tree below it
    int traced(const char* kernel, uint64_t first, const char* note = "") const
    {
        HIP_TRY(hipGetLastError());
        return trace_launch(c, "%s %s%s rays %llu..", what, kernel, note, (unsigned long long)first);
    }
};

// wide = false: a query that walks the binary tree alone (no hand-over list)
int query_prepare(CapContext* c, const char* what, uint64_t n, QueryRun& run, bool wide = true)
{
    HIP_TRY(hipSetDevice(c->device));
    run.c = c, run.what = what;
    run.bvh          = bvh_dev(c, c->lane[0]);  // (lane 0's spill area: a render's second lane has its own, and the stream orders us behind both)
    run.bvh.wide8_ok = wide && run.bvh.wide8_ok && query8_stack_matches();
    run.per          = std::min<uint64_t>(n, kQueryRaysPerLaunch);
    if (c->query_work.n < 2 * kCounterStride || (run.bvh.wide8_ok && c->query_defer.n < run.per))
    {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (a grown buffer replaces one an earlier query may still be using)
        HIP_TRY(c->query_work.ensure(2 * kCounterStride));
        if (run.bvh.wide8_ok) HIP_TRY(c->query_defer.ensure(run.per));
    }
    run.cfg    = LaunchCfg{c->stream, (uint32_t)c->cu_count * 4u, c->bvh_info.stack_entries, (uint32_t)c->cu_count};
    run.cfg.sw = &c->sw;
    // box-test error budget of the wide view (wide_builder.cpp, query.hip): M as the build computed it
    double m = 0.0;
    for (int k = 0; k < 3; ++k)
        m = std::max({m, (double)c->bvh_info.bounds_hi[k] - (double)c->bvh_info.bounds_lo[k], std::fabs((double)c->bvh_info.bounds_lo[k]),
                      std::fabs((double)c->bvh_info.bounds_hi[k])});
    run.safe = (float)(kQuerySafeScale * m);
    run.slack = (float)((double)kClosestSlackScale * m);  // (m >= the largest |coordinate|: the bound only grows)
    run.mag   = std::nextafter((float)m, INFINITY);
    return CAP_OK;
}

// Points a prepared run at the instance table: the top-level tree, and in run.bvh the pools the instance records' roots refer to -- the
// scene's tree, or with an object table the forest (run.bvh.tris_by_id stays the scene's: the multi-hit write-out reads it)
void use_instance_pools(QueryRun& run)
{
    const CapContext* c = run.c;
    run.tl = TlasDev{c->inst_rec.p, c->inst_tlas.p, c->inst_level_off.p, c->inst_top}, run.depth = c->bvh_info.max_depth;
    if (!c->obj_count) return;
    run.bvh.nodes = c->forest_nodes.p, run.bvh.tris = c->forest_tris.p;
    run.depth = c->obj_max_depth, run.cfg.stack_entries = run.depth <= 32 ? 32 : 64;
}

// The filter of an _ex call (CapTraceOptions; NULL = the plain call).  on: the call takes the filtered kernels -- it has a cull or
// first-hit flag, or a mask table is installed (then also through the plain entry points: a mesh with mask 0 is invisible to every
// query).  With every mask 0xFF no inclusion mask rejects anything and the plain kernels answer.
struct QueryFilter
{
    bool      on = false, first_hit = false;
    RayFilter f{};
    const RayFilter* scene() const { return on ? &f : nullptr; }  // what the scene-tree launchers take: NULL = the plain kernels
};

int query_filter(CapContext* c, const char* what, const CapTraceOptions* o, bool multi, QueryFilter& out)
{
    static_assert(sizeof(CapTraceOptions) == 16, "CapTraceOptions is four words");
    const uint32_t flags = o ? o->ray_flags : 0u, mask = o ? o->instance_mask : 0u;
    const uint32_t known = CAP_RAY_FLAG_ACCEPT_FIRST_HIT | CAP_RAY_FLAG_CULL_BACK_FACING | CAP_RAY_FLAG_CULL_FRONT_FACING;
    const uint32_t cull  = flags & (CAP_RAY_FLAG_CULL_BACK_FACING | CAP_RAY_FLAG_CULL_FRONT_FACING);
    if (flags & ~known) return fail(CAP_ERR_INVALID_ARG, "%s: unknown ray_flags 0x%x", what, flags);
    if (cull == (CAP_RAY_FLAG_CULL_BACK_FACING | CAP_RAY_FLAG_CULL_FRONT_FACING))
        return fail(CAP_ERR_INVALID_ARG, "%s: CAP_RAY_FLAG_CULL_BACK_FACING and CAP_RAY_FLAG_CULL_FRONT_FACING exclude each other", what);
    if (multi && (flags & CAP_RAY_FLAG_ACCEPT_FIRST_HIT))
        return fail(CAP_ERR_INVALID_ARG, "%s: CAP_RAY_FLAG_ACCEPT_FIRST_HIT has no meaning for a multi-hit query", what);
    if (o && (o->reserved[0] || o->reserved[1])) return fail(CAP_ERR_INVALID_ARG, "%s: options->reserved must be 0", what);
    if (mask > 0xFFu) return fail(CAP_ERR_INVALID_ARG, "%s: instance_mask 0x%x exceeds 8 bits", what, mask);
    out.first_hit  = (flags & CAP_RAY_FLAG_ACCEPT_FIRST_HIT) != 0;
    out.f.cull_and = cull ? 0x80000000u : 0u;
    out.f.cull_xor = cull == CAP_RAY_FLAG_CULL_FRONT_FACING ? 0x80000000u : 0u;
    out.f.mask     = mask ? mask : 0xFFu;
    out.f.tri_mask = c->tri_mask_on ? c->tri_mask.p : nullptr;
    out.on         = cull || out.first_hit || c->tri_mask_on;
    return CAP_OK;
}

// Flags, filter and k of a multi-hit entry point.  `pages`: the arrays that hold k records per ray ("hits", "hits and instances"),
// any_page: one of them was given.
int multi_rules(CapContext* c, const char* what, uint32_t k, uint32_t flags, const CapTraceOptions* options, const char* pages, bool any_page,
                const uint32_t* counts, QueryFilter& flt)
{
    if (flags & ~(uint32_t)CAP_MULTI_CONTINUE) return fail(CAP_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (const int rc = query_filter(c, what, options, true, flt)) return rc;
    if (k > CAP_MULTI_MAX_K) return fail(CAP_ERR_INVALID_ARG, "%s: k = %u exceeds CAP_MULTI_MAX_K (%d); page with CAP_MULTI_CONTINUE", what, k, CAP_MULTI_MAX_K);
    if (k == 0 && (any_page || !counts)) return fail(CAP_ERR_INVALID_ARG, "%s: k = 0 counts only: %s must be NULL and counts given", what, pages);
    if (k == 0 && (flags & CAP_MULTI_CONTINUE)) return fail(CAP_ERR_INVALID_ARG, "%s: CAP_MULTI_CONTINUE needs k >= 1 (the cursor is slot k - 1)", what);
    return CAP_OK;
}

// A caller's array of `stride` bytes per ray; NULL: left out
QueryRange range(const char* name, const void* p, uint64_t stride, uint32_t align) { return QueryRange{name, (uintptr_t)p, stride, align, p != nullptr}; }
QueryRange ray_range(const CapRayDesc* rays) { return range("rays", rays, sizeof(CapRayDesc), 16); }

int check_ranges(const char* what, uint64_t n, std::initializer_list<QueryRange> r)
{
    char msg[256];
    return query_ranges_ok(what, n, r.begin(), r.size(), msg, sizeof(msg)) ? CAP_OK : fail(CAP_ERR_INVALID_ARG, "%s", msg);
}

template <typename T>
T* at(T* p, uint64_t i) { return p ? p + i : nullptr; }  // element i of an array the caller may have left out

// launch(q, first) for every run.per rays (or points: Record = CapPointDesc) of the call: q holds the chunk's rays, counters and hand-over bound, first is its first ray
template <typename Record, typename Launch>
int for_each_chunk(const QueryRun& run, const Record* rays, uint64_t n, Launch&& launch)
{
    for (uint64_t first = 0; first < n; first += run.per)
    {
        QueryArgs q{};
        q.rays  = reinterpret_cast<const float4*>(rays + first);
        q.n     = (uint32_t)std::min<uint64_t>(run.per, n - first);
        q.work  = run.c->query_work.p;
        q.defer = run.c->query_defer.p;
        q.safe  = run.safe;
        if (const int rc = launch(q, first)) return rc;
    }
    return CAP_OK;
}

// One chunk through the scene's trees: the 8-wide kernel and then the binary one for the rays it handed over, or the binary one alone
template <typename Wide, typename Binary>
int launch_scene_chunk(const QueryRun& run, uint64_t first, const char* wide_name, Wide&& wide, const char* binary_name, Binary&& binary)
{
    if (!run.bvh.wide8_ok)
    {
        binary(false);
        return run.traced(binary_name, first);
    }
    HIP_TRY(hipMemsetAsync(run.c->query_work.p, 0, sizeof(uint32_t) * 2 * kCounterStride, run.c->stream));
    wide();
    if (const int rc = run.traced(wide_name, first)) return rc;
    binary(true);
    return run.traced(binary_name, first, " (handed-over rays)");
}

// a chunk's page of k records per ray and its counts
MultiArgs multi_args(QueryArgs q, uint64_t first, uint32_t k, CapHit* hits, uint32_t* counts, uint32_t flags)
{
    q.out = at(hits, first * k);
    return MultiArgs{q, k, at(counts, first), (flags & CAP_MULTI_CONTINUE) ? 1u : 0u};
}

// cap_trace_rays / cap_trace_occlusion and their _ex forms (query.hip k_query_closest8 / k_query_any8, k_query_binary)
int trace_query(CapContext* c, const char* what, const CapRayDesc* rays, uint64_t n, void* out, size_t out_stride, uint32_t flags, bool any,
                const CapTraceOptions* options = nullptr)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (flags != 0) return fail(CAP_ERR_INVALID_ARG, "%s: flags is reserved and must be 0 (got 0x%x)", what, flags);
    QueryFilter flt;
    if (const int rc = query_filter(c, what, options, false, flt)) return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (n == 0) return CAP_OK;
    if (!rays || !out) return fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {ray_range(rays), range("output", out, out_stride, 16)})) return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run)) return rc;
    const bool       first_hit = flt.first_hit && !any;  // (an occlusion query ends at its first hit anyway)
    const RayFilter* f         = flt.scene();
    return for_each_chunk(run, rays, n, [&](QueryArgs q, uint64_t first) {
        q.out = static_cast<uint8_t*>(out) + first * out_stride;
        return launch_scene_chunk(
            run, first, any ? "k_query_any8" : "k_query_closest8", [&] { launch_query8(run.cfg, run.bvh, q, any, f, first_hit); },
            any ? "k_query_binary<any>" : "k_query_binary<closest>",
            [&](bool handed_over) {
                if (f)
                    launch_query_binary_filtered(run.cfg, run.bvh, q, *f, any, first_hit, handed_over);
                else
                    launch_query_binary(run.cfg, run.bvh, q, any, handed_over);
            });
    });
}

// cap_trace_rays_multi: the first k hits of each ray in (t, triangle) order, and / or its hit count (query.hip k_query_multi8,
// k_query_binary_multi).  k records per ray: their offsets are 64-bit.
int trace_multi(CapContext* c, const char* what, const CapRayDesc* rays, uint64_t n, uint32_t k, CapHit* hits, uint32_t* counts, uint32_t flags,
                const CapTraceOptions* options = nullptr)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    QueryFilter flt;
    if (const int rc = multi_rules(c, what, k, flags, options, "hits", hits != nullptr, counts, flt)) return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (n == 0) return CAP_OK;
    if (!rays || (k && !hits)) return fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {ray_range(rays), range("hits", hits, (uint64_t)k * sizeof(CapHit), 16), range("counts", counts, sizeof(uint32_t), 4)}))
        return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run)) return rc;
    const RayFilter* f = flt.scene();
    return for_each_chunk(run, rays, n, [&](const QueryArgs& q, uint64_t first) {
        const MultiArgs m = multi_args(q, first, k, hits, counts, flags);
        return launch_scene_chunk(
            run, first, "k_query_multi8", [&] { launch_query8_multi(run.cfg, run.bvh, m, f); }, "k_query_binary_multi",
            [&](bool handed_over) { launch_query_binary_multi(run.cfg, run.bvh, m, handed_over, f); });
    });
}

// cap_trace_instances / cap_trace_instances_occlusion (instance.hip k_query_inst)
int trace_instances(CapContext* c, const char* what, const CapRayDesc* rays, uint64_t n, void* out, size_t out_stride, uint32_t* inst, bool any,
                    const CapTraceOptions* options)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    QueryFilter flt;
    if (const int rc = query_filter(c, what, options, false, flt)) return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    if (n == 0) return CAP_OK;
    if (!rays || !out) return fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {ray_range(rays), range("output", out, out_stride, 16), range("instances", inst, sizeof(uint32_t), 4)})) return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run)) return rc;
    use_instance_pools(run);
    const int mode = any ? 2 : flt.first_hit ? 1 : 0;
    return for_each_chunk(run, rays, n, [&](QueryArgs q, uint64_t first) {
        q.out = static_cast<uint8_t*>(out) + first * out_stride;
        launch_query_instances(run.cfg, run.bvh, q, run.tl, flt.f, mode, at(inst, first), run.depth);
        return run.traced(any ? "k_query_inst<any>" : "k_query_inst<closest>", first);
    });
}

// cap_trace_instances_multi: the first k pairs of each ray in (t, instance, triangle) order and / or the number of its pairs
// (instance.hip k_query_inst_multi): trace_multi with the instance page as a fourth array, over trace_instances' state and pools
int trace_instances_multi(CapContext* c, const char* what, const CapRayDesc* rays, uint64_t n, uint32_t k, CapHit* hits, uint32_t* inst,
                          uint32_t* counts, uint32_t flags, const CapTraceOptions* options)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    QueryFilter flt;
    if (const int rc = multi_rules(c, what, k, flags, options, "hits and instances", hits || inst, counts, flt)) return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    if (n == 0) return CAP_OK;
    if (!rays || (k && (!hits || !inst))) return fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer (k = %u needs hits and instances)", what, k);
    if (const int rc = check_ranges(what, n, {ray_range(rays), range("hits", hits, (uint64_t)k * sizeof(CapHit), 16),
                                              range("instances", inst, (uint64_t)k * sizeof(uint32_t), 4), range("counts", counts, sizeof(uint32_t), 4)}))
        return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run)) return rc;
    use_instance_pools(run);
    return for_each_chunk(run, rays, n, [&](const QueryArgs& q, uint64_t first) {
        launch_query_instances_multi(run.cfg, run.bvh, multi_args(q, first, k, hits, counts, flags), run.tl, flt.f, at(inst, first * k), run.depth);
        return run.traced("k_query_inst_multi", first);
    });
}

// What one of the six closest-point entry points is, beside the points and the record array every one of them has: its further arrays
// and its page rules.  One record per point (k = 1) unless multi.
struct PointCall
{
    bool      with_sign  = false;    // cap_signed_distance*: the pseudonormal table is part of the state ...
    float*    signed_out = nullptr;  // ... and the signed array a third range
    bool      instanced  = false;    // cap_closest_instances*: trace_instances' state and pools ...
    uint32_t* inst       = nullptr;  // ... and the instance array, one entry per record (may be left out unless multi)
    bool      multi      = false;    // cap_closest_*_multi: trace_multi's rules on k, counts and flags
    uint32_t  k          = 1;
    uint32_t* counts     = nullptr;
    uint32_t  flags      = 0;
};
PointCall with_sign(float* signed_out)
{
    PointCall q;
    q.with_sign = true, q.signed_out = signed_out;
    return q;
}
PointCall over_instances(uint32_t* inst, PointCall q = PointCall{})
{
    q.instanced = true, q.inst = inst;
    return q;
}
PointCall paged(PointCall q, uint32_t k, uint32_t* counts, uint32_t flags)
{
    q.multi = true, q.k = k, q.counts = counts, q.flags = flags;
    return q;
}

// The closest-point queries (point_query.hip): the binary tree alone, or with q.instanced the object trees under the instance table.
// A multi call with k = 1, no counts and no cursor IS the single query and takes its kernel.
int closest_query(CapContext* c, const char* what, const CapPointDesc* points, uint64_t n, CapClosest* out, const PointCall& q, const CapTraceOptions* options)
{
    static_assert(sizeof(CapPointDesc) == sizeof(float4) && sizeof(CapClosest) == 2 * sizeof(float4), "point records are the kernel's float4 records");
    const bool pairs = q.instanced && q.multi;  // a page of instances belongs to the page of records
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (options && options->ray_flags) return fail(CAP_ERR_INVALID_ARG, "%s: ray_flags 0x%x: facing and first hit have no meaning for a point", what, options->ray_flags);
    QueryFilter flt;
    if (const int rc = q.multi ? multi_rules(c, what, q.k, q.flags, options, pairs ? "output and instances" : "output", out || (pairs && q.inst), q.counts, flt)
                               : query_filter(c, what, options, false, flt))
        return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (q.with_sign && !c->pn_ready) return fail(CAP_ERR_STATE, "%s: call cap_pseudonormals_build first", what);
    if (q.instanced && c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    if (n == 0) return CAP_OK;
    if (!points || (q.k && !out) || (q.k && pairs && !q.inst) || (q.with_sign && !q.signed_out))
        return pairs ? fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer (k = %u needs output and instances)", what, q.k) : fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {range("points", points, sizeof(CapPointDesc), 16), range("output", out, (uint64_t)q.k * sizeof(CapClosest), 16),
                                              range("signed", q.signed_out, sizeof(float), 4), range("instances", q.inst, (uint64_t)q.k * sizeof(uint32_t), 4),
                                              range("counts", q.counts, sizeof(uint32_t), 4)}))
        return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run, false)) return rc;
    if (q.instanced) use_instance_pools(run);
    const RayFilter* f      = flt.scene();
    const uint32_t   resume = (q.flags & CAP_MULTI_CONTINUE) ? 1u : 0u;
    const bool       single = q.k == 1 && !q.counts && !resume;
    return for_each_chunk(run, points, n, [&](const QueryArgs& chunk, uint64_t first) {
        // (the instanced kernels take their slack per point and instance: cap_near.h; the signed one's object-space walk takes the scene's)
        const ClosestArgs a{chunk.rays, chunk.n, reinterpret_cast<float4*>(at(out, first * q.k)), q.instanced && !q.with_sign ? 0.f : run.slack};
        uint32_t* const   counts = at(q.counts, first);
        if (!q.instanced)
        {
            if (q.with_sign)
            {
                launch_signed_distance(run.cfg, run.bvh, a, SignedArgs{c->pn_table.p, q.signed_out + first}, f, c->bvh_info.max_depth);
                return run.traced("k_closest_points<signed>", first);
            }
            if (single)
            {
                launch_closest_points(run.cfg, run.bvh, a, f, c->bvh_info.max_depth);
                return run.traced("k_closest_points", first);
            }
            launch_closest_points_multi(run.cfg, run.bvh, ClosestMultiArgs{a, q.k, counts, resume}, f, c->bvh_info.max_depth);
            return run.traced("k_closest_points_multi", first);
        }
        const ClosestInstArgs ia{a, at(q.inst, first * q.k), c->inst_desc.p, c->inst_near.p, c->inst_misc.p + 7};
        if (q.with_sign)
        {
            launch_signed_distance_instances(run.cfg, run.bvh, ia, SignedArgs{c->pn_table.p, q.signed_out + first}, run.tl, flt.f, run.depth);
            return run.traced("k_closest_inst<signed>", first);
        }
        if (single)
        {
            launch_closest_instances(run.cfg, run.bvh, ia, run.tl, flt.f, run.depth);
            return run.traced("k_closest_inst", first);
        }
        launch_closest_instances_multi(run.cfg, run.bvh, ClosestInstMultiArgs{ia, q.k, counts, resume}, run.tl, flt.f, run.depth);
        return run.traced("k_closest_inst_multi", first);
    });
}

// cap_sweep_spheres (sweep.hip k_sweep_spheres): the first contact of each moving sphere with the scene, on the binary tree alone;
// with `instanced` cap_sweep_instances (k_sweep_inst): world-space sweeps over the instance table, `inst` the instance of each record
// (may be left out).  cap_closest_points' and cap_closest_instances' checks, with "sweeps", "hits" and "instances" as the arrays' names.
int sweep_query(CapContext* c, const char* what, const CapSweepDesc* sweeps, uint64_t n, CapSweepHit* out, uint32_t* inst, bool instanced,
                const CapTraceOptions* options)
{
    static_assert(sizeof(CapSweepDesc) == 2 * sizeof(float4) && sizeof(CapSweepHit) == 2 * sizeof(float4), "sweep records are the kernel's float4 records");
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (options && options->ray_flags) return fail(CAP_ERR_INVALID_ARG, "%s: ray_flags 0x%x: a sweep is two-sided and has one first contact", what, options->ray_flags);
    QueryFilter flt;
    if (const int rc = query_filter(c, what, options, false, flt)) return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (instanced && c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    if (n == 0) return CAP_OK;
    if (!sweeps || !out) return fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {range("sweeps", sweeps, sizeof(CapSweepDesc), 16), range("hits", out, sizeof(CapSweepHit), 16),
                                              range("instances", inst, sizeof(uint32_t), 4)}))
        return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run, false)) return rc;
    if (instanced) use_instance_pools(run);
    const RayFilter* f = flt.scene();
    return for_each_chunk(run, sweeps, n, [&](const QueryArgs& chunk, uint64_t first) {
        // (the instanced kernel takes its prune radius per sweep and instance: cap_near.h)
        const SweepArgs a{chunk.rays, chunk.n, reinterpret_cast<float4*>(out + first), instanced ? 0.f : run.mag};
        if (!instanced)
        {
            launch_sweep_spheres(run.cfg, run.bvh, a, f, c->bvh_info.max_depth);
            return run.traced("k_sweep_spheres", first);
        }
        launch_sweep_instances(run.cfg, run.bvh, SweepInstArgs{a, at(inst, first), c->inst_desc.p, c->inst_near.p, c->inst_misc.p + 7}, run.tl, flt.f, run.depth);
        return run.traced("k_sweep_inst", first);
    });
}

// cap_overlap_boxes (overlap.hip k_overlap_boxes): the triangles that meet each box, pages of k ids and / or counts, on the binary tree
// alone; with `instanced` cap_overlap_instances (k_overlap_inst): world-space boxes over the instance table, pages of k (triangle,
// instance) pairs; with Record = CapTriangleDesc cap_overlap_triangles (k_overlap_triangles): the triangles that meet each query
// triangle, and with both cap_overlap_triangles_instances (k_overlap_tri_inst): world-space query triangles over the instance table.
// closest_query's checks for a multi call, word for word, with "boxes" (or "queries"), "triangles" and "instances" as the
// arrays' names.
template <typename Record>
int overlap_query(CapContext* c, const char* what, const Record* queries, uint64_t n, uint32_t k, uint32_t* ids, uint32_t* inst, bool instanced,
                  uint32_t* counts, uint32_t flags, const CapTraceOptions* options)
{
    constexpr bool tri = std::is_same<Record, CapTriangleDesc>::value;
    static_assert(sizeof(CapBoxDesc) == 2 * sizeof(float4), "a box record is the kernel's two float4");
    static_assert(sizeof(CapTriangleDesc) == 3 * sizeof(float4), "a triangle record is the kernel's three float4");
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (options && options->ray_flags)
        return fail(CAP_ERR_INVALID_ARG, "%s: ray_flags 0x%x: facing and first hit have no meaning for a %s", what, options->ray_flags, tri ? "triangle" : "box");
    QueryFilter flt;
    if (const int rc = multi_rules(c, what, k, flags, options, instanced ? "triangles and instances" : "triangles", ids || (instanced && inst), counts, flt))
        return rc;
    if (const int rc = query_state(c, what)) return rc;
    if (instanced && c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    if (n == 0) return CAP_OK;
    if (!queries || (k && !ids) || (k && instanced && !inst))
        return instanced ? fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer (k = %u needs triangles and instances)", what, k)
                         : fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {range(tri ? "queries" : "boxes", queries, sizeof(Record), 16), range("triangles", ids, (uint64_t)k * sizeof(uint32_t), 4),
                                              range("instances", inst, (uint64_t)k * sizeof(uint32_t), 4), range("counts", counts, sizeof(uint32_t), 4)}))
        return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run, false)) return rc;
    if (instanced) use_instance_pools(run);
    const RayFilter* f      = flt.scene();
    const uint32_t   resume = (flags & CAP_MULTI_CONTINUE) ? 1u : 0u;
    return for_each_chunk(run, queries, n, [&](const QueryArgs& chunk, uint64_t first) {
        if constexpr (tri)
        {
            // (the instanced kernel takes its slack per query and instance: cap_near.h)
            const OverlapTriArgs a{chunk.rays, chunk.n, at(ids, first * k), k, at(counts, first), resume, instanced ? 0.f : run.slack};
            if (!instanced)
            {
                launch_overlap_triangles(run.cfg, run.bvh, a, f, c->bvh_info.max_depth);
                return run.traced("k_overlap_triangles", first);
            }
            launch_overlap_triangles_instances(run.cfg, run.bvh, OverlapTriInstArgs{a, at(inst, first * k), c->inst_desc.p, c->inst_near.p, c->inst_misc.p + 7},
                                               run.tl, flt.f, run.depth);
            return run.traced("k_overlap_tri_inst", first);
        }
        // (the instanced kernel takes its slack per box and instance: cap_near.h)
        const OverlapArgs a{chunk.rays, chunk.n, at(ids, first * k), k, at(counts, first), resume, instanced ? 0.f : run.slack};
        if (!instanced)
        {
            launch_overlap_boxes(run.cfg, run.bvh, a, f, c->bvh_info.max_depth);
            return run.traced("k_overlap_boxes", first);
        }
        launch_overlap_instances(run.cfg, run.bvh, OverlapInstArgs{a, at(inst, first * k), c->inst_desc.p, c->inst_near.p, c->inst_misc.p + 7}, run.tl, flt.f,
                                 run.depth);
        return run.traced("k_overlap_inst", first);
    });
}

// cap_winding_numbers (winding.hip k_winding: the walk of the binary tree over the dipole table) and, with `instanced`,
// cap_winding_instances (k_winding_inst: the two-level walk over the top-level dipoles and the objects' tables; four visit words per point
// instead of two).  No options: the moments cover every triangle, so there is no filter to check.  The derived tables of the instanced
// form are brought up to date on the stream after the last check, ahead of the first launch.
int winding_query(CapContext* c, const char* what, const CapPointDesc* points, uint64_t n, float beta, float* winding, uint32_t* visits, bool instanced)
{
    const uint32_t vw = instanced ? 4u : 2u;
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (!(beta >= 1.0f)) return fail(CAP_ERR_INVALID_ARG, "%s: beta = %g must be finite and >= 1, or +inf", what, (double)beta);  // (a NaN fails the comparison)
    if (const int rc = query_state(c, what)) return rc;
    if (!c->wn_ready) return fail(CAP_ERR_STATE, "%s: call cap_winding_build first", what);
    if (instanced && c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    if (n == 0) return CAP_OK;
    if (!points || !winding) return fail(CAP_ERR_INVALID_ARG, "%s: NULL device pointer", what);
    if (const int rc = check_ranges(what, n, {range("points", points, sizeof(CapPointDesc), 16), range("winding", winding, sizeof(float), 4),
                                              range("visits", visits, vw * sizeof(uint32_t), 4)}))
        return rc;
    QueryRun run;
    if (const int rc = query_prepare(c, what, n, run, false)) return rc;
    if (instanced)
    {
        if (const int rc = winding_instances_ensure(c, what)) return rc;
        use_instance_pools(run);
    }
    const float4* table = instanced && c->obj_count ? c->wi_forest.p : c->wn_table.p;
    return for_each_chunk(run, points, n, [&](const QueryArgs& chunk, uint64_t first) {
        const WindingArgs a{chunk.rays, chunk.n, table, beta, winding + first, at(visits, vw * first)};
        if (!instanced)
        {
            launch_winding_numbers(run.cfg, run.bvh, a, c->bvh_info.max_depth);
            return run.traced("k_winding", first);
        }
        launch_winding_instances(run.cfg, run.bvh, WindingInstArgs{a, c->wi_inst.p, c->wi_top.p}, run.tl, run.depth);
        return run.traced("k_winding_inst", first);
    });
}
}  // namespace

extern "C" {

int cap_sweep_spheres(CapContext* c, const CapSweepDesc* device_sweeps, uint64_t n, CapSweepHit* device_out, const CapTraceOptions* options)
{
    return sweep_query(c, "cap_sweep_spheres", device_sweeps, n, device_out, nullptr, false, options);
}

int cap_sweep_instances(CapContext* c, const CapSweepDesc* device_sweeps, uint64_t n, CapSweepHit* device_out, uint32_t* device_instances,
                        const CapTraceOptions* options)
{
    return sweep_query(c, "cap_sweep_instances", device_sweeps, n, device_out, device_instances, true, options);
}

int cap_overlap_boxes(CapContext* c, const CapBoxDesc* device_boxes, uint64_t n, uint32_t k, uint32_t* device_triangles, uint32_t* device_counts,
                      uint32_t multi_flags, const CapTraceOptions* options)
{
    return overlap_query(c, "cap_overlap_boxes", device_boxes, n, k, device_triangles, nullptr, false, device_counts, multi_flags, options);
}

int cap_overlap_instances(CapContext* c, const CapBoxDesc* device_boxes, uint64_t n, uint32_t k, uint32_t* device_triangles, uint32_t* device_instances,
                          uint32_t* device_counts, uint32_t multi_flags, const CapTraceOptions* options)
{
    return overlap_query(c, "cap_overlap_instances", device_boxes, n, k, device_triangles, device_instances, true, device_counts, multi_flags, options);
}

int cap_overlap_triangles(CapContext* c, const CapTriangleDesc* device_queries, uint64_t n, uint32_t k, uint32_t* device_triangles, uint32_t* device_counts,
                          uint32_t multi_flags, const CapTraceOptions* options)
{
    return overlap_query(c, "cap_overlap_triangles", device_queries, n, k, device_triangles, nullptr, false, device_counts, multi_flags, options);
}

int cap_overlap_triangles_instances(CapContext* c, const CapTriangleDesc* device_queries, uint64_t n, uint32_t k, uint32_t* device_triangles,
                                    uint32_t* device_instances, uint32_t* device_counts, uint32_t multi_flags, const CapTraceOptions* options)
{
    return overlap_query(c, "cap_overlap_triangles_instances", device_queries, n, k, device_triangles, device_instances, true, device_counts, multi_flags,
                         options);
}

int cap_winding_instances(CapContext* c, const CapPointDesc* device_points, uint64_t n, float beta, float* device_winding, uint32_t* device_visits)
{
    return winding_query(c, "cap_winding_instances", device_points, n, beta, device_winding, device_visits, true);
}

int cap_winding_numbers(CapContext* c, const CapPointDesc* device_points, uint64_t n, float beta, float* device_winding, uint32_t* device_visits)
{
    return winding_query(c, "cap_winding_numbers", device_points, n, beta, device_winding, device_visits, false);
}

int cap_trace_rays(CapContext* c, const CapRayDesc* device_rays, uint64_t n, CapHit* device_hits, uint32_t flags)
{
    return trace_query(c, "cap_trace_rays", device_rays, n, device_hits, sizeof(CapHit), flags, false);
}

int cap_trace_occlusion(CapContext* c, const CapRayDesc* device_rays, uint64_t n, uint32_t* device_occluded, uint32_t flags)
{
    return trace_query(c, "cap_trace_occlusion", device_rays, n, device_occluded, sizeof(uint32_t), flags, true);
}

int cap_trace_rays_multi(CapContext* c, const CapRayDesc* device_rays, uint64_t n, uint32_t k, CapHit* device_hits, uint32_t* device_counts,
                         uint32_t flags)
{
    return trace_multi(c, "cap_trace_rays_multi", device_rays, n, k, device_hits, device_counts, flags);
}

int cap_trace_rays_ex(CapContext* c, const CapRayDesc* device_rays, uint64_t n, CapHit* device_hits, const CapTraceOptions* options)
{
    return trace_query(c, "cap_trace_rays_ex", device_rays, n, device_hits, sizeof(CapHit), 0, false, options);
}

int cap_trace_occlusion_ex(CapContext* c, const CapRayDesc* device_rays, uint64_t n, uint32_t* device_occluded, const CapTraceOptions* options)
{
    return trace_query(c, "cap_trace_occlusion_ex", device_rays, n, device_occluded, sizeof(uint32_t), 0, true, options);
}

int cap_trace_rays_multi_ex(CapContext* c, const CapRayDesc* device_rays, uint64_t n, uint32_t k, CapHit* device_hits, uint32_t* device_counts,
                            uint32_t multi_flags, const CapTraceOptions* options)
{
    return trace_multi(c, "cap_trace_rays_multi_ex", device_rays, n, k, device_hits, device_counts, multi_flags, options);
}

int cap_trace_instances(CapContext* c, const CapRayDesc* device_rays, uint64_t n, CapHit* device_hits, uint32_t* device_instances,
                        const CapTraceOptions* options)
{
    return trace_instances(c, "cap_trace_instances", device_rays, n, device_hits, sizeof(CapHit), device_instances, false, options);
}

int cap_trace_instances_occlusion(CapContext* c, const CapRayDesc* device_rays, uint64_t n, uint32_t* device_occluded, const CapTraceOptions* options)
{
    return trace_instances(c, "cap_trace_instances_occlusion", device_rays, n, device_occluded, sizeof(uint32_t), nullptr, true, options);
}

int cap_trace_instances_multi(CapContext* c, const CapRayDesc* device_rays, uint64_t n, uint32_t k, CapHit* device_hits, uint32_t* device_instances,
                              uint32_t* device_counts, uint32_t flags, const CapTraceOptions* options)
{
    return trace_instances_multi(c, "cap_trace_instances_multi", device_rays, n, k, device_hits, device_instances, device_counts, flags, options);
}

int cap_closest_points(CapContext* c, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out, const CapTraceOptions* options)
{
    return closest_query(c, "cap_closest_points", device_points, n, device_out, PointCall{}, options);
}

int cap_signed_distance(CapContext* c, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out, float* device_signed,
                        const CapTraceOptions* options)
{
    return closest_query(c, "cap_signed_distance", device_points, n, device_out, with_sign(device_signed), options);
}

int cap_closest_points_multi(CapContext* c, const CapPointDesc* device_points, uint64_t n, uint32_t k, CapClosest* device_out, uint32_t* device_counts,
                             uint32_t multi_flags, const CapTraceOptions* options)
{
    return closest_query(c, "cap_closest_points_multi", device_points, n, device_out, paged(PointCall{}, k, device_counts, multi_flags), options);
}

int cap_closest_instances(CapContext* c, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out, uint32_t* device_instances,
                          const CapTraceOptions* options)
{
    return closest_query(c, "cap_closest_instances", device_points, n, device_out, over_instances(device_instances), options);
}

int cap_signed_distance_instances(CapContext* c, const CapPointDesc* device_points, uint64_t n, CapClosest* device_out, uint32_t* device_instances,
                                  float* device_signed, const CapTraceOptions* options)
{
    return closest_query(c, "cap_signed_distance_instances", device_points, n, device_out, over_instances(device_instances, with_sign(device_signed)), options);
}

int cap_closest_instances_multi(CapContext* c, const CapPointDesc* device_points, uint64_t n, uint32_t k, CapClosest* device_out,
                                uint32_t* device_instances, uint32_t* device_counts, uint32_t multi_flags, const CapTraceOptions* options)
{
    return closest_query(c, "cap_closest_instances_multi", device_points, n, device_out, paged(over_instances(device_instances), k, device_counts, multi_flags),
                         options);
}
}  // extern "C"
