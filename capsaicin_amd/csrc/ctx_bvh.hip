// ctx_bvh.hip — the trees of a context: cap_bvh_build, vertex updates and cap_bvh_refit, the object forest (cap_objects_set) and the
// instance table with its top-level tree (cap_instances_set); launchers in bvh.hip, ploc.hip, refit.hip, instance.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "cap_context.h"
#include "sah_builder.h"
#include "wide_builder.h"
#include "cap_wide.h"

// AUTO builds with surface-area splits (ploc.hip, sah_device) from this many triangles on, the clustering alone below (see cap_bvh_build)
constexpr uint32_t kAutoSahTriangles = 4096;

// the build's (and the refit's) view of the context's scene and tree buffers
static BvhBuildArgs bvh_args(const CapContext* c)
{
    BvhBuildArgs a{};
    a.positions = c->positions.p, a.normals = c->normals.p, a.texcoords = c->texcoords.p, a.indices = c->indices.p;
    a.tri_ids = c->tri_ids.p, a.mesh_offsets = c->mesh_offsets.p, a.tri_count = c->tri_count;
    a.shade_tris = c->shade_tris.p, a.tris_sorted = c->tris_sorted.p, a.nodes = c->nodes.p, a.leaf_tri = c->leaf_tri.p;
    a.tri_raw = c->tri_raw.p, a.tri_box = c->tri_box.p;
    a.keys[0] = c->keys0.p, a.keys[1] = c->keys1.p, a.vals[0] = c->vals0.p, a.vals[1] = c->vals1.p;
    a.hist = c->hist.p, a.parent = c->parent.p, a.flags = c->flags.p, a.bounds = c->bvh_misc.p, a.max_depth = c->bvh_misc.p + 6;
    return a;
}

// CapBvhInfo::bounds_lo / hi from the six ordered-uint words k_tri_setup reduced into bvh_misc
static void set_bounds(CapBvhInfo& bi, const uint32_t misc[6])
{
    auto dec = [](uint32_t o) {
        uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
        float    f;
        memcpy(&f, &u, 4);
        return f;
    };
    for (int k = 0; k < 3; ++k) bi.bounds_lo[k] = dec(misc[k]), bi.bounds_hi[k] = dec(misc[3 + k]);
}

// the 8-wide view's child-box padding, kWidePad * max(scene extent, largest |coordinate|) (wide_builder.cpp: its error budget)
static double wide_pad(const CapBvhInfo& bi)
{
    double m = 0.0;
    for (int k = 0; k < 3; ++k)
        m = std::max({m, (double)bi.bounds_hi[k] - (double)bi.bounds_lo[k], std::fabs((double)bi.bounds_lo[k]), std::fabs((double)bi.bounds_hi[k])});
    return (double)kWidePad * std::max(m, 1e-30);
}

// The object box of k_instance_setup: every point the triangle test can report lies in a leaf box, the triangle's box padded by
// 1e-5 max(1, |coordinate|) (bvh.hip k_refit); twice that around the bounds, in double
static InstObject object_box(const float lo3[3], const float hi3[3], int32_t root)
{
    InstObject o{};
    for (int k = 0; k < 3; ++k)
    {
        const double lo = lo3[k], hi = hi3[k];
        const double pad = 2e-5 * std::max(1.0, std::max(std::fabs(lo), std::fabs(hi)));
        o.blo[k] = lo - pad, o.bhi[k] = hi + pad;
    }
    o.root = root;
    return o;
}

// The builder cap_bvh_build takes for n triangles under the context's mode; for an object, the host builder is replaced by its
// device counterpart (include/capsaicin_hip.h cap_objects_set)
static uint32_t object_builder(const CapContext* c, uint32_t n)
{
    const uint32_t mode = c->bvh_build_mode;
    if (n >= 2 && (mode == CAP_BVH_BUILD_SAH || mode == CAP_BVH_BUILD_SAH_DEVICE ||
                   (mode == CAP_BVH_BUILD_AUTO && n >= (uint32_t)c->sw.get(SW_AUTO_SAH_TRIANGLES, kAutoSahTriangles))))
        return CAP_BVH_BUILD_SAH_DEVICE;
    if (n >= 2 && (mode == CAP_BVH_BUILD_PLOC || (mode == CAP_BVH_BUILD_AUTO && n > kExhaustiveMax))) return CAP_BVH_BUILD_PLOC;
    return CAP_BVH_BUILD_LBVH;
}

// The forest of the installed object table from the current vertices: what cap_objects_set, cap_bvh_build and cap_bvh_refit share.
// Each object's tree is built by the scene's builders on the object's triangle range (offset pointers; the scene's build scratch,
// which no kept structure lives in, and the forest's own tri_raw / tri_box / leaf_tri so that the scene's stay as they are) straight
// into its place in the pools, then relocated in place (instance.hip).  The shading records the triangle setup rewrites get the
// values they hold.  Waits for the stream: depths and bounds are read back.  Nothing when no table is installed; a failure drops it.
static int objects_rebuild(CapContext* c, const char* what)
{
    const uint32_t count = c->obj_count;
    c->wi_dirty = c->wi_forest_dirty = true;  // cap_winding_instances' derived tables follow the forest
    if (count == 0) return CAP_OK;
    c->obj_count = 0;  // (until the forest stands)
    uint32_t max_n = 0;
    for (const CapObjectInfo& o : c->obj_info) max_n = std::max(max_n, o.triangle_count);
    const int radius = (int)c->sw.get(SW_PLOC_RADIUS, 16), leaf = (int)c->sw.get(SW_SAHDEV_LEAF, 32);
    DevBuf<uint32_t> sahdev;  // the surface-area builder's scratch, of no use after the build
    for (uint32_t k = 0; k < count; ++k)
    {
        CapObjectInfo& o = c->obj_info[k];
        const uint32_t n = o.triangle_count, first = o.first_triangle;
        o.builder        = object_builder(c, n);
        BvhBuildArgs a   = bvh_args(c);
        a.tri_ids = c->tri_ids.p + first, a.tri_count = n;
        a.shade_tris  = c->shade_tris.p + kShadeRec * (size_t)first;
        a.tris_sorted = c->forest_tris.p + 4 * (size_t)c->obj_rec_base[k], a.nodes = c->forest_nodes.p + 4 * (size_t)c->obj_node_base[k];
        a.leaf_tri = c->obj_leaf_tri.p, a.tri_raw = c->obj_tri_raw.p, a.tri_box = c->obj_tri_box.p;
        a.bounds = c->obj_misc.p + 8 * (size_t)k, a.max_depth = a.bounds + 6;
        int rc = 0;
        if (o.builder == CAP_BVH_BUILD_LBVH)
            launch_bvh_build(c->stream, a);
        else
        {
            HIP_TRY(c->ploc_boxes.ensure(4 * (size_t)max_n));
            HIP_TRY(c->ploc_ints.ensure(3 * (size_t)max_n + 4));
            const PlocScratch ps{c->ploc_boxes.p, c->ploc_ints.p};
            if (o.builder == CAP_BVH_BUILD_SAH_DEVICE)
            {
                HIP_TRY(sahdev.ensure(bvh_sah_device_scratch_words(max_n)));
                rc = launch_bvh_build_sah_device(c->stream, a, ps, sahdev.p, (uint32_t)radius, (uint32_t)(leaf < 1 ? 1 : leaf));
            }
            else
                rc = launch_bvh_build_ploc(c->stream, a, ps, (uint32_t)radius);
        }
        if (rc != 0) return fail(CAP_ERR_HIP, "%s: device build of object %u failed (%d)", what, k, rc);
        launch_forest_relocate(c->stream, ForestRelocArgs{a.nodes, a.tris_sorted, n, c->obj_node_base[k], c->obj_rec_base[k], first});
        HIP_TRY(hipGetLastError());
    }
    std::vector<uint32_t> misc(8 * (size_t)count);
    HIP_TRY(hipMemcpyAsync(misc.data(), c->obj_misc.p, sizeof(uint32_t) * misc.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<InstObject> table(count);
    uint32_t depth = 0;
    for (uint32_t k = 0; k < count; ++k)
    {
        CapObjectInfo& o = c->obj_info[k];
        CapBvhInfo     b{};
        set_bounds(b, misc.data() + 8 * (size_t)k);
        for (int j = 0; j < 3; ++j) o.bounds_lo[j] = b.bounds_lo[j], o.bounds_hi[j] = b.bounds_hi[j];
        o.max_depth = misc[8 * (size_t)k + 6];
        depth       = std::max(depth, o.max_depth);
        // a one-triangle object has no node: its root is the leaf code of its record
        table[k] = object_box(o.bounds_lo, o.bounds_hi, o.triangle_count >= 2 ? (int32_t)c->obj_node_base[k] : (int32_t)~c->obj_rec_base[k]);
    }
    if (depth > 64) return fail(CAP_ERR_UNSUPPORTED, "%s: object tree depth %u exceeds the 64-entry traversal stack", what, depth);
    HIP_TRY(hipMemcpy(c->obj_table.p, table.data(), sizeof(InstObject) * count, hipMemcpyHostToDevice));
    c->obj_count = count, c->obj_max_depth = depth;
    return CAP_OK;
}

// World boxes and top-level tree of the installed instance table from the kept descriptors and the current bounds: what
// cap_instances_set, cap_bvh_build and cap_bvh_refit share.  Enqueues on the context stream; nothing when no table is installed.
static int instances_rebuild(CapContext* c)
{
    const uint32_t n = c->inst_count;
    c->wi_dirty      = true;  // cap_winding_instances' derived tables follow the instance table (a flag: nothing is built here)
    if (n == 0) return CAP_OK;
    InstanceBuildArgs a{};
    a.descs = reinterpret_cast<const float*>(c->inst_desc.p), a.n = n;
    if (c->obj_count)
        a.objects = c->obj_table.p, a.n_objects = c->obj_count;
    else
    {
        // no object table: the one object is the scene, its tree the scene's
        c->scene_object_host = object_box(c->bvh_info.bounds_lo, c->bvh_info.bounds_hi, c->tri_count >= 2 ? 0 : ~0);
        HIP_TRY(c->scene_object.ensure(1));
        HIP_TRY(hipMemcpyAsync(c->scene_object.p, &c->scene_object_host, sizeof(InstObject), hipMemcpyHostToDevice, c->stream));
        a.objects = c->scene_object.p, a.n_objects = 1;
    }
    a.object_index = c->inst_obj_on ? c->inst_obj.p : nullptr;
    a.rec = c->inst_rec.p, a.box = c->inst_box.p, a.tlas = c->inst_tlas.p, a.near = c->inst_near.p;
    a.keys[0] = c->inst_keys[0].p, a.keys[1] = c->inst_keys[1].p, a.vals[0] = c->inst_vals[0].p, a.vals[1] = c->inst_vals[1].p;
    a.hist = c->inst_hist.p, a.scan = c->inst_scan.p, a.misc = c->inst_misc.p;
    launch_instances_build(c->stream, a);
    HIP_TRY(hipGetLastError());
    return CAP_OK;
}

// The pseudonormal table from the current vertices (pseudonormal.hip): what cap_pseudonormals_build, cap_bvh_build and cap_bvh_refit
// share.  The scratch is the build's own -- the tree builders' buffers are sized by triangles, these by corners -- and goes when the
// call returns.  Waits for the stream: the statistics are read back.  A failure drops the table.
static int pseudonormals_rebuild(CapContext* c, const char* what)
{
    c->pn_ready = false;  // (until the table stands)
    const uint32_t t = c->tri_count;
    if (3ull * t >= (1ull << 32)) return fail(CAP_ERR_UNSUPPORTED, "%s: %u triangles have more than 2^32 - 1 corners", what, t);
    const auto     wall0 = std::chrono::steady_clock::now();
    const uint32_t n     = 3u * t;
    uint32_t       stats[8] = {0};
    if (t)
    {
        if (c->pn_table.n < 21 * (size_t)t)
        {
            HIP_TRY(hipStreamSynchronize(c->stream));  // (a grown table replaces one an earlier query may still be reading)
            HIP_TRY(c->pn_table.ensure(21 * (size_t)t));
        }
        DevBuf<uint32_t> words, hist, scan, st;
        DevBuf<double>   reals;
        HIP_TRY(words.ensure(9 * (size_t)n));
        HIP_TRY(hist.ensure(256 * bvh_radix_blocks(n)));
        HIP_TRY(scan.ensure(pseudonormal_scan_words(n)));
        HIP_TRY(st.ensure(8));
        HIP_TRY(reals.ensure(2 * (size_t)n));
        PseudonormalArgs a{};
        a.positions = c->positions.p, a.indices = c->indices.p, a.tri_ids = c->tri_ids.p, a.mesh_offsets = c->mesh_offsets.p, a.tri_count = t;
        a.table = c->pn_table.p;
        uint32_t* w = words.p;
        a.kx = w, a.ky = w + n, a.kz = w + 2 * (size_t)n, a.keys[0] = w + 3 * (size_t)n, a.keys[1] = w + 4 * (size_t)n;
        a.vals[0] = w + 5 * (size_t)n, a.vals[1] = w + 6 * (size_t)n, a.weld = w + 7 * (size_t)n, a.flag = w + 8 * (size_t)n;
        a.hist = hist.p, a.scan = scan.p, a.nf = reals.p, a.ang = reals.p + n, a.stats = st.p;
        launch_pseudonormals_build(c->stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(stats, st.p, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    CapPseudonormalsInfo& pi = c->pn_info;
    pi                       = CapPseudonormalsInfo{};
    pi.vertices = stats[0], pi.edges = stats[1], pi.boundary_edges = stats[2], pi.nonmanifold_edges = stats[3], pi.inconsistent_edges = stats[4];
    pi.degenerate_triangles = stats[5];
    pi.closed   = (stats[2] | stats[3] | stats[4]) == 0 && stats[5] < t ? 1u : 0u;
    pi.ms       = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    c->pn_ready = true;
    return CAP_OK;
}

// One dipole build (winding.hip) over a tree of t triangles, the scene's (no recs, bases 0) or an object's at (node_base, rec_base) of the
// forest's pools: its scratch, and its arguments from scratch of at least that size; root receives the tree's sums
static size_t winding_scratch_reals(uint32_t t) { return t ? 7 * (size_t)t + 14 * (size_t)(t - 1) : 0; }  // per triangle, per inner node
static size_t winding_scratch_words(uint32_t t) { return t ? 2 * (size_t)(t - 1) + 2 : 0; }               // per inner node, two counters
static WindingBuildArgs winding_build_args(const CapContext* c, const float4* nodes, float4* table, const float4* recs, uint32_t node_base, uint32_t rec_base,
                                           uint32_t t, double* reals, uint32_t* words, double* root)
{
    WindingBuildArgs a{c->positions.p, c->indices.p, c->tri_ids.p, c->mesh_offsets.p, t};  // (the rest zero)
    a.nodes = nodes + 4 * (size_t)node_base, a.table = table + 4 * (size_t)node_base, a.node_base = node_base, a.rec_base = rec_base;
    a.leaf_tri = c->leaf_tri.p, a.rec_ids = recs ? recs + 4 * (size_t)rec_base : nullptr;
    a.tri_sums = reals, a.sums = reals + 7 * (size_t)t, a.root = root, a.parent = words, a.flags = words + (t - 1u), a.stats = words + 2 * (size_t)(t - 1u);
    return a;
}

// The dipole table of cap_winding_numbers from the current vertices and the current binary tree (winding.hip): what cap_winding_build,
// cap_bvh_build and cap_bvh_refit share, by pseudonormals_rebuild's rules.  The scratch goes when the call returns.  Waits for the
// stream: the statistics are read back.  A failure drops the table.
static int winding_rebuild(CapContext* c)
{
    c->wn_ready = false;  // (until the table stands)
    c->wi_dirty = c->wi_forest_dirty = true;  // cap_winding_instances' derived tables follow the table
    const auto     wall0 = std::chrono::steady_clock::now();
    const uint32_t t     = c->tri_count, inner = t >= 2 ? t - 1 : 0;
    uint32_t       stats[2] = {0, 0};
    double         root[7]  = {0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(c->wn_root.ensure(7));  // the whole tree's sums, kept: the scene as the one object of cap_winding_instances
    if (!t) HIP_TRY(hipMemsetAsync(c->wn_root.p, 0, 7 * sizeof(double), c->stream));
    if (t)
    {
        if (c->wn_table.n < 4 * (size_t)inner)
        {
            HIP_TRY(hipStreamSynchronize(c->stream));  // (a grown table replaces one an earlier query may still be reading)
            HIP_TRY(c->wn_table.ensure(4 * (size_t)inner));
        }
        DevBuf<double>   reals;
        DevBuf<uint32_t> words;
        HIP_TRY(reals.ensure(winding_scratch_reals(t)));
        HIP_TRY(words.ensure(winding_scratch_words(t)));
        const WindingBuildArgs a = winding_build_args(c, c->nodes.p, c->wn_table.p, nullptr, 0, 0, t, reals.p, words.p, c->wn_root.p);
        launch_winding_build(c->stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(stats, a.stats, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(root, a.root, sizeof(root), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    CapWindingInfo& wi = c->wn_info;
    wi                 = CapWindingInfo{};
    wi.inner_nodes = inner, wi.degenerate_triangles = stats[0], wi.total_area = root[3];
    for (int k = 0; k < 3; ++k)
    {
        wi.root_n[k] = (float)root[k];
        // (without area: the centre of the scene's bounds, as a child without area takes the centre of its box)
        wi.root_p[k] = root[3] != 0.0 ? (float)(root[4 + k] / root[3]) : (float)(0.5 * ((double)c->bvh_info.bounds_lo[k] + (double)c->bvh_info.bounds_hi[k]));
    }
    wi.ms       = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    c->wn_ready = true;
    return CAP_OK;
}

// The derived tables of cap_winding_instances (winding.hip), enqueued on the context stream ahead of the query that found them dirty: no
// host wait, unless a buffer has to grow under a query that may still be reading it.  With an object table, first every object's dipole
// table and root sums, by the scene's build on the object's node and record range of the forest (only when the forest, the trees or
// the scene table changed: cap_instances_set alone leaves them); then the per-instance records and the top-level dipoles.
int cap::winding_instances_ensure(CapContext* c, const char* what)
{
    if (c->wi_built && !c->wi_dirty && !c->wi_forest_dirty) return CAP_OK;
    const uint32_t n = c->inst_count;
    uint32_t       off[kTlasMaxLevels], total = 0;
    tlas_layout(n, off, &total);
    uint32_t forest_nodes = 0, max_n = 0;
    for (uint32_t k = 0; k < c->obj_count; ++k) forest_nodes += c->obj_info[k].triangle_count - 1u, max_n = std::max(max_n, c->obj_info[k].triangle_count);
    const size_t roots = 7 * (size_t)std::max(c->obj_count, 1u), reals = winding_scratch_reals(max_n), words = winding_scratch_words(max_n);
    if (c->wi_inst.n < 3 * (size_t)n || c->wi_top.n < 2 * (size_t)total || c->wi_forest.n < 4 * (size_t)forest_nodes || c->wi_obj_root.n < roots ||
        c->wi_reals.n < reals || c->wi_words.n < words || !c->wi_count.p)
    {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (grown buffers replace ones an earlier query may still be reading)
        HIP_TRY(c->wi_inst.ensure(3 * (size_t)n));
        HIP_TRY(c->wi_top.ensure(2 * (size_t)total));
        HIP_TRY(c->wi_top_sums.ensure(7 * (size_t)total));
        HIP_TRY(c->wi_obj_root.ensure(roots));
        HIP_TRY(c->wi_count.ensure(1));
        if (c->obj_count)
        {
            if (c->wi_forest.n < 4 * (size_t)forest_nodes) c->wi_forest_dirty = true;
            HIP_TRY(c->wi_forest.ensure(4 * (size_t)forest_nodes));
            HIP_TRY(c->wi_reals.ensure(reals));
            HIP_TRY(c->wi_words.ensure(words));
        }
    }
    if (c->obj_count && c->wi_forest_dirty)
        for (uint32_t k = 0; k < c->obj_count; ++k)  // (the objects share the scratch: the stream orders them)
            launch_winding_build(c->stream, winding_build_args(c, c->forest_nodes.p, c->wi_forest.p, c->forest_tris.p, c->obj_node_base[k], c->obj_rec_base[k],
                                                               c->obj_info[k].triangle_count, c->wi_reals.p, c->wi_words.p, c->wi_obj_root.p + 7 * (size_t)k));
    WindingInstBuildArgs b{};
    b.descs = c->inst_desc.p, b.rec = c->inst_rec.p, b.tlas = c->inst_tlas.p, b.n = n;
    b.obj_root = c->obj_count ? c->wi_obj_root.p : c->wn_root.p;
    b.inst = c->wi_inst.p, b.top = c->wi_top.p, b.top_sums = c->wi_top_sums.p, b.count = c->wi_count.p;
    launch_winding_instances_build(c->stream, b);
    HIP_TRY(hipGetLastError());
    c->wi_built = true, c->wi_dirty = c->wi_forest_dirty = false;
    return trace_launch(c, "%s: derived tables of %u instances, %u forest records", what, n, forest_nodes);
}

void cap::winding_instances_release(CapContext* c)
{
    c->wi_inst.release(), c->wi_top.release(), c->wi_forest.release(), c->wi_top_sums.release(), c->wi_obj_root.release();
    c->wi_reals.release(), c->wi_words.release(), c->wi_count.release();
    c->wi_built = false, c->wi_dirty = c->wi_forest_dirty = true;
}

// what cap_winding_instances and its read-backs need of the context beyond query_state
static int winding_instances_state(CapContext* c, const char* what)
{
    if (const int rc = query_state(c, what)) return rc;
    if (!c->wn_ready) return fail(CAP_ERR_STATE, "%s: call cap_winding_build first", what);
    if (c->inst_count == 0) return fail(CAP_ERR_STATE, "%s: call cap_instances_set first", what);
    return CAP_OK;
}

extern "C" {

int cap_winding_instances_info(CapContext* c, CapWindingInstancesInfo* out)
{
    static_assert(sizeof(CapWindingInstancesInfo) == 160, "the header's record");
    if (!c || !out) return fail(CAP_ERR_INVALID_ARG, "cap_winding_instances_info: NULL argument");
    *out = CapWindingInstancesInfo{};
    out->instances = c->inst_count;
    if (c->inst_count)
    {
        uint32_t       off[kTlasMaxLevels], total = 0;
        const uint32_t top = tlas_layout(c->inst_count, off, &total);
        out->levels = top + 1u, out->entries = total;
        for (uint32_t l = 0; l <= top; ++l) out->level_entries[l] = (l < top ? off[l + 1] : total) - off[l];
    }
    const bool current = c->wi_built && !c->wi_dirty && !c->wi_forest_dirty && c->wn_ready && c->bvh_ready && !c->bvh_stale && c->inst_count;
    out->built = current ? 1u : 0u;
    if (!current) return CAP_OK;
    for (uint32_t k = 0; k < c->obj_count; ++k) out->forest_records += c->obj_info[k].triangle_count - 1u;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&out->contributing, c->wi_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    // the whole table: the one entry of the last level
    const size_t root = (size_t)out->entries - out->level_entries[out->levels - 1u];
    double       s[7];
    float        e[8];
    HIP_TRY(hipMemcpy(s, c->wi_top_sums.p + 7 * root, sizeof(s), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(e, c->wi_top.p + 2 * root, sizeof(e), hipMemcpyDeviceToHost));
    out->total_weight = s[3];
    for (int k = 0; k < 3; ++k) out->root_n[k] = e[4 + k], out->root_p[k] = e[k];
    return CAP_OK;
}

int cap_winding_instances_readback(CapContext* c, float* host_top, float* host_inst, float* host_forest)
{
    const char* what = "cap_winding_instances_readback";
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (const int rc = winding_instances_state(c, what)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = winding_instances_ensure(c, what)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t off[kTlasMaxLevels], total = 0, forest_nodes = 0;
    tlas_layout(c->inst_count, off, &total);
    for (uint32_t k = 0; k < c->obj_count; ++k) forest_nodes += c->obj_info[k].triangle_count - 1u;
    if (host_top) HIP_TRY(hipMemcpy(host_top, c->wi_top.p, sizeof(float4) * 2 * (size_t)total, hipMemcpyDeviceToHost));
    if (host_inst) HIP_TRY(hipMemcpy(host_inst, c->wi_inst.p, sizeof(float4) * 3 * (size_t)c->inst_count, hipMemcpyDeviceToHost));
    if (host_forest && forest_nodes) HIP_TRY(hipMemcpy(host_forest, c->wi_forest.p, sizeof(float4) * 4 * (size_t)forest_nodes, hipMemcpyDeviceToHost));
    return CAP_OK;
}

int cap_winding_build(CapContext* c, CapWindingInfo* out)
{
    static_assert(sizeof(CapWindingInfo) == 48, "the header's record");
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_winding_build: ctx is NULL");
    if (const int rc = query_state(c, "cap_winding_build")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = winding_rebuild(c)) return rc;
    if (out) *out = c->wn_info;
    return CAP_OK;
}

int cap_winding_drop(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_winding_drop: ctx is NULL");
    if (c->wn_table.p)
    {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (a query may still be reading it)
        c->wn_table.release();
    }
    if (c->wi_built || c->wi_inst.p || c->wi_forest.p)
    {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        winding_instances_release(c);
    }
    c->wn_ready = false;
    return CAP_OK;
}

int cap_winding_readback(CapContext* c, float* host_table)
{
    if (!c || !host_table) return fail(CAP_ERR_INVALID_ARG, "cap_winding_readback: NULL argument");
    if (const int rc = query_state(c, "cap_winding_readback")) return rc;
    if (!c->wn_ready) return fail(CAP_ERR_STATE, "cap_winding_readback: call cap_winding_build first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->wn_info.inner_nodes) HIP_TRY(hipMemcpy(host_table, c->wn_table.p, sizeof(float4) * 4 * (size_t)c->wn_info.inner_nodes, hipMemcpyDeviceToHost));
    return CAP_OK;
}

int cap_pseudonormals_build(CapContext* c, CapPseudonormalsInfo* out)
{
    static_assert(sizeof(CapPseudonormalsInfo) == 40, "the header's record");
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_pseudonormals_build: ctx is NULL");
    if (const int rc = query_state(c, "cap_pseudonormals_build")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = pseudonormals_rebuild(c, "cap_pseudonormals_build")) return rc;
    if (out) *out = c->pn_info;
    return CAP_OK;
}

int cap_pseudonormals_drop(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_pseudonormals_drop: ctx is NULL");
    if (c->pn_table.p)
    {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (a query may still be reading it)
        c->pn_table.release();
    }
    c->pn_ready = false;
    return CAP_OK;
}

int cap_pseudonormals_readback(CapContext* c, float* host_normals)
{
    if (!c || !host_normals) return fail(CAP_ERR_INVALID_ARG, "cap_pseudonormals_readback: NULL argument");
    if (const int rc = query_state(c, "cap_pseudonormals_readback")) return rc;
    if (!c->pn_ready) return fail(CAP_ERR_STATE, "cap_pseudonormals_readback: call cap_pseudonormals_build first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->tri_count) HIP_TRY(hipMemcpy(host_normals, c->pn_table.p, sizeof(float) * 21 * (size_t)c->tri_count, hipMemcpyDeviceToHost));
    return CAP_OK;
}

int cap_bvh_build(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_bvh_build: ctx is NULL");
    ++c->scene_generation;  // (the camera-vertex table of an earlier cap_render no longer stands for the scene: CameraTableKey)
    if (!c->scene_ready) return fail(CAP_ERR_STATE, "cap_bvh_build: no scene uploaded");
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = c->tri_count;
    // the dipole table belongs to the tree that is about to go (unlike the pseudonormal table, which is per triangle): it is not
    // ready again until the rebuild at the end has made the new tree's, whatever fails on the way
    const bool had_winding = c->wn_ready;
    c->wn_ready            = false;
    HIP_TRY(c->shade_tris.ensure(kShadeRec * (size_t)n));
    // + 4 zero records: the exhaustive kernels test triangles in pairs and fetch one pair ahead (cap_exhaustive.h); a zero record
    // has det == 0 and is never hit
    HIP_TRY(c->tris_sorted.ensure(4 * ((size_t)n + 4)));
    HIP_TRY(hipMemsetAsync(c->tris_sorted.p, 0, sizeof(float4) * 4 * ((size_t)n + 4), c->stream));
    HIP_TRY(c->tri_raw.ensure(4 * (size_t)n));
    HIP_TRY(c->tri_box.ensure(2 * (size_t)n));
    HIP_TRY(c->nodes.ensure(4 * (size_t)(n > 1 ? n - 1 : 1)));
    HIP_TRY(c->lane[0].stack_spill.ensure((size_t)c->cu_count * 8 * kBlock * kSpillEntries));  // up to 8 workgroups per CU
    HIP_TRY(c->leaf_tri.ensure(n));
    HIP_TRY(c->keys0.ensure(n));
    HIP_TRY(c->keys1.ensure(n));
    HIP_TRY(c->vals0.ensure(n));
    HIP_TRY(c->vals1.ensure(n));
    HIP_TRY(c->hist.ensure(256 * bvh_radix_blocks(n)));
    HIP_TRY(c->parent.ensure(2 * (size_t)n));
    HIP_TRY(c->flags.ensure(n));
    HIP_TRY(c->bvh_misc.ensure(8));
    const BvhBuildArgs a = bvh_args(c);
    // AUTO: scenes the exhaustive kernels handle need no tree quality (Morton hierarchy); everything else gets the clustering
    // build -- on the device like the driver build it replaces (blas_system.cpp:42-65), within 1 % of the host SAH tree's trace
    // times (builders table) at 1 / 40 of its build time.  The host SAH build stays available by name.
    const bool sah  = n >= 2 && c->bvh_build_mode == CAP_BVH_BUILD_SAH;
    // ... and from kAutoSahTriangles on the surface-area splits on top of it (round 6): host-SAH quality (expected node visits 44.6 against
    // 44.4 and the clustering's 47.6 on the 262 k hall) for 10 ms at 262 k and 0.2 s at 16.8 M triangles, built once like the reference's
    // PREFER_FAST_TRACE structures (blas_system.cpp:44); below, a build is a few dozen launches whatever it holds and the trees do not differ.
    const bool sahdev = n >= 2 && (c->bvh_build_mode == CAP_BVH_BUILD_SAH_DEVICE || (c->bvh_build_mode == CAP_BVH_BUILD_AUTO && n >= (uint32_t)c->sw.get(SW_AUTO_SAH_TRIANGLES, kAutoSahTriangles)));
    const bool ploc = n >= 2 && !sahdev && (c->bvh_build_mode == CAP_BVH_BUILD_PLOC || (c->bvh_build_mode == CAP_BVH_BUILD_AUTO && n > kExhaustiveMax));
    const auto wall0 = std::chrono::steady_clock::now();
    uint32_t   host_depth = 0;
    std::vector<float> bnodes_host;  // the binary tree on the host, for the collapse into the compressed 8-wide view
    if (sah)
    {
        launch_bvh_setup(c->stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        std::vector<float> boxes(8 * (size_t)n);
        HIP_TRY(hipMemcpy(boxes.data(), c->tri_box.p, sizeof(float) * boxes.size(), hipMemcpyDeviceToHost));
        HostTree tree;
        build_sah_tree(boxes.data(), n, kLeafMax, kLeafCountShift, tree);
        host_depth = tree.depth;
        HIP_TRY(hipMemcpy(c->nodes.p, tree.nodes.data(), sizeof(float) * tree.nodes.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->leaf_tri.p, tree.order.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        launch_bvh_finish_host(c->stream, a);
        bnodes_host.swap(tree.nodes);
    }
    else if (sahdev)
    {
        // surface-area splits from the root down, the clustering inside the finished segments: the PREFER_FAST_TRACE tree the reference
        // asks its driver for (blas_system.cpp:44), built where the geometry is
        HIP_TRY(c->ploc_boxes.ensure(4 * (size_t)n));
        HIP_TRY(c->ploc_ints.ensure(3 * (size_t)n + 4));
        HIP_TRY(c->sahdev_words.ensure(bvh_sah_device_scratch_words(n)));
        const int radius = (int)c->sw.get(SW_PLOC_RADIUS, 16), leaf = (int)c->sw.get(SW_SAHDEV_LEAF, 32);  // A/B switches
        const int rc = launch_bvh_build_sah_device(c->stream, a, PlocScratch{c->ploc_boxes.p, c->ploc_ints.p}, c->sahdev_words.p, (uint32_t)radius,
                                                   (uint32_t)(leaf < 1 ? 1 : leaf));
        if (rc != 0) return fail(CAP_ERR_HIP, "cap_bvh_build: device surface-area build failed (%d)", rc);
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->sahdev_words.release();  // 90 B per triangle, of no use after the build
    }
    else if (ploc)
    {
        HIP_TRY(c->ploc_boxes.ensure(4 * (size_t)n));
        HIP_TRY(c->ploc_ints.ensure(3 * (size_t)n + 4));
        const int radius = (int)c->sw.get(SW_PLOC_RADIUS, 16);  // A/B switch
        const int rc = launch_bvh_build_ploc(c->stream, a, PlocScratch{c->ploc_boxes.p, c->ploc_ints.p}, (uint32_t)radius);
        if (rc != 0) return fail(CAP_ERR_HIP, "cap_bvh_build: clustering build failed (%d)", rc);
    }
    else
        launch_bvh_build(c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    uint32_t misc[8] = {0};
    if (n) HIP_TRY(hipMemcpy(misc, c->bvh_misc.p, sizeof(misc), hipMemcpyDeviceToHost));
    CapBvhInfo& bi    = c->bvh_info;
    bi                = CapBvhInfo{};
    bi.triangle_count = n;
    bi.node_count     = n > 1 ? n - 1 : 0;
    bi.max_depth      = n ? (sah ? host_depth : misc[6]) : 0;
    bi.build_ms       = ms;
    if (n) set_bounds(bi, misc);
    c->shade_tame = n != 0 && misc[7] == 0;
    if (bi.max_depth > 64)
        return fail(CAP_ERR_UNSUPPORTED, "LBVH depth %u exceeds the 64-entry traversal stack", bi.max_depth);
    bi.stack_entries = bi.max_depth <= 32 ? 32 : 64;
    // Compressed 8-wide view of the same tree (cap_wide.h) for the extension- and shadow-ray kernels of scenes the exhaustive
    // kernels do not take: collapsed on the host from the binary nodes (read back when the device built them).
    c->wide8_nodes = c->wide8_depth = c->wide8_top = 0;
    c->wide_levels.clear();
    if (n >= 1)
    {
        const auto w0 = std::chrono::steady_clock::now();
        HIP_TRY(c->tris8.ensure(4 * (size_t)n));
        HIP_TRY(c->wide_src.ensure(n));
        size_t   wn = 0;
        uint32_t wdepth = 0, wtop = 0;
        const bool host_collapse = c->sw.on(SW_WIDE_HOST_COLLAPSE);  // A/B switch
        if (!sah && n >= 2 && !host_collapse)
        {
            // the device built the binary tree: collapse it there too (bvh.hip k_wide_level), nothing leaves the GPU
            const uint32_t cap = n / 2u + 16u;  // an inner child stands for >= 4 triangles
            HIP_TRY(c->nodes8.ensure((kWideNodeStride / 4) * std::max<size_t>((size_t)cap + 1, kWideTopNodes)));
            HIP_TRY(c->wide_task.ensure(cap));
            HIP_TRY(c->wide_cnt.ensure(2 * (size_t)cap + 2 * ((size_t)cap / 1024 + 2)));  // per-level bases + the scan's tile sums
            HIP_TRY(c->wide_alloc.ensure(2));
            WideCollapseArgs wa{};
            wa.bnodes = c->nodes.p, wa.count = c->keys1.p, wa.n_tris = n, wa.capacity = cap;
            wa.pad = wide_pad(bi);
            wa.task = c->wide_task.p, wa.cnt = c->wide_cnt.p, wa.alloc = c->wide_alloc.p, wa.nodes8 = reinterpret_cast<uint32_t*>(c->nodes8.p), wa.tri_src = c->wide_src.p;
            uint32_t count = 0;
            if (launch_wide_collapse(c->stream, wa, &count, &wdepth, &wtop, &c->wide_levels) != 0) return fail(CAP_ERR_HIP, "cap_bvh_build: device collapse into the 8-wide view failed");
            wn = count;
        }
        else
        {
            if (n >= 2 && bnodes_host.empty())
            {
                bnodes_host.resize(16 * (size_t)(n - 1));
                HIP_TRY(hipMemcpy(bnodes_host.data(), c->nodes.p, sizeof(float) * bnodes_host.size(), hipMemcpyDeviceToHost));
            }
            WideTree wt;
            build_wide_tree(n >= 2 ? bnodes_host.data() : nullptr, n, bi.bounds_lo, bi.bounds_hi, wt);
            wn = wt.nodes.size() / kWideNodeWords, wdepth = wt.depth, wtop = wt.top_nodes;
            c->wide_levels = wt.level_begin;
            c->wide_levels.push_back((uint32_t)wn);
            HIP_TRY(c->nodes8.ensure((kWideNodeStride / 4) * std::max<size_t>(wn + 1, kWideTopNodes)));
            if (wn) HIP_TRY(hipMemcpy2D(c->nodes8.p, sizeof(uint32_t) * kWideNodeStride, wt.nodes.data(), sizeof(uint32_t) * kWideNodeWords,
                                        sizeof(uint32_t) * kWideNodeWords, wn, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(c->wide_src.p, wt.tri_src.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        }
        launch_gather_wide(c->stream, c->wide_src.p, c->tris_sorted.p, n, c->tris8.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->wide8_nodes = (uint32_t)wn, c->wide8_depth = wdepth, c->wide8_top = wtop;
        c->wide8_ms    = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
        bi.build_ms += c->wide8_ms;  // the collapse is part of the build
        if (c->sw.on(SW_TRACE_LAUNCHES))
            fprintf(stderr, "[cap] wide view: %zu nodes, depth %u, top %u, %.1f ms\n", wn, wdepth, wtop, c->wide8_ms);
    }
    if (const int rc = upload_fan_records(c)) return rc;
    c->bvh_ready          = true;
    c->bvh_stale          = false;
    c->visits_built_known = false;  // the first refit measures the boxes this build leaves
    if (const int rc = update_nee_pairs(c)) return rc;
    if (const int rc = objects_rebuild(c, "cap_bvh_build"))  // the objects' trees from the same vertices (nothing without a table)
    {
        c->inst_count = 0;  // (the instances' objects are gone)
        return rc;
    }
    if (const int rc = instances_rebuild(c)) return rc;  // (nothing without a table)
    if (c->pn_ready)  // the pseudonormal table, when one exists
        if (const int rc = pseudonormals_rebuild(c, "cap_bvh_build")) return rc;
    return had_winding ? winding_rebuild(c) : CAP_OK;  // the dipole table, when one existed: the new tree's
}

int cap_scene_update_vertices(CapContext* c, const float* positions, const float* normals, const float* texcoords, uint32_t flags)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_scene_update_vertices: ctx is NULL");
    ++c->scene_generation;  // (the camera-vertex table of an earlier cap_render no longer stands for the scene: CameraTableKey)
    if (!c->scene_ready) return fail(CAP_ERR_STATE, "cap_scene_update_vertices: no scene uploaded");
    if (flags & ~(uint32_t)CAP_VERTICES_DEVICE) return fail(CAP_ERR_INVALID_ARG, "cap_scene_update_vertices: unknown flags 0x%x", flags);
    const bool   device = (flags & CAP_VERTICES_DEVICE) != 0;
    const float* src[3] = {positions, normals, texcoords};
    const char*  name[3] = {"positions", "normals", "texcoords"};
    float*       dst[3] = {c->positions.p, c->normals.p, c->texcoords.p};
    const size_t bytes[3] = {sizeof(float) * 3 * (size_t)c->vertex_count, sizeof(float) * 3 * (size_t)c->vertex_count,
                             sizeof(float) * 2 * (size_t)c->vertex_count};
    HIP_TRY(hipSetDevice(c->device));
    if (device)
        for (int i = 0; i < 3; ++i)
        {
            if (!src[i]) continue;
            if ((uintptr_t)src[i] & 3u) return fail(CAP_ERR_INVALID_ARG, "cap_scene_update_vertices: %s is not 4-byte aligned", name[i]);
            hipPointerAttribute_t at{};
            const hipError_t      e = hipPointerGetAttributes(&at, src[i]);
            if (e != hipSuccess) (void)hipGetLastError();  // (an unknown pointer is the caller's error, not a sticky one)
            if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != c->device)
                return fail(CAP_ERR_INVALID_ARG, "cap_scene_update_vertices: %s is not device memory of device %d", name[i], c->device);
        }
    // ordered on the context stream behind everything enqueued (a render's second lane joins it at the end of its call)
    bool copied = false;
    for (int i = 0; i < 3; ++i)
        if (src[i] && bytes[i])
        {
            HIP_TRY(hipMemcpyAsync(dst[i], src[i], bytes[i], device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
            copied = true;
        }
    if (copied && !device) HIP_TRY(hipStreamSynchronize(c->stream));  // host arrays may go once the call returns
    if (positions)
    {
        if (device)
            c->positions_host_stale = true;  // read back only if the light table or the next-event list needs it
        else
        {
            c->positions_host.assign(positions, positions + 3 * (size_t)c->vertex_count);
            c->positions_host_stale = false;
        }
    }
    c->bvh_stale = true;  // normals and uvs too: the shading records hold them
    return CAP_OK;
}

int cap_bvh_refit(CapContext* c, CapRefitInfo* out)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_bvh_refit: ctx is NULL");
    ++c->scene_generation;  // (the camera-vertex table of an earlier cap_render no longer stands for the scene: CameraTableKey)
    if (!c->scene_ready || !c->bvh_ready) return fail(CAP_ERR_STATE, "cap_bvh_refit: no tree built since the last cap_scene_upload");
    HIP_TRY(hipSetDevice(c->device));
    const auto         wall0 = std::chrono::steady_clock::now();
    const uint32_t     n     = c->tri_count;
    const BvhBuildArgs a     = bvh_args(c);
    // the tree metric of the build's boxes (first refit after a build only: before they are overwritten), then of the refitted ones
    const size_t scratch = tree_visits_scratch();
    HIP_TRY(c->refit_sums.ensure(scratch + 2));
    double* const visits = c->refit_sums.p + scratch;  // {this refit, the build}
    if (!c->visits_built_known) launch_tree_visits(c->stream, c->nodes.p, n, c->refit_sums.p, visits + 1);
    // triangle records, shading records, triangle boxes, scene bounds; binary boxes; records in leaf order
    launch_refit_binary(c->stream, a);
    launch_tree_visits(c->stream, c->nodes.p, n, c->refit_sums.p, visits);
    HIP_TRY(hipGetLastError());
    // the one read inside the refit: the new scene bounds (the wide view's padding, the render's camera test, the queries' hand-over)
    CapBvhInfo& bi = c->bvh_info;
    if (n)
    {
        uint32_t misc[8];  // ... and whether the rewritten shading records are tame
        HIP_TRY(hipMemcpyAsync(misc, c->bvh_misc.p, sizeof(misc), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        set_bounds(bi, misc);
        c->shade_tame = misc[7] == 0;
    }
    // the 8-wide view: records in its leaf order, then its planes bottom-up
    if (c->wide8_nodes)
    {
        launch_gather_wide(c->stream, c->wide_src.p, c->tris_sorted.p, n, c->tris8.p);
        HIP_TRY(c->wide_boxes.ensure(6 * (size_t)c->wide8_nodes));
        WideRefitArgs wa{};
        wa.nodes8 = reinterpret_cast<uint32_t*>(c->nodes8.p), wa.tris8 = c->tris8.p, wa.tri_box = c->tri_box.p, wa.boxes = c->wide_boxes.p;
        wa.pad = wide_pad(bi), wa.one_triangle = n == 1 ? 1u : 0u;
        launch_refit_wide(c->stream, wa, c->wide_levels);
        HIP_TRY(hipGetLastError());
    }
    // the small-scene records, the EXT light table and next-event pair list
    if (const int rc = upload_fan_records(c)) return rc;
    if (c->materials_ready && c->light_count)
        if (const int rc = upload_light_table(c)) return rc;
    if (const int rc = update_nee_pairs(c)) return rc;
    double v[2] = {1.0, 1.0};
    if (n >= 2) HIP_TRY(hipMemcpyAsync(v, visits, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!c->visits_built_known) c->refit_visits_built = v[1], c->visits_built_known = true;
    c->bvh_stale = false;
    if (const int rc = objects_rebuild(c, "cap_bvh_refit"))  // the objects' trees: rebuilt, not refitted (nothing without a table)
    {
        c->inst_count = 0;
        return rc;
    }
    if (const int rc = instances_rebuild(c)) return rc;  // world boxes and TLAS from the new bounds (nothing without a table)
    if (c->pn_ready)                                     // the pseudonormal table, when one exists: rebuilt, the weld included
        if (const int rc = pseudonormals_rebuild(c, "cap_bvh_refit")) return rc;
    if (c->wn_ready)                                     // the dipole table, when one exists: the moved triangles' moments, the refitted boxes' radii
        if (const int rc = winding_rebuild(c)) return rc;
    if (out)
    {
        out->ms                         = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        out->expected_node_visits       = v[0];
        out->expected_node_visits_built = c->refit_visits_built;
    }
    return CAP_OK;
}

int cap_bvh_info(CapContext* c, CapBvhInfo* out)
{
    if (!c || !out) return fail(CAP_ERR_INVALID_ARG, "cap_bvh_info: NULL argument");
    if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_bvh_info: BVH not built");
    *out = c->bvh_info;
    return CAP_OK;
}

int cap_bvh_readback(CapContext* c, float* nodes, uint32_t* leaf_triangles)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_bvh_readback: ctx is NULL");
    if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_bvh_readback: BVH not built");
    if (c->bvh_stale) return fail(CAP_ERR_STATE, "cap_bvh_readback: vertices changed; call cap_bvh_refit or cap_bvh_build");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nodes && c->bvh_info.node_count)
        HIP_TRY(hipMemcpy(nodes, c->nodes.p, sizeof(float4) * 4 * c->bvh_info.node_count, hipMemcpyDeviceToHost));
    if (leaf_triangles && c->tri_count)
        HIP_TRY(hipMemcpy(leaf_triangles, c->leaf_tri.p, sizeof(uint32_t) * c->tri_count, hipMemcpyDeviceToHost));
    return CAP_OK;
}

int cap_bvh_wide_readback(CapContext* c, uint32_t* nodes, uint32_t* tri_src, uint32_t* info)
{
    if (!c || !info) return fail(CAP_ERR_INVALID_ARG, "cap_bvh_wide_readback: NULL argument");
    if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_bvh_wide_readback: BVH not built");
    if (c->bvh_stale) return fail(CAP_ERR_STATE, "cap_bvh_wide_readback: vertices changed; call cap_bvh_refit or cap_bvh_build");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    info[0] = c->wide8_nodes, info[1] = c->wide8_depth, info[2] = c->wide8_top;
    if (nodes && c->wide8_nodes)
        HIP_TRY(hipMemcpy2D(nodes, sizeof(uint32_t) * kWideNodeWords, c->nodes8.p, sizeof(uint32_t) * kWideNodeStride, sizeof(uint32_t) * kWideNodeWords,
                            c->wide8_nodes, hipMemcpyDeviceToHost));
    if (tri_src && c->tri_count) HIP_TRY(hipMemcpy(tri_src, c->wide_src.p, sizeof(uint32_t) * c->tri_count, hipMemcpyDeviceToHost));
    return CAP_OK;
}

}  // extern "C"

// ---- the instance table and its top-level tree (instance.hip) ----
namespace
{
// `p` is usable as a device array of the context's GPU (what CAP_INSTANCES_DEVICE promises)
int device_array(CapContext* c, const char* what, const char* name, const void* p)
{
    if ((uintptr_t)p & 3u) return fail(CAP_ERR_INVALID_ARG, "%s: %s is not 4-byte aligned", what, name);
    hipPointerAttribute_t at{};
    const hipError_t      e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) (void)hipGetLastError();  // (an unknown pointer is the caller's error, not a sticky one)
    if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != c->device)
        return fail(CAP_ERR_INVALID_ARG, "%s: %s is not device memory of device %d", what, name, c->device);
    return CAP_OK;
}

int instances_set(CapContext* c, const char* what, const CapInstanceDesc* descs, const uint32_t* object_index, uint32_t count, uint32_t flags,
                  CapInstancesInfo* out)
{
    static_assert(sizeof(CapInstanceDesc) == 64, "CapInstanceDesc is 16 words");
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (flags & ~(uint32_t)CAP_INSTANCES_DEVICE) return fail(CAP_ERR_INVALID_ARG, "%s: unknown flags 0x%x", what, flags);
    if (count > CAP_INSTANCE_MAX_COUNT) return fail(CAP_ERR_INVALID_ARG, "%s: %u instances exceed CAP_INSTANCE_MAX_COUNT (%u)", what, count, CAP_INSTANCE_MAX_COUNT);
    if (count && !descs) return fail(CAP_ERR_INVALID_ARG, "%s: descs is NULL", what);
    const bool device = (flags & CAP_INSTANCES_DEVICE) != 0;
    if (!device)
        for (uint32_t i = 0; i < count; ++i)
            if (descs[i].reserved[0] | descs[i].reserved[1] | descs[i].reserved[2])
                return fail(CAP_ERR_INVALID_ARG, "%s: descs[%u].reserved must be 0", what, i);
    if (const int rc = query_state(c, what)) return rc;
    // host object indices are checked here; device ones in k_instance_setup, where an out-of-range one makes the instance inert
    const uint32_t n_objects = c->obj_count ? c->obj_count : 1u;
    if (!device && object_index)
        for (uint32_t i = 0; i < count; ++i)
            if (object_index[i] >= n_objects)
                return fail(CAP_ERR_INVALID_ARG, c->obj_count ? "%s: object_index[%u] = %u, the object table has %u objects"
                                                              : "%s: object_index[%u] = %u without an object table (%u object: the scene)",
                            what, i, object_index[i], n_objects);
    const auto wall0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c->device));
    if (device && count)
    {
        if (const int rc = device_array(c, what, "descs", descs)) return rc;
        if (object_index)
            if (const int rc = device_array(c, what, "object_index", object_index)) return rc;
    }
    if (count == 0)
    {
        c->inst_count = 0;  // host state: queries already enqueued keep the table they were given
        c->wi_dirty   = true;
        if (out) *out = CapInstancesInfo{};
        return CAP_OK;
    }
    uint32_t       off[kTlasMaxLevels], total = 0;
    const uint32_t top = tlas_layout(count, off, &total);
    if (c->inst_desc.n < 4 * (size_t)count || c->inst_misc.n < 8 || c->inst_obj.n < count || c->inst_near.n < count)
    {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (grown buffers replace ones an earlier query may still be reading)
        HIP_TRY(c->inst_desc.ensure(4 * (size_t)count));
        HIP_TRY(c->inst_rec.ensure(4 * (size_t)count));
        HIP_TRY(c->inst_box.ensure(2 * (size_t)count));
        HIP_TRY(c->inst_near.ensure(count));
        HIP_TRY(c->inst_tlas.ensure(2 * ((size_t)count + (size_t)count + 2 * kTlasMaxLevels + 2)));
        for (int k = 0; k < 2; ++k)
        {
            HIP_TRY(c->inst_keys[k].ensure(count));
            HIP_TRY(c->inst_vals[k].ensure(count));
        }
        HIP_TRY(c->inst_hist.ensure(256 * bvh_radix_blocks(count)));
        HIP_TRY(c->inst_scan.ensure(bvh_radix_scan_words(count) + 1));
        HIP_TRY(c->inst_misc.ensure(8));
        HIP_TRY(c->inst_level_off.ensure(kTlasMaxLevels + 1));
        HIP_TRY(c->inst_obj.ensure(count));
    }
    if ((size_t)total * 2 > c->inst_tlas.n) return fail(CAP_ERR_HIP, "%s: top-level tree of %u entries exceeds its buffer", what, total);
    // ordered on the context stream behind every query enqueued
    HIP_TRY(hipMemcpyAsync(c->inst_desc.p, descs, sizeof(CapInstanceDesc) * (size_t)count, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(c->inst_level_off.p, off, sizeof(uint32_t) * (top + 1), hipMemcpyHostToDevice, c->stream));
    if (object_index)
        HIP_TRY(hipMemcpyAsync(c->inst_obj.p, object_index, sizeof(uint32_t) * (size_t)count, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               c->stream));
    c->inst_obj_on = object_index != nullptr;
    c->inst_count = count, c->inst_top = top, c->inst_nodes = total - (count + (count & 1u));
    if (const int rc = instances_rebuild(c))
    {
        c->inst_count = 0;
        return rc;
    }
    uint32_t inert = 0;
    if (out) HIP_TRY(hipMemcpyAsync(&inert, c->inst_misc.p + 6, sizeof(inert), hipMemcpyDeviceToHost, c->stream));
    if (out || !device) HIP_TRY(hipStreamSynchronize(c->stream));  // host descriptors and `off` may go once the call returns
    if (out)
    {
        out->count = count, out->inert = inert, out->tlas_nodes = c->inst_nodes, out->tlas_depth = top + 1;
        out->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return CAP_OK;
}
}  // namespace

extern "C" {

int cap_instances_set(CapContext* c, const CapInstanceDesc* descs, uint32_t count, uint32_t flags, CapInstancesInfo* out)
{
    return instances_set(c, "cap_instances_set", descs, nullptr, count, flags, out);
}

int cap_instances_set_ex(CapContext* c, const CapInstanceDesc* descs, const uint32_t* object_index, uint32_t count, uint32_t flags, CapInstancesInfo* out)
{
    return instances_set(c, "cap_instances_set_ex", descs, object_index, count, flags, out);
}

// ---- objects: per-mesh-range trees below the instances (objects_rebuild; instance.hip) ----
int cap_objects_set(CapContext* c, const CapObjectRange* ranges, uint32_t count, CapObjectsInfo* out)
{
    static_assert(sizeof(CapObjectRange) == 8 && sizeof(CapObjectInfo) == 48 && sizeof(CapObjectsInfo) == 24, "the header's object records");
    const char* what = "cap_objects_set";
    if (!c) return fail(CAP_ERR_INVALID_ARG, "%s: ctx is NULL", what);
    if (count > CAP_OBJECT_MAX_COUNT) return fail(CAP_ERR_INVALID_ARG, "%s: %u objects exceed CAP_OBJECT_MAX_COUNT (%u)", what, count, CAP_OBJECT_MAX_COUNT);
    if (count && !ranges) return fail(CAP_ERR_INVALID_ARG, "%s: ranges is NULL", what);
    if (const int rc = query_state(c, what)) return rc;
    const auto wall0 = std::chrono::steady_clock::now();
    // global triangle ids are assigned mesh by mesh in upload order: a mesh range is a triangle range
    std::vector<uint64_t> tri_begin(c->mesh_count + 1, 0);
    for (uint32_t m = 0; m < c->mesh_count; ++m) tri_begin[m + 1] = tri_begin[m] + c->meshes_host[m].index_count / 3;
    std::vector<CapObjectInfo> info(count);
    std::vector<uint32_t>      node_base(count), rec_base(count);
    std::vector<std::pair<uint32_t, uint32_t>> sorted;  // (first mesh, object)
    uint64_t nodes = 0, recs = 0;
    for (uint32_t k = 0; k < count; ++k)
    {
        const CapObjectRange& r = ranges[k];
        if (r.mesh_count == 0) return fail(CAP_ERR_INVALID_ARG, "%s: ranges[%u].mesh_count is 0", what, k);
        if ((uint64_t)r.first_mesh + r.mesh_count > c->mesh_count)
            return fail(CAP_ERR_INVALID_ARG, "%s: ranges[%u] = meshes %u + %u exceeds the scene's %u", what, k, r.first_mesh, r.mesh_count, c->mesh_count);
        const uint64_t first = tri_begin[r.first_mesh], n = tri_begin[r.first_mesh + r.mesh_count] - first;
        if (n == 0) return fail(CAP_ERR_INVALID_ARG, "%s: ranges[%u] holds no triangle", what, k);
        // the walk's leaf code keeps a record's forest position in kLeafCountShift bits (cap_leaf.h)
        if (recs + n > kLeafFirstMask) return fail(CAP_ERR_UNSUPPORTED, "%s: forest position %llu of object %u does not fit the traversal-leaf code (limit %u)", what, (unsigned long long)(recs + n), k, kLeafFirstMask);
        info[k]                = CapObjectInfo{};
        info[k].first_triangle = (uint32_t)first, info[k].triangle_count = (uint32_t)n, info[k].node_count = (uint32_t)n - 1u;
        node_base[k] = (uint32_t)nodes, rec_base[k] = (uint32_t)recs;
        nodes += n - 1, recs += n;
        sorted.emplace_back(r.first_mesh, k);
    }
    std::sort(sorted.begin(), sorted.end());
    for (size_t j = 1; j < sorted.size(); ++j)
    {
        const CapObjectRange& a = ranges[sorted[j - 1].second];
        if (a.first_mesh + a.mesh_count > sorted[j].first)
            return fail(CAP_ERR_INVALID_ARG, "%s: ranges[%u] and ranges[%u] overlap", what, sorted[j - 1].second, sorted[j].second);
    }
    // from here on the tables change: object indices lose their meaning, so the instance table goes with the old object table
    c->inst_count = 0;
    c->obj_count  = 0;
    c->wi_dirty = c->wi_forest_dirty = true;
    if (count == 0)
    {
        if (out) *out = CapObjectsInfo{};
        return CAP_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    uint32_t max_n = 0;
    for (const CapObjectInfo& o : info) max_n = std::max(max_n, o.triangle_count);
    if (c->forest_tris.n < 4 * (size_t)recs || c->forest_nodes.n < 4 * (size_t)std::max<uint64_t>(nodes, 1) || c->obj_table.n < count || c->obj_misc.n < 8 * (size_t)count ||
        c->obj_tri_raw.n < 4 * (size_t)max_n)
    {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (grown buffers replace ones an earlier query may still be reading)
        HIP_TRY(c->forest_tris.ensure(4 * (size_t)recs));
        HIP_TRY(c->forest_nodes.ensure(4 * (size_t)std::max<uint64_t>(nodes, 1)));
        HIP_TRY(c->obj_table.ensure(count));
        HIP_TRY(c->obj_misc.ensure(8 * (size_t)count));
        HIP_TRY(c->obj_tri_raw.ensure(4 * (size_t)max_n));
        HIP_TRY(c->obj_tri_box.ensure(2 * (size_t)max_n));
        HIP_TRY(c->obj_leaf_tri.ensure(max_n));
    }
    c->obj_info.swap(info), c->obj_node_base.swap(node_base), c->obj_rec_base.swap(rec_base);
    c->obj_count = count;
    if (const int rc = objects_rebuild(c, what)) return rc;
    if (out)
    {
        out->count = count, out->triangles = (uint32_t)recs, out->nodes = (uint32_t)nodes, out->max_depth = c->obj_max_depth;
        out->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return CAP_OK;
}

int cap_objects_info(CapContext* c, CapObjectInfo* out, uint32_t capacity, uint32_t* count_out)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_objects_info: ctx is NULL");
    if (capacity && !out) return fail(CAP_ERR_INVALID_ARG, "cap_objects_info: out is NULL with capacity %u", capacity);
    if (count_out) *count_out = c->obj_count;
    const uint32_t n = std::min(capacity, c->obj_count);
    if (n) std::copy(c->obj_info.begin(), c->obj_info.begin() + n, out);
    return CAP_OK;
}

int cap_objects_readback(CapContext* c, float* nodes, uint32_t* leaf_triangles)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_objects_readback: ctx is NULL");
    if (const int rc = query_state(c, "cap_objects_readback")) return rc;
    if (c->obj_count == 0) return fail(CAP_ERR_STATE, "cap_objects_readback: no object table installed");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n_nodes = (size_t)c->obj_node_base.back() + c->obj_info.back().triangle_count - 1u;
    const size_t n_recs  = (size_t)c->obj_rec_base.back() + c->obj_info.back().triangle_count;
    if (nodes && n_nodes) HIP_TRY(hipMemcpy(nodes, c->forest_nodes.p, sizeof(float4) * 4 * n_nodes, hipMemcpyDeviceToHost));
    // word 12 of each 64-byte record: the scene's triangle id
    if (leaf_triangles)
        HIP_TRY(hipMemcpy2D(leaf_triangles, sizeof(uint32_t), reinterpret_cast<const float*>(c->forest_tris.p) + 12, sizeof(float4) * 4, sizeof(uint32_t), n_recs,
                            hipMemcpyDeviceToHost));
    return CAP_OK;
}

int cap_instances_readback(CapContext* c, float* world_to_object, float* world_boxes)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_instances_readback: ctx is NULL");
    if (c->inst_count == 0) return fail(CAP_ERR_STATE, "cap_instances_readback: no instance table installed");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t n = c->inst_count;
    std::vector<float> rec(16 * n), box(8 * n);
    HIP_TRY(hipMemcpy(rec.data(), c->inst_rec.p, sizeof(float) * rec.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(box.data(), c->inst_box.p, sizeof(float) * box.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
    {
        if (world_to_object) std::copy(rec.begin() + 16 * i, rec.begin() + 16 * i + 12, world_to_object + 12 * i);
        if (world_boxes)
            for (int k = 0; k < 3; ++k) world_boxes[6 * i + k] = box[8 * i + k], world_boxes[6 * i + 3 + k] = box[8 * i + 4 + k];
    }
    return CAP_OK;
}
}  // extern "C"
