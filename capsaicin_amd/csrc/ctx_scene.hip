// ctx_scene.hip — what a context knows of its scene beside the trees: geometry, instance masks, textures, blue noise and materials as
// uploaded, the small-scene fan records and the next-event pair list made from them, the EXT model's light table.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cap_context.h"

extern "C" {

int cap_scene_upload(CapContext* c, const float* positions, const float* normals, const float* texcoords, const uint32_t* indices,
                     const CapMeshDesc* meshes, uint32_t vertex_count, uint32_t index_count, uint32_t mesh_count)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_scene_upload: ctx is NULL");
    ++c->scene_generation;  // (the camera-vertex table of an earlier cap_render no longer stands for the scene: CameraTableKey)
    if ((vertex_count && (!positions || !normals || !texcoords)) || (index_count && !indices) || (mesh_count && !meshes))
        return fail(CAP_ERR_INVALID_ARG, "cap_scene_upload: NULL array with non-zero count");
    // validate the descriptors on the host: the kernels index with them unchecked
    std::vector<uint4> tri_ids;
    std::vector<uint4> mesh_offsets(mesh_count);
    std::vector<uint32_t> mesh_texture(mesh_count);
    for (uint32_t m = 0; m < mesh_count; ++m)
    {
        const CapMeshDesc& d = meshes[m];
        if (d.index != m) return fail(CAP_ERR_INVALID_ARG, "mesh %u: index field is %u (InstanceID must equal the mesh slot)", m, d.index);
        if (d.index_count % 3) return fail(CAP_ERR_INVALID_ARG, "mesh %u: index_count %u is not a multiple of 3", m, d.index_count);
        if ((uint64_t)d.first_index_offset + d.index_count > index_count || (uint64_t)d.first_vertex_offset + d.vertex_count > vertex_count)
            return fail(CAP_ERR_INVALID_ARG, "mesh %u: ranges exceed the pools", m);
        for (uint32_t k = 0; k < d.index_count; ++k)
            if (indices[d.first_index_offset + k] >= d.vertex_count)
                return fail(CAP_ERR_INVALID_ARG, "mesh %u: index %u out of range", m, indices[d.first_index_offset + k]);
        mesh_offsets[m] = make_uint4(d.first_vertex_offset, d.first_index_offset, 0, 0);
        mesh_texture[m] = d.texture_index;
        for (uint32_t p = 0; p < d.index_count / 3; ++p) tri_ids.push_back(make_uint4(m, p, d.texture_index, 0u));
    }
    // the traversal-leaf code keeps the first sorted triangle in kLeafCountShift bits (cap_leaf.h)
    if (tri_ids.size() > kLeafFirstMask) return fail(CAP_ERR_UNSUPPORTED, "too many triangles: %zu (limit %u)", tri_ids.size(), kLeafFirstMask);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->positions.ensure(3 * (size_t)vertex_count));
    HIP_TRY(c->normals.ensure(3 * (size_t)vertex_count));
    HIP_TRY(c->texcoords.ensure(2 * (size_t)vertex_count));
    HIP_TRY(c->indices.ensure(index_count));
    HIP_TRY(c->tri_ids.ensure(tri_ids.size()));
    HIP_TRY(c->mesh_offsets.ensure(mesh_count));
    HIP_TRY(c->mesh_texture.ensure(mesh_count));
    if (vertex_count)
    {
        HIP_TRY(hipMemcpy(c->positions.p, positions, sizeof(float) * 3 * vertex_count, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->normals.p, normals, sizeof(float) * 3 * vertex_count, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->texcoords.p, texcoords, sizeof(float) * 2 * vertex_count, hipMemcpyHostToDevice));
    }
    if (index_count) HIP_TRY(hipMemcpy(c->indices.p, indices, sizeof(uint32_t) * index_count, hipMemcpyHostToDevice));
    if (!tri_ids.empty()) HIP_TRY(hipMemcpy(c->tri_ids.p, tri_ids.data(), sizeof(uint4) * tri_ids.size(), hipMemcpyHostToDevice));
    if (mesh_count)
    {
        HIP_TRY(hipMemcpy(c->mesh_offsets.p, mesh_offsets.data(), sizeof(uint4) * mesh_count, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->mesh_texture.p, mesh_texture.data(), sizeof(uint32_t) * mesh_count, hipMemcpyHostToDevice));
    }
    c->positions_host.assign(positions, positions + 3 * (size_t)vertex_count);
    c->indices_host.assign(indices, indices + index_count);
    c->meshes_host.assign(meshes, meshes + mesh_count);
    c->materials_ready = false;  // per-mesh materials belong to the previous scene
    c->light_count     = 0;
    c->light_tris_host.clear();  // (and with them the next-event pair list: rebuilt by the next cap_materials_upload)
    c->vertex_count = vertex_count, c->index_count = index_count, c->mesh_count = mesh_count, c->tri_count = (uint32_t)tri_ids.size();
    c->scene_ready = true;
    c->bvh_ready   = false;
    c->bvh_stale   = false;
    c->positions_host_stale = false;
    c->lane1_failed_paths = 0;  // another scene, other buffers: a second batch lane that did not fit before may fit now
    c->tri_mask_on = false;     // instance masks belong to the previous scene's meshes
    c->inst_count  = 0;         // ... and the instance table to its trees
    c->obj_count   = 0;         // ... and the object table to its mesh table
    c->pn_ready    = false;     // ... and the pseudonormal table to its triangles
    c->pn_table.release();
    c->wn_ready    = false;     // ... and the dipole table to its tree
    c->wn_table.release();
    winding_instances_release(c);
    return CAP_OK;
}

int cap_scene_set_instance_masks(CapContext* c, const uint8_t* masks, uint32_t mesh_count)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_scene_set_instance_masks: ctx is NULL");
    if (!c->scene_ready) return fail(CAP_ERR_STATE, "cap_scene_set_instance_masks: no scene uploaded");
    if (mesh_count != c->mesh_count)
        return fail(CAP_ERR_INVALID_ARG, "cap_scene_set_instance_masks: mesh_count %u is not the uploaded scene's (%u)", mesh_count, c->mesh_count);
    bool all = true;
    for (uint32_t m = 0; masks && m < mesh_count; ++m) all = all && masks[m] == 0xFFu;
    if (all)
    {
        c->tri_mask_on = false;  // host state: the queries that follow take the plain kernels; those enqueued keep the table they were given
        return CAP_OK;
    }
    // one byte per global triangle id (mesh-table order, then primitive order: the ids of cap_scene_upload)
    std::vector<uint8_t> bytes;
    bytes.reserve(c->tri_count);
    for (uint32_t m = 0; m < mesh_count; ++m) bytes.insert(bytes.end(), c->meshes_host[m].index_count / 3, masks[m]);
    HIP_TRY(hipSetDevice(c->device));
    if (c->tri_mask.n < bytes.size())
    {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (a grown buffer replaces one an earlier query may still be reading)
        HIP_TRY(c->tri_mask.ensure(bytes.size()));
    }
    // ordered on the context stream behind every query enqueued; the host bytes may go once the call returns
    if (!bytes.empty())
    {
        HIP_TRY(hipMemcpyAsync(c->tri_mask.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->tri_mask_on = true;
    return CAP_OK;
}

int cap_texture_upload(CapContext* c, uint32_t index, const uint8_t* rgba8, uint32_t width, uint32_t height)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_texture_upload: ctx is NULL");
    ++c->scene_generation;  // (the camera-vertex table of an earlier cap_render no longer stands for the scene: CameraTableKey)
    if (index >= 1024) return fail(CAP_ERR_INVALID_ARG, "texture index %u exceeds the reference's 1024-entry table", index);
    static const uint8_t zero_texel[4] = {0, 0, 0, 0};  // texture_system.cpp:47-56
    if (!rgba8) rgba8 = zero_texel, width = height = 1;
    if (!width || !height) return fail(CAP_ERR_INVALID_ARG, "texture %u: empty extent", index);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->texture_host.size() <= index)
    {
        const size_t old = c->texture_host.size();
        c->texture_data.resize(index + 1);
        c->texture_host.resize(index + 1);
        for (size_t i = old; i <= index; ++i)
        {
            // holes behave like the missing-texture texel
            static const uint8_t zero_quad[16] = {0};
            HIP_TRY(c->texture_data[i].ensure(16));
            HIP_TRY(hipMemcpy(c->texture_data[i].p, zero_quad, 16, hipMemcpyHostToDevice));
            c->texture_host[i] = TextureDev{reinterpret_cast<const uint4*>(c->texture_data[i].p), 1, 1};
        }
    }
    // stored as the bilinear footprint of every texel: (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1) with WRAP, four RGBA8 words --
    // expanded on the device from the plain image (4 bytes per texel cross the bus, not 16)
    const size_t texels = (size_t)width * height;
    c->texture_data[index].release();
    HIP_TRY(c->texture_data[index].ensure(16 * texels));
    DevBuf<uint8_t> plain;
    HIP_TRY(plain.ensure(4 * texels));
    HIP_TRY(hipMemcpy(plain.p, rgba8, 4 * texels, hipMemcpyHostToDevice));
    launch_texture_footprints(c->stream, reinterpret_cast<const uint32_t*>(plain.p), reinterpret_cast<uint4*>(c->texture_data[index].p), width, height);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    plain.release();
    c->texture_host[index] = TextureDev{reinterpret_cast<const uint4*>(c->texture_data[index].p), width, height};
    c->textures_dirty = true;
    return CAP_OK;
}

int cap_bluenoise_upload(CapContext* c, const uint8_t* rgba8)
{
    if (!c || !rgba8) return fail(CAP_ERR_INVALID_ARG, "cap_bluenoise_upload: NULL argument");
    std::vector<float2> lut(256 * 256);
    for (size_t i = 0; i < lut.size(); ++i) lut[i] = make_float2((float)rgba8[4 * i] / 255.0f, (float)rgba8[4 * i + 1] / 255.0f);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->bluenoise.ensure(lut.size()));
    HIP_TRY(hipMemcpy(c->bluenoise.p, lut.data(), sizeof(float2) * lut.size(), hipMemcpyHostToDevice));
    // EXT: the B and A channels feed the extra random numbers of the EXT shading model (lobe choice, light triangle)
    for (size_t i = 0; i < lut.size(); ++i) lut[i] = make_float2((float)rgba8[4 * i + 2] / 255.0f, (float)rgba8[4 * i + 3] / 255.0f);
    HIP_TRY(c->bluenoise_ba.ensure(lut.size()));
    HIP_TRY(hipMemcpy(c->bluenoise_ba.p, lut.data(), sizeof(float2) * lut.size(), hipMemcpyHostToDevice));
    c->bluenoise_ready = true;
    return CAP_OK;
}

int cap_materials_upload(CapContext* c, const CapMaterial* materials, uint32_t mesh_count)
{
    if (!c || (!materials && mesh_count)) return fail(CAP_ERR_INVALID_ARG, "cap_materials_upload: NULL argument");
    ++c->scene_generation;  // (the camera-vertex table of an earlier cap_render no longer stands for the scene: CameraTableKey)
    if (!c->scene_ready || mesh_count != c->mesh_count) return fail(CAP_ERR_STATE, "cap_materials_upload: expected %u materials (one per mesh)", c->mesh_count);
    c->materials_host.assign(materials, materials + mesh_count);
    c->materials_ready = false;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->materials.ensure(mesh_count));
    if (mesh_count) HIP_TRY(hipMemcpy(c->materials.p, materials, sizeof(CapMaterial) * mesh_count, hipMemcpyHostToDevice));
    if (const int rc = upload_light_table(c)) return rc;
    c->materials_ready = true;
    if (c->bvh_ready && !c->bvh_stale) return update_nee_pairs(c);  // (a stale tree gets its list from cap_bvh_refit / cap_bvh_build)
    return CAP_OK;
}
}  // extern "C"

namespace cap
{
// Exhaustive path (cap_set_traversal): triangles that come in fans (k, k + 1 share v0 and the edge v0->v2, as every
// triangulated quad of an OBJ face does) are stored as one record, so the kernels compute tvec, q and the shared edge's dot
// product once for both.  Same per-triangle arithmetic, same results; the pairing only depends on bit-equal vertices.
// BvhDev::tri_ids_dense: a triangle's id is its position in the pair list.  (No triangles: nothing to walk, not dense.)
bool pair_ids_dense(const float* pairs, uint32_t pair_count, uint32_t single_count, uint32_t tri_count)
{
    if (!tri_count || single_count || tri_count != 2u * (uint64_t)pair_count) return false;
    for (uint32_t j = 0; j < pair_count; ++j)
    {
        uint32_t id;
        memcpy(&id, pairs + 20 * (size_t)j + 18, sizeof(id));
        if (id != 2u * j) return false;
    }
    return true;
}

int upload_fan_records(CapContext* c)
{
    const uint32_t n = c->tri_count;
    c->fan_pair_count = c->fan_single_count = 0;
    c->tri_ids_dense = 0;
    if (n && n <= 4096)
    {
        std::vector<float> raw(16 * (size_t)n);
        HIP_TRY(hipMemcpy(raw.data(), c->tri_raw.p, sizeof(float) * raw.size(), hipMemcpyDeviceToHost));
        std::vector<float> pairs, singles;
        auto rec = [&](uint32_t k) { return raw.data() + 16 * (size_t)k; };  // v0(3) e1(3) e2(3) n(3) id(1) pad(3)
        for (uint32_t k = 0; k < n;)
        {
            const float* a = rec(k);
            const float* b = k + 1 < n ? rec(k + 1) : nullptr;
            const bool   fan = b && memcmp(a, b, 12) == 0 && memcmp(a + 6, b + 3, 12) == 0;  // same v0, e2(k) == e1(k+1)
            if (fan)
            {
                // (v0, e1, e2, e3 = e2 of k+1, nA, nB, id of k, 0)
                const float r[20] = {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], b[6], b[7], b[8], a[9], a[10], a[11],
                                     b[9], b[10], b[11], a[12], 0.0f};
                pairs.insert(pairs.end(), r, r + 20);
                k += 2;
            }
            else
            {
                singles.insert(singles.end(), a, a + 16);
                k += 1;
            }
        }
        c->fan_pair_count   = (uint32_t)(pairs.size() / 20);
        c->fan_single_count = (uint32_t)(singles.size() / 16);
        c->tri_ids_dense    = pair_ids_dense(pairs.data(), c->fan_pair_count, c->fan_single_count, n) ? 1u : 0u;
        // padded by four records so that an unrolled scalar load past the end stays inside the allocation
        pairs.resize(pairs.size() + 80, 0.0f), singles.resize(singles.size() + 64, 0.0f);
        c->fan_pairs_host   = pairs;
        HIP_TRY(c->fan_pairs.ensure(pairs.size() / 4));
        HIP_TRY(c->fan_singles.ensure(singles.size() / 4));
        HIP_TRY(hipMemcpy(c->fan_pairs.p, pairs.data(), sizeof(float) * pairs.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->fan_singles.p, singles.data(), sizeof(float) * singles.size(), hipMemcpyHostToDevice));
    }
    if (c->fan_pair_count == 0) c->fan_pairs_host.clear();
    return CAP_OK;
}

// EXT model, next-event rays on the small-scene path: which fan pairs can occlude a segment from a scene point p to a point y of a light
// triangle?  The fused kernel tests every pair for every such ray (an OR without an early exit, 8.3 of the 31 ms of BASELINE's literal
// "Lambert+GGX" step, docs/experiments.md (48)); a pair that provably never reports an occlusion is moved behind the count that loop runs to.
//
// Rule (in double, over the vertices as uploaded).  A pair is left out iff for BOTH of its triangles, with plane (v0, n):
//   (i)  every scene vertex lies on one closed side of the plane, at most eps = 2.5e-7 * Dv beyond it (Dv = the largest distance from
//        v0 to a scene vertex): the plane supports the scene's convex hull to within eps, so p (a convex combination of scene vertices)
//        is at most eps outside it;
//   (ii) every vertex of every light triangle is at least delta = 1e-2 * D * Dv inside it, D = the scene's diagonal (numbers in scene
//        units: the bound is against the contract's ABSOLUTE tmin = 1e-4).
// Why that is exact under the intersection contract, whose occlusion test is  tmin * det < T < tmax * det  with
// T = +-(p - v0).n, det = |d.n|, d the unit direction, tmax = 0.999 |y - p|:  in exact arithmetic the segment meets the plane at t* =
// T / det, and with both ends on the inner side t* <= 0 or t* >= |y - p| + delta / sin(theta) (theta = the angle between d and the plane),
// never inside (tmin, tmax).  A p that is s <= eps OUTSIDE the plane crosses it on its way in, at t* = s |y - p| / (s + h) with h >= delta
// the light point's depth: t* <= eps D / delta = 2.5e-5, a quarter of tmin.  (eps was 1e-6 D until the tests built the case: a decal
// 1e-6 D outside a wall whose Dv is half the room, segments 1.5 Dv long, t* = 1.5e-4 -- inside the interval, where the wall, culled,
// cannot shadow the decal next to its edge; tests/pair_cull_support.py nee_truth, tests/test_pair_culls_gpu.py N3.)
// The computed T differs from the exact one by at most ~4 ulp of |p - v0| |n| (a three-term fma chain on a
// difference that is exact to an ulp; p itself is off its surface by as much): |t_computed - t*| <= 2.4e-7 |p - v0| / sin(theta) --
// the classic grazing-ray blow-up ((25), (64) of docs/experiments.md closed two earlier culls over it).  (ii) bounds the grazing angle:
// sin(theta) >= delta / |y - p| >= delta / D, so the error is below 2.4e-7 * Dv * D / delta = 2.4e-5, a quarter of tmin on the near side
// (t* <= 2.5e-5 stays below tmin) and nothing against the 1e-3 |y - p| + delta between tmax and t* on the far side.  The ceiling of the
// Cornell box (its lamp hangs 1 cm below it: rays from the ceiling's rim to the lamp graze it) fails (ii) and stays in the list, as
// does every pair that is not a hull face.  tests: the EXT parity tests run this list; `tools/build_variant.sh neecheck -DCAP_NEE_CHECK`
// runs both lists on every ray and counts disagreements in CapStats::guard_shade (0 over BASELINE configs[2]'s 8 G next-event rays).
int update_nee_pairs(CapContext* c)
{
    c->fan_pair_nee_count = c->fan_pair_count;
    c->fan_pairs_nee.release();
    const uint32_t np = c->fan_pair_count;
    if (!np || !c->materials_ready || c->light_tris_host.empty() || c->fan_pairs_host.size() < 20 * (size_t)np || c->sw.on(SW_NO_NEE_PAIR_CULL)) return CAP_OK;
    if (const int rc = ensure_positions_host(c)) return rc;
    const size_t nv = c->positions_host.size() / 3;
    if (!nv) return CAP_OK;
    auto P = [&](size_t i, int k) { return (double)c->positions_host[3 * i + k]; };
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (size_t i = 0; i < nv; ++i)
        for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], P(i, k)), hi[k] = std::max(hi[k], P(i, k));
    const double D = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    if (!(D > 0.0)) return CAP_OK;
    // the light triangles' vertices (global triangle id -> mesh -> indices, as cap_materials_upload walks them)
    std::vector<double> lv;
    {
        uint32_t g = 0;
        size_t   li = 0;
        for (uint32_t m = 0; m < c->mesh_count && li < c->light_tris_host.size(); ++m)
        {
            const CapMeshDesc& d = c->meshes_host[m];
            for (uint32_t k = 0; k + 2 < d.index_count + 0u && li < c->light_tris_host.size(); k += 3, ++g)
            {
                if (c->light_tris_host[li] != g) continue;
                ++li;
                for (int j = 0; j < 3; ++j)
                {
                    const uint32_t vi = d.first_vertex_offset + c->indices_host[d.first_index_offset + k + j];
                    for (int x = 0; x < 3; ++x) lv.push_back(P(vi, x));
                }
            }
        }
        if (li != c->light_tris_host.size()) return CAP_OK;  // (cannot happen: the ids come from the same walk) -- keep every pair
    }
    std::vector<uint8_t> skip(np, 0);
    uint32_t             n_skip = 0;
    for (uint32_t k = 0; k < np; ++k)
    {
        const float* r  = c->fan_pairs_host.data() + 20 * (size_t)k;
        const double v0[3] = {r[0], r[1], r[2]};
        bool         ok = true;
        for (int t = 0; t < 2 && ok; ++t)
        {
            const double n[3] = {r[12 + 3 * t], r[13 + 3 * t], r[14 + 3 * t]};
            const double nl   = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(nl > 0.0))
            {
                ok = false;
                break;
            }
            double smin = 0.0, smax = 0.0, dv = 0.0;
            for (size_t i = 0; i < nv; ++i)
            {
                const double e[3] = {P(i, 0) - v0[0], P(i, 1) - v0[1], P(i, 2) - v0[2]};
                const double sd   = (e[0] * n[0] + e[1] * n[1] + e[2] * n[2]) / nl;
                smin = std::min(smin, sd), smax = std::max(smax, sd);
                dv   = std::max(dv, std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
            }
            const double tol = 2.5e-7 * dv;  // (i): t* of a point this far outside stays below tmin / 4, see above
            double       sign;
            if (smax <= tol)
                sign = -1.0;  // the scene lies on the negative side
            else if (smin >= -tol)
                sign = 1.0;
            else
            {
                ok = false;
                break;
            }
            const double delta = 1e-2 * D * dv;
            for (size_t i = 0; i + 2 < lv.size() && ok; i += 3)
            {
                const double sd = ((lv[i] - v0[0]) * n[0] + (lv[i + 1] - v0[1]) * n[1] + (lv[i + 2] - v0[2]) * n[2]) / nl;
                if (!(sign * sd >= delta)) ok = false;
            }
        }
        skip[k] = ok ? 1 : 0;
        n_skip += ok ? 1u : 0u;
    }
    if (!n_skip) return CAP_OK;
    std::vector<float> list;
    list.reserve(c->fan_pairs_host.size());
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t k = 0; k < np; ++k)
            if ((int)skip[k] == pass) list.insert(list.end(), c->fan_pairs_host.begin() + 20 * (size_t)k, c->fan_pairs_host.begin() + 20 * (size_t)(k + 1));
    list.resize(c->fan_pairs_host.size(), 0.0f);  // the same zero padding records behind the list
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->fan_pairs_nee.ensure(list.size() / 4));
    HIP_TRY(hipMemcpy(c->fan_pairs_nee.p, list.data(), sizeof(float) * list.size(), hipMemcpyHostToDevice));
    c->fan_pair_nee_count = np - n_skip;
    return CAP_OK;
}

// positions_host after a device-side vertex update: read back once, and only when the light table or the next-event pair list needs it
// (a large scene without lights does not pay a device-to-host copy per refit)
int ensure_positions_host(CapContext* c)
{
    if (!c->positions_host_stale) return CAP_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->positions_host.resize(3 * (size_t)c->vertex_count);
    if (c->vertex_count)
        HIP_TRY(hipMemcpy(c->positions_host.data(), c->positions.p, sizeof(float) * c->positions_host.size(), hipMemcpyDeviceToHost));
    c->positions_host_stale = false;
    return CAP_OK;
}

// Light table of the EXT model: emissive triangles in global triangle order with float prefix sums of their areas
// (area = |e1 x e2| / 2 with the arithmetic of cap_math.h, so the table is the one the oracle builds).  From materials_host and the
// current vertices: cap_materials_upload and cap_bvh_refit.
int upload_light_table(CapContext* c)
{
    const CapMaterial* materials = c->materials_host.data();
    bool               any = false;
    for (uint32_t m = 0; m < c->mesh_count; ++m) any = any || materials[m].ke[0] > 0.0f || materials[m].ke[1] > 0.0f || materials[m].ke[2] > 0.0f;
    if (any)
        if (const int rc = ensure_positions_host(c)) return rc;
    std::vector<uint32_t> light_tris;
    std::vector<float>    light_cdf;
    float                 area = 0.0f;
    uint32_t              g    = 0;
    for (uint32_t m = 0; m < c->mesh_count; ++m)
    {
        const CapMeshDesc& d  = c->meshes_host[m];
        const CapMaterial& mt = materials[m];
        const bool         emissive = mt.ke[0] > 0.0f || mt.ke[1] > 0.0f || mt.ke[2] > 0.0f;
        for (uint32_t k = 0; k + 2 < d.index_count; k += 3, ++g)
        {
            if (!emissive) continue;
            v3 p[3];
            for (int j = 0; j < 3; ++j)
            {
                const uint32_t vi = d.first_vertex_offset + c->indices_host[d.first_index_offset + k + j];
                p[j]              = mk3(c->positions_host[3 * vi], c->positions_host[3 * vi + 1], c->positions_host[3 * vi + 2]);
            }
            area = area + 0.5f * length3(cross3(p[1] - p[0], p[2] - p[0]));
            light_tris.push_back(g);
            light_cdf.push_back(area);
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->light_tris.ensure(light_tris.size()));
    HIP_TRY(c->light_cdf.ensure(light_cdf.size()));
    if (!light_tris.empty())
    {
        HIP_TRY(hipMemcpy(c->light_tris.p, light_tris.data(), sizeof(uint32_t) * light_tris.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->light_cdf.p, light_cdf.data(), sizeof(float) * light_cdf.size(), hipMemcpyHostToDevice));
    }
    c->light_count     = (uint32_t)light_tris.size();
    c->light_area      = area;
    c->light_tris_host = light_tris;
    return CAP_OK;
}
}  // namespace cap
