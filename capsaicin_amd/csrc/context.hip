// context.hip — the context behind the C ABI of include/capsaicin_hip.h: creation and destruction, settings, cap_debug_*, accumulation,
// readback, statistics, tiles, and the helpers the other units share (error reporting, sync_and_collect, the device views of the
// camera, the scene and the tree).
//
// The product path is HIP only: every entry point that needs the GPU fails with CAP_ERR_HIP when no device or
// kernel is available; there is no CPU fallback.
//
// The rest of the ABI by role: ctx_render.hip (cap_render: plan, lanes, batches), ctx_scene.hip (uploads, light table), ctx_bvh.hip (builds,
// refit, objects, instances), ctx_query.hip (ray queries), ctx_post.hip (reconstruction chain), ctx_comm.hip (RCCL frame exchange);
// cap_context.h is what they share.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cap_context.h"
#include "cap_near.h"
#include "cap_wide.h"
#include "query_ranges.h"

namespace
{
thread_local std::string g_error;
}  // namespace

namespace cap
{
int fail(int code, const char* fmt, ...)
{
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

int sync_and_collect(CapContext* c)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto& sp : c->spans)
    {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess)
        {
            for (int stage : {sp.stage, sp.also})
                switch (stage)
                {
                case ST_PRIMARY: c->stats.ms_primary += ms; break;
                case ST_CLOSEST: c->stats.ms_trace_closest += ms; break;
                case ST_ANY: c->stats.ms_trace_any += ms; break;
                case ST_SHADE: c->stats.ms_shade += ms; break;
                case ST_RESOLVE: c->stats.ms_resolve += ms; break;
                case ST_POST: c->stats.ms_post += ms; break;
                case ST_COUNT: c->stats.ms_total += ms; break;
                case ST_DIRECT: c->stats.ms_direct += ms; break;
                default:
                    if (stage >= ST_POST_PASS0 && stage < ST_POST_PASS0 + 5) c->stats.ms_post_pass[stage - ST_POST_PASS0] += ms;
                }
        }
        c->event_pool.push_back(sp.a);
        c->event_pool.push_back(sp.b);
    }
    c->spans.clear();
    for (auto& m : c->post_marks)
    {
        for (int pass = 0; pass < 5; ++pass)
        {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, m[pass], m[pass + 1]) == hipSuccess) c->stats.ms_post_pass[pass] += ms, c->stats.ms_post += ms;
        }
        for (hipEvent_t e : m) c->event_pool.push_back(e);
    }
    c->post_marks.clear();
    for (auto& pc : c->pending)
    {
        const bool   queued = pc.second.shadow_queued;
        const size_t per = CounterLayout::per_queue();
        for (uint32_t b = 0; b <= pc.second.num_bounces; ++b)
            for (uint32_t k = 0; k < kQueueClasses; ++k)
            {
                c->stats.rays_extension += pc.first[b * per + k * kCounterStride];
                c->stats.rays_shadow += pc.first[b * per + k * kCounterStride + 1];
                if (queued) c->stats.shadow_entries += pc.first[b * per + k * kCounterStride + 1];
                if (b == 0)
                {
                    c->stats.rays_extension_bounce0 += pc.first[k * kCounterStride];
                    c->stats.rays_shadow_bounce0 += pc.first[k * kCounterStride + 1];
                    if (queued) c->stats.shadow_entries_bounce0 += pc.first[k * kCounterStride + 1];
                }
                // word 2: shadow rays the producer's probe answered (rays, though never queue entries); word 3: shaded vertices
                c->stats.rays_shadow += pc.first[b * per + k * kCounterStride + 2];
                if (b == 0) c->stats.rays_shadow_bounce0 += pc.first[k * kCounterStride + 2];
                c->stats.shaded_vertices += pc.first[b * per + k * kCounterStride + 3];
            }
        c->pinned_pool.push_back(pc.first);
    }
    c->pending.clear();
    if (c->pinned_shaded && c->shaded_counter.p)
    {
        HIP_TRY(hipMemcpy(c->pinned_shaded, c->shaded_counter.p, kGuardWords * sizeof(uint64_t), hipMemcpyDeviceToHost));
        c->stats.guard_shade     = c->pinned_shaded[1];
        c->stats.guard_trace_any = c->pinned_shaded[2];
        c->stats.guard_last      = c->pinned_shaded[3];
        c->stats.guard_append    = c->pinned_shaded[4];
    }
    return CAP_OK;
}

hipEvent_t get_event(CapContext* c)
{
    if (!c->event_pool.empty())
    {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

CameraDev camera_dev(const CapCameraData& cd)
{
    CameraDev d{};
    for (int k = 0; k < 3; ++k) d.position[k] = cd.position[k], d.right[k] = cd.right[k], d.forward[k] = cd.forward[k], d.up[k] = cd.up[k];
    d.focal_length = cd.focal_length;
    d.sensor_x     = cd.sensor_size[0];
    d.sensor_y     = cd.sensor_size[1];
    return d;
}

SceneDev scene_dev(const CapContext* c)
{
    SceneDev s{};
    s.shade_tris    = c->shade_tris.p;
    s.tri_ids       = c->tri_ids.p;
    s.mesh_texture  = c->mesh_texture.p;
    s.textures      = c->textures.p;
    s.texture_count = (uint32_t)c->texture_host.size();
    s.bluenoise     = c->bluenoise.p;
    s.kd_untextured = pow22_c(0.75f);
    s.shade_tame    = c->shade_tame ? 1u : 0u;
    s.bluenoise_ba  = c->bluenoise_ba.p;
    s.materials     = reinterpret_cast<const MaterialDev*>(c->materials.p);
    s.material_count = c->materials_ready ? c->mesh_count : 0u;
    s.light_tris    = c->light_tris.p;
    s.light_cdf     = c->light_cdf.p;
    s.light_count   = c->light_count;
    s.light_area    = c->light_area;
    return s;
}

// the tree view of a launch whose traversal stacks spill into `lane`'s area
BvhDev bvh_dev(const CapContext* c, const CapContext::Lane& lane)
{
    BvhDev b{};
    b.nodes     = c->nodes.p;
    b.tris      = c->tris_sorted.p;
    b.tris_by_id = c->tri_raw.p;
    b.stack_spill   = lane.stack_spill.p;
    b.spill_threads = (uint32_t)(lane.stack_spill.n / kSpillEntries);
    // A/B switch: the binary-tree kernels (also what runs if the 8-wide view's depth ever exceeds the pair stacks)
    const bool no_wide8 = c->sw.on(SW_NO_WIDE8);
    b.nodes8 = c->nodes8.p, b.tris8 = c->tris8.p;
    b.wide8_ok  = !no_wide8 && lane.stack_spill.p && c->wide8_nodes != 0 && c->wide8_depth <= wide8_stack_pairs() + 1u &&
                 c->wide8_depth <= kWideLdsEntries / 2u + kSpillEntries / 2u + 1u &&
                 (c->debug_wide_depth_limit == 0u || c->wide8_depth <= c->debug_wide_depth_limit);
    b.wide8_top = c->wide8_top;
    b.fan_pairs = c->fan_pairs.p, b.fan_singles = c->fan_singles.p;
    b.fan_pair_count = c->fan_pair_count, b.fan_single_count = c->fan_single_count;
    b.tri_ids_dense = c->tri_ids_dense;
    b.fan_pairs_nee = c->fan_pairs_nee.p ? c->fan_pairs_nee.p : c->fan_pairs.p;
    b.fan_pair_nee_count = c->fan_pairs_nee.p ? c->fan_pair_nee_count : c->fan_pair_count;
    b.tri_count = c->tri_count;
    b.root      = c->tri_count >= 2 ? 0 : ~0;
    return b;
}

AovPlanes aov_planes(const CapContext* c)
{
    const size_t off = (size_t)(c->last_slots ? c->last_slots - 1 : 0) * c->screen.pixels_padded;
    return AovPlanes{c->lane[0].pl_color.p + off, c->lane[0].pl_direct.p + off, c->lane[0].pl_albedo.p + off};
}

// CAP_TRACE_LAUNCHES=1: name every launch on stderr and drain the stream after it (fault localisation only)
int trace_launch(const CapContext* c, const char* fmt, ...)
{
    if (!c->sw.on(SW_TRACE_LAUNCHES)) return CAP_OK;
    va_list ap;
    va_start(ap, fmt);
    fputs("[cap] ", stderr);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputs(" ... ", stderr);
    fflush(stderr);
    hipError_t e = hipStreamSynchronize(c->stream);
    fprintf(stderr, "%s\n", hipGetErrorString(e));
    fflush(stderr);
    return e == hipSuccess ? CAP_OK : CAP_ERR_HIP;
}
}  // namespace cap

namespace
{
void update_screen(CapContext* c, uint32_t w, uint32_t h, uint32_t shard_index, uint32_t shard_count)
{
    ScreenDev& s  = c->screen;
    s.width       = w;
    s.height      = h;
    s.tiles_x     = (w + kTileDim - 1) / kTileDim;
    s.tiles_y     = (h + kTileDim - 1) / kTileDim;
    s.tile_count  = s.tiles_x * s.tiles_y;
    s.shard_index = shard_index;
    s.shard_count = shard_count ? shard_count : 1;
    const uint32_t max_local = (s.tile_count + s.shard_count - 1) / s.shard_count;
    s.local_tiles   = s.tile_count > s.shard_index ? (s.tile_count - s.shard_index + s.shard_count - 1) / s.shard_count : 0;
    s.pixels_padded = max_local * kTilePixels;
    tile_div_setup(s.tiles_x, s.tiles_x_mul, s.tiles_x_shift);
    c->frames_accumulated = 0;
    c->aov_valid = false;
}

// Launches something that counts into N zeroed 64-bit words on the context's stream and waits for them: h = the words.  (cap_debug_get's
// self-tests and canary count; the buffer is released on every path: ADVICE r5)
template <size_t N, class Launch>
int count_on_device(CapContext* c, unsigned long long (&h)[N], Launch launch)
{
    DevBuf<unsigned long long> d;
    HIP_TRY(d.ensure(N));
    HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(h), c->stream));
    launch(d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CAP_OK;
}
}  // namespace

// (x, y) -> the four RGBA8 words a bilinear WRAP sample at that texel reads (cap_device.h TextureDev)
__global__ __launch_bounds__(256) void k_texture_footprints(const uint32_t* src, uint4* dst, uint32_t width, uint32_t height)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)width * height) return;
    const uint32_t y = (uint32_t)(i / width), x = (uint32_t)(i - (size_t)y * width);
    const uint32_t x1 = x + 1 == width ? 0 : x + 1, y1 = y + 1 == height ? 0 : y + 1;
    dst[i] = make_uint4(src[(size_t)y * width + x], src[(size_t)y * width + x1], src[(size_t)y1 * width + x], src[(size_t)y1 * width + x1]);
}

void cap::launch_texture_footprints(hipStream_t stream, const uint32_t* src, uint4* dst, uint32_t width, uint32_t height)
{
    const size_t texels = (size_t)width * height;
    hipLaunchKernelGGL(k_texture_footprints, dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, stream, src, dst, width, height);
}

extern "C" {

const char* cap_last_error(void) { return g_error.c_str(); }
// used by the host-side half of the library (obj_loader.cpp) so both report through cap_last_error()
void cap_set_error_(const char* msg) { g_error = msg ? msg : ""; }

int cap_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The switches' names: environment variables read ONCE, at cap_ctx_create (tools and profiling scripts set them around a whole process),
// and the strings cap_debug_switch_index() resolves for cap_debug_set.  A presence flag counts as set unless its value is "0".
static const char* const kSwitchNames[SW_COUNT] = {
    "CAP_NO_WIDE8", "CAP_LANE1_PRIORITY", "CAP_PLOC_RADIUS", "CAP_SAHDEV_LEAF", "CAP_WIDE_HOST_COLLAPSE", "CAP_TRACE_LAUNCHES", "CAP_NO_TWO_LANES",
    "CAP_LANE_SPLIT_MIN", "CAP_BLOCKS_PER_CU", "CAP_NO_CAMERA_CULL", "CAP_NO_ALBEDO_IN_W", "CAP_NO_INLINE_NEE", "CAP_NO_INLINE_PROBE", "CAP_NO_WAVE_RING",
    "CAP_ANY_REFILL", "CAP_PRIMARY_WIDE", "CAP_NO_PACKET", "CAP_NO_ANY_PROBE", "CAP_ANY_PROBE", "CAP_ANY_BLOCKS", "CAP_NO_PRIMARY_FUSE", "CAP_W8_REFILL",
    "CAP_W8_GRID", "CAP_AUTO_SAH_TRIANGLES", "CAP_NO_NEE_PAIR_CULL", "CAP_RAYGEN_KERNEL", "CAP_NO_PLANE_CODE", "CAP_SAMPLE_TABLE", "CAP_NO_CAMERA_TABLE",
    "CAP_NO_GRAY_ENTRIES", "CAP_NO_GROUP_WALK", "CAP_NO_TABLE_REUSE", "CAP_NO_SKY_PLANE"};

static void switches_from_environment(SwitchTable& t)
{
    for (uint32_t k = 0; k < SW_COUNT; ++k)
    {
        const char* e = getenv(kSwitchNames[k]);
        t.v[k]        = -1;
        if (!e) continue;
        char*           end = nullptr;
        const long long v   = strtoll(e, &end, 10);
        t.v[k]              = (end != e && v >= 0) ? v : 1;  // "CAP_NO_X=" / "=yes": a set flag
    }
    if (getenv("CAP_BVH_BINARY") && t.v[SW_NO_WIDE8] < 0) t.v[SW_NO_WIDE8] = 1;  // older name of the same switch
}

int cap_debug_switch_index(const char* name)
{
    for (uint32_t k = 0; name && k < SW_COUNT; ++k)
        if (strcmp(name, kSwitchNames[k]) == 0) return (int)k;
    return -1;
}

// Host-callable check of tile_div() (cap_device.h), the division by tiles_x of the small-scene kernels' bounce >= 1 plumbing: quotient
// and remainder of n[k] / tiles_x by the multiplier and shift update_screen() stores, the remainder by the kernel's gt - ty * tiles_x.
// No context, no device: tests/test_tile_div.py compares it with // and % (like cap_debug_stamps, not part of the declared ABI).
extern "C" int cap_debug_tile_divmod(uint32_t tiles_x, const uint32_t* n, uint64_t count, uint32_t* quotient, uint32_t* remainder)
{
    if (!tiles_x || !n || !quotient || !remainder) return CAP_ERR_INVALID_ARG;
    uint32_t mul, shift;
    tile_div_setup(tiles_x, mul, shift);
    for (uint64_t k = 0; k < count; ++k)
    {
        quotient[k]  = tile_div(n[k], mul, shift);
        remainder[k] = n[k] - quotient[k] * tiles_x;
    }
    return CAP_OK;
}

// head_chunk() (cap_device.h), the head kernels' mapping of bounce 0's chunk indices, for tests/test_group_walk.py.  No device.
int cap_debug_head_chunk(uint32_t cps, uint32_t m, const uint8_t* order, uint32_t n_slots, const uint32_t* c, uint64_t count, uint32_t* slot,
                         uint32_t* group64)
{
    if (!order || !c || !slot || !group64 || !m || !cps || n_slots > kMaxFrameSlots || n_slots % m != 0u || (uint64_t)cps * n_slots > (1ull << kTileDivBits))
        return CAP_ERR_INVALID_ARG;
    const HeadWalk w = head_walk(m, cps, order, n_slots);
    for (uint64_t k = 0; k < count; ++k) head_chunk(w, cps, c[k], slot[k], group64[k]);
    return CAP_OK;
}

// The rule behind upload_fan_records' dense bit (ctx_scene.hip pair_ids_dense), for tests/test_pair_carry.py.  No device.
int cap_debug_pair_ids_dense(const float* pair_records, uint32_t pair_count, uint32_t single_count, uint32_t tri_count)
{
    if (!pair_records && pair_count) return 0;
    return pair_ids_dense(pair_records, pair_count, single_count, tri_count) ? 1 : 0;
}

// The address checks of the ray-query entry points (query_ranges.h) on `count` ranges of n x stride[i] bytes from base[i], base[i] to be a
// multiple of align[i] (a power of two); stride[i] == 0: the caller left array i out.  CAP_OK, or CAP_ERR_INVALID_ARG with the message the
// entry points give.  No context, no device: tests/test_query_ranges.py.
int cap_debug_query_ranges(uint64_t n, uint32_t count, const uint64_t* base, const uint64_t* stride, const uint32_t* align)
{
    static const char* const names[4] = {"range 0", "range 1", "range 2", "range 3"};
    if (count > 4 || (count && (!base || !stride || !align))) return fail(CAP_ERR_INVALID_ARG, "cap_debug_query_ranges: at most 4 ranges, no NULL array");
    QueryRange r[4];
    for (uint32_t i = 0; i < count; ++i)
    {
        if (!align[i] || (align[i] & (align[i] - 1u))) return fail(CAP_ERR_INVALID_ARG, "cap_debug_query_ranges: align[%u] is not a power of two", i);
        r[i] = QueryRange{names[i], (uintptr_t)base[i], stride[i], align[i], stride[i] != 0};
    }
    char msg[256];
    return query_ranges_ok("cap_debug_query_ranges", n, r, count, msg, sizeof(msg)) ? CAP_OK : fail(CAP_ERR_INVALID_ARG, "%s", msg);
}

// The per-instance data and the skip predicate of cap_closest_instances (cap_near.h: the functions k_instance_setup and k_closest_inst
// run) for one transform, one object-space box, one world point and one best dist2.  No context, no device: tests/test_closest_instances.py.
int cap_debug_closest_instance_bound(const float* transform, const float* box_lo, const float* box_hi, const float* point, float best_dist2,
                                     float* world_to_object, float* g, float* xw, float* slack, uint32_t* skip)
{
    if (!transform || !box_lo || !box_hi || !point) return fail(CAP_ERR_INVALID_ARG, "cap_debug_closest_instance_bound: NULL input");
    double m[12], w[12], wd[12], A[12], nA, kappa, blo[3], bhi[3];
    float  wf[12];
    bool   live = true;
    for (int k = 0; k < 12; ++k) m[k] = (double)transform[k], live = live && finite_d(m[k]);
    for (int k = 0; k < 3; ++k) blo[k] = (double)box_lo[k], bhi[k] = (double)box_hi[k];
    live = instance_inverse(m, live, w, wf, wd, A, nA, kappa, (float)CAP_INSTANCE_MAX_CONDITION);
    const float gi = live ? near_sigma_min_bound(w) : 0.0f, xi = live ? near_world_extent(m, blo, bhi) : 0.0f;
    const float pmax = fmaxf(fabsf(point[0]), fmaxf(fabsf(point[1]), fabsf(point[2])));
    const float sl   = near_slack(pmax, xi);
    float       ox, oy, oz;
    near_to_object(wf, point[0], point[1], point[2], ox, oy, oz);
    const float bd2 = box_dist2(ox, oy, oz, box_lo[0], box_lo[1], box_lo[2], box_hi[0], box_hi[1], box_hi[2]);
    if (world_to_object)
        for (int k = 0; k < 12; ++k) world_to_object[k] = wf[k];
    if (g) *g = gi;
    if (xw) *xw = xi;
    if (slack) *slack = sl;
    // an inert instance is never entered: nothing to skip
    if (skip) *skip = live && near_skip(bd2, near_bound2_object(sqrtf(best_dist2), sl, gi)) ? 1u : 0u;
    return CAP_OK;
}

// The prune of cap_overlap_instances (cap_near.h: the functions k_overlap_inst runs, over the per-instance data of k_instance_setup) for
// one transform, one object box, one world box and one object-space box against one query box.  No context, no device:
// tests/test_overlap_instances.py.
int cap_debug_overlap_instance_prune(const float* transform, const float* object_lo, const float* object_hi, const float* world_lo, const float* world_hi,
                                     const float* node_lo, const float* node_hi, const float* box_lo, const float* box_hi, float* world_to_object, float* g,
                                     float* xw, float* slack, float* image_lo, float* image_hi, uint32_t* skip_top, uint32_t* skip_node)
{
    if (!transform || !object_lo || !object_hi || !world_lo || !world_hi || !node_lo || !node_hi || !box_lo || !box_hi)
        return fail(CAP_ERR_INVALID_ARG, "cap_debug_overlap_instance_prune: NULL input");
    double m[12], w[12], wd[12], A[12], nA, kappa, blo[3], bhi[3];
    float  wf[12];
    bool   live = true;
    for (int k = 0; k < 12; ++k) m[k] = (double)transform[k], live = live && finite_d(m[k]);
    for (int k = 0; k < 3; ++k) blo[k] = (double)object_lo[k], bhi[k] = (double)object_hi[k];
    live = instance_inverse(m, live, w, wf, wd, A, nA, kappa, (float)CAP_INSTANCE_MAX_CONDITION);
    const float gi = live ? near_sigma_min_bound(w) : 0.0f, xi = live ? near_world_extent(m, blo, bhi) : 0.0f;
    // the kernel's frame of the box (overlap.hip box_frame) and its two slacks
    const float hl[3] = {box_lo[0] * 0.5f, box_lo[1] * 0.5f, box_lo[2] * 0.5f}, hh[3] = {box_hi[0] * 0.5f, box_hi[1] * 0.5f, box_hi[2] * 0.5f};
    const float bmax  = overlap_box_max(box_lo[0], box_lo[1], box_lo[2], box_hi[0], box_hi[1], box_hi[2]);
    const float sl    = overlap_slack(bmax, xi);
    float       olo[3] = {0.f, 0.f, 0.f}, ohi[3] = {0.f, 0.f, 0.f};
    if (live) overlap_image(wf, hl[0] + hh[0], hl[1] + hh[1], hl[2] + hh[2], hh[0] - hl[0], hh[1] - hl[1], hh[2] - hl[2], sl / gi, olo, ohi);
    if (world_to_object)
        for (int k = 0; k < 12; ++k) world_to_object[k] = wf[k];
    if (g) *g = gi;
    if (xw) *xw = xi;
    if (slack) *slack = sl;
    for (int k = 0; k < 3; ++k)
    {
        if (image_lo) image_lo[k] = olo[k];
        if (image_hi) image_hi[k] = ohi[k];
    }
    // an inert instance is never entered and has no world box: nothing to skip
    if (skip_top)
        *skip_top = live && overlap_miss(world_lo[0], world_lo[1], world_lo[2], world_hi[0], world_hi[1], world_hi[2], box_lo[0] - sl, box_lo[1] - sl,
                                         box_lo[2] - sl, box_hi[0] + sl, box_hi[1] + sl, box_hi[2] + sl)
                        ? 1u
                        : 0u;
    if (skip_node)
        *skip_node = live && overlap_miss(node_lo[0], node_lo[1], node_lo[2], node_hi[0], node_hi[1], node_hi[2], olo[0], olo[1], olo[2], ohi[0], ohi[1], ohi[2])
                         ? 1u
                         : 0u;
    return CAP_OK;
}

// The bottom-level prune of cap_overlap_triangles_instances (cap_near.h: the functions k_overlap_tri_inst's world_node_step runs) for one
// transform, one object box, one object-space node box and one world query box.  No context, no device:
// tests/test_overlap_triangles_instances.py.
int cap_debug_overlap_world_node(const float* transform, const float* object_lo, const float* object_hi, const float* node_lo, const float* node_hi,
                                 const float* query_lo, const float* query_hi, float* xw, float* slack, float* world_lo, float* world_hi, uint32_t* skip_node)
{
    if (!transform || !object_lo || !object_hi || !node_lo || !node_hi || !query_lo || !query_hi)
        return fail(CAP_ERR_INVALID_ARG, "cap_debug_overlap_world_node: NULL input");
    double m[12], w[12], wd[12], A[12], nA, kappa, blo[3], bhi[3];
    float  wf[12], mf[12];
    bool   live = true;
    for (int k = 0; k < 12; ++k) mf[k] = transform[k], m[k] = (double)transform[k], live = live && finite_d(m[k]);
    for (int k = 0; k < 3; ++k) blo[k] = (double)object_lo[k], bhi[k] = (double)object_hi[k];
    live = instance_inverse(m, live, w, wf, wd, A, nA, kappa, (float)CAP_INSTANCE_MAX_CONDITION);
    const float xi   = live ? near_world_extent(m, blo, bhi) : 0.0f;
    const float bmax = overlap_box_max(query_lo[0], query_lo[1], query_lo[2], query_hi[0], query_hi[1], query_hi[2]);
    const float sl   = live ? overlap_slack(bmax, xi) : 0.0f;
    float       wlo[3] = {0.f, 0.f, 0.f}, whi[3] = {0.f, 0.f, 0.f};
    if (live) overlap_world_box(mf, node_lo[0], node_lo[1], node_lo[2], node_hi[0], node_hi[1], node_hi[2], wlo, whi);
    if (xw) *xw = xi;
    if (slack) *slack = sl;
    for (int k = 0; k < 3; ++k)
    {
        if (world_lo) world_lo[k] = wlo[k];
        if (world_hi) world_hi[k] = whi[k];
    }
    // an inert instance is never entered: nothing to skip
    if (skip_node)
        *skip_node = live && overlap_miss(wlo[0], wlo[1], wlo[2], whi[0], whi[1], whi[2], query_lo[0] - sl, query_lo[1] - sl, query_lo[2] - sl,
                                          query_hi[0] + sl, query_hi[1] + sl, query_hi[2] + sl)
                         ? 1u
                         : 0u;
    return CAP_OK;
}

// The bottom-level prune of cap_sweep_instances (cap_near.h: the functions k_sweep_inst's sweep_world_node_step runs) for one transform,
// one object box, one object-space node box, one sweep (origin, radius, direction, tmax: the tmax word is not read) and one far bound.
// No context, no device: tests/test_sweep_instances.py.
int cap_debug_sweep_instance_prune(const float* transform, const float* object_lo, const float* object_hi, const float* node_lo, const float* node_hi,
                                   const float* sweep, float far_bound, float* xw, float* radius, float* world_lo, float* world_hi, float* entry,
                                   float* exit_padded, uint32_t* skip_node)
{
    if (!transform || !object_lo || !object_hi || !node_lo || !node_hi || !sweep) return fail(CAP_ERR_INVALID_ARG, "cap_debug_sweep_instance_prune: NULL input");
    double m[12], w[12], wd[12], A[12], nA, kappa, blo[3], bhi[3];
    float  wf[12], mf[12];
    bool   live = true;
    for (int k = 0; k < 12; ++k) mf[k] = transform[k], m[k] = (double)transform[k], live = live && finite_d(m[k]);
    for (int k = 0; k < 3; ++k) blo[k] = (double)object_lo[k], bhi[k] = (double)object_hi[k];
    live = instance_inverse(m, live, w, wf, wd, A, nA, kappa, (float)CAP_INSTANCE_MAX_CONDITION);
    const float xi   = live ? near_world_extent(m, blo, bhi) : 0.0f;
    const float omax = fmaxf(fabsf(sweep[0]), fmaxf(fabsf(sweep[1]), fabsf(sweep[2])));
    const float R    = live ? sweep_prune_radius(sweep[3], omax, xi) : 0.0f;
    float       wlo[3] = {0.f, 0.f, 0.f}, whi[3] = {0.f, 0.f, 0.f}, tn = 0.f, xp = 0.f;
    bool        keep = true;
    if (live)
    {
        const SweepRay s{sweep[0], sweep[1], sweep[2], 1.0f / sweep[4], 1.0f / sweep[5], 1.0f / sweep[6], R};
        overlap_world_box(mf, node_lo[0], node_lo[1], node_lo[2], node_hi[0], node_hi[1], node_hi[2], wlo, whi);
        keep = sweep_slab_times(s, wlo[0], wlo[1], wlo[2], whi[0], whi[1], whi[2], far_bound, tn, xp);
    }
    if (xw) *xw = xi;
    if (radius) *radius = R;
    for (int k = 0; k < 3; ++k)
    {
        if (world_lo) world_lo[k] = wlo[k];
        if (world_hi) world_hi[k] = whi[k];
    }
    if (entry) *entry = tn;
    if (exit_padded) *exit_padded = xp;
    // an inert instance is never entered: nothing to skip
    if (skip_node) *skip_node = live && !keep ? 1u : 0u;
    return CAP_OK;
}

int cap_ctx_create(int device_id, void* hip_stream, CapContext** out_ctx)
{
    if (!out_ctx) return fail(CAP_ERR_INVALID_ARG, "cap_ctx_create: out_ctx is NULL");
    *out_ctx = nullptr;
    int n    = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) return fail(CAP_ERR_HIP, "cap_ctx_create: device %d not present (%d HIP devices)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    CapContext* c = new CapContext;
    c->device     = device_id;
    switches_from_environment(c->sw);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->cu_count = prop.multiProcessorCount;
    if (hip_stream)
        c->stream = (hipStream_t)hip_stream;
    else
    {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess)
        {
            delete c;
            return fail(CAP_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
        }
        c->own_stream = true;
    }
    c->lane[0].stream = c->stream;
    (void)hipHostMalloc((void**)&c->pinned_shaded, kGuardWords * sizeof(uint64_t), hipHostMallocDefault);
    update_screen(c, 0, 0, 0, 1);
    *out_ctx = c;
    return CAP_OK;
}

void cap_ctx_destroy(CapContext* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& sp : c->spans)
    {
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    for (auto& pc : c->pending) (void)hipHostFree(pc.first);
    for (auto p : c->pinned_pool) (void)hipHostFree(p);
    if (c->pinned_shaded) (void)hipHostFree(c->pinned_shaded);
    (void)cap_comm_destroy(c);
    for (int k = 0; k < CapContext::kFrameRing; ++k)
    {
        if (c->frames_pinned[k]) (void)hipHostFree(c->frames_pinned[k]);
        if (c->frames_event[k]) (void)hipEventDestroy(c->frames_event[k]);
    }
    if (c->stream2) (void)hipStreamSynchronize(c->stream2), (void)hipStreamDestroy(c->stream2);
    for (hipEvent_t e : {c->lane_ev[0], c->lane_ev[1], c->fork_ev, c->join_ev})
        if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int cap_camera_set(CapContext* c, const CapCameraData* camera)
{
    if (!c || !camera) return fail(CAP_ERR_INVALID_ARG, "cap_camera_set: NULL argument");
    c->camera       = *camera;
    c->camera_ready = true;
    return CAP_OK;
}

int cap_prev_camera_set(CapContext* c, const CapCameraData* camera)
{
    if (!c || !camera) return fail(CAP_ERR_INVALID_ARG, "cap_prev_camera_set: NULL argument");
    c->prev_camera       = *camera;
    c->prev_camera_ready = true;
    return CAP_OK;
}

int cap_set_resolution(CapContext* c, uint32_t width, uint32_t height)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_set_resolution: ctx is NULL");
    if (!width || !height || width > 32768 || height > 32768) return fail(CAP_ERR_INVALID_ARG, "cap_set_resolution: bad extent %ux%u", width, height);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    update_screen(c, width, height, c->screen.shard_index, c->screen.shard_count);
    if ((uint64_t)c->screen.pixels_padded > kPidMask) return fail(CAP_ERR_UNSUPPORTED, "too many pixels per shard");
    c->accum.release();
    c->lane1_failed_paths = 0;
    c->post_w = c->post_h = 0;  // histories restart at the next cap_post_frame
    c->post_last_dst = -1;
    return CAP_OK;
}

int cap_set_shard(CapContext* c, uint32_t shard_index, uint32_t shard_count)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_set_shard: ctx is NULL");
    if (!shard_count || shard_index >= shard_count) return fail(CAP_ERR_INVALID_ARG, "cap_set_shard: bad shard %u of %u", shard_index, shard_count);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    update_screen(c, c->screen.width, c->screen.height, shard_index, shard_count);
    c->accum.release();
    c->lane1_failed_paths = 0;
    return CAP_OK;
}

int cap_set_batch_paths(CapContext* c, uint64_t max_paths)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_set_batch_paths: ctx is NULL");
    c->max_batch_paths = max_paths;
    c->lane1_failed_paths = 0;
    return CAP_OK;
}

// Canary for the append-guard test (tests/test_append_guard_gpu.py): the extension queues' six planes of lane 0 are filled with one
// word; after a render with undersized sub-queues every entry BEHIND the last class's sub-queue must still hold it.  (With 32-byte entries
// the two thr_pid planes are never written: they keep the word throughout, BEHIND stays 0 for them and USED counts the other four.)
constexpr uint32_t kCanaryWord = 0x7fc0da7au;  // (a quiet NaN nobody computes)
__global__ __launch_bounds__(256) void k_canary_count(const uint4* p, size_t begin, size_t end, unsigned long long* out)
{
    unsigned long long n = 0;
    for (size_t i = begin + blockIdx.x * (size_t)256 + threadIdx.x; i < end; i += (size_t)gridDim.x * 256)
    {
        const uint4 v = p[i];
        n += (v.x != kCanaryWord || v.y != kCanaryWord || v.z != kCanaryWord || v.w != kCanaryWord) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(out, n);
}
static int canary_count(CapContext* c, bool behind, uint64_t* value)
{
    CapContext::Lane& L = c->lane[0];
    if (!L.q_org[0].p || !c->last_class_capacity) return fail(CAP_ERR_STATE, "cap_debug_get: no render yet");
    HIP_TRY(hipSetDevice(c->device));
    const size_t       used = std::min((size_t)kQueueClasses * c->last_class_capacity, L.q_org[0].n);
    unsigned long long h[1];
    if (int e = count_on_device(c, h, [&](unsigned long long* d) {
            for (int k = 0; k < 2; ++k)
                for (DevBuf<float4>* b : {&L.q_org[k], &L.q_dir[k], &L.q_thr[k]})
                {
                    const size_t lo = behind ? used : 0, hi = behind ? b->n : used;
                    if (hi > lo) hipLaunchKernelGGL(k_canary_count, dim3(512), dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(b->p), lo, hi, d);
                }
        }))
        return e;
    *value = h[0];
    return CAP_OK;
}

int cap_debug_set(CapContext* c, uint32_t key, uint64_t value)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_debug_set: ctx is NULL");
    switch (key)
    {
    case CAP_DEBUG_QUEUE_CAPACITY_DIV:
        if (value < 1 || value > 1024) return fail(CAP_ERR_INVALID_ARG, "cap_debug_set: capacity divisor %llu not in 1..1024", (unsigned long long)value);
        c->debug_capacity_div = (uint32_t)value;
        return CAP_OK;
    case CAP_DEBUG_WIDE_DEPTH_LIMIT:
        c->debug_wide_depth_limit = (uint32_t)value;
        return CAP_OK;
    case CAP_DEBUG_QUEUE_CANARY_FILL:
        if (!c->lane[0].q_org[0].p) return fail(CAP_ERR_STATE, "cap_debug_set: the queues are allocated by the first cap_render");
        HIP_TRY(hipSetDevice(c->device));
        for (int k = 0; k < 2; ++k)
            for (DevBuf<float4>* b : {&c->lane[0].q_org[k], &c->lane[0].q_dir[k], &c->lane[0].q_thr[k]})
                HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)b->p, (int)kCanaryWord, b->n * 4, c->stream));
        return CAP_OK;
    case CAP_DEBUG_FAIL_LANE1:
        c->debug_fail_lane = value != 0;
        if (!value) c->lane1_failed_paths = 0;  // "memory has been released"
        return CAP_OK;
    default:
        if (key >= CAP_DEBUG_SWITCH_BASE && key < CAP_DEBUG_SWITCH_BASE + SW_COUNT)
        {
            // ~0 = back to the product's choice.  Read at the next build / render: a switch that selects buffers (second lane, rings)
            // takes effect with the next call that sizes them.
            c->sw.v[key - CAP_DEBUG_SWITCH_BASE] = value == ~0ull ? -1 : (int64_t)value;
            return CAP_OK;
        }
        return fail(CAP_ERR_INVALID_ARG, "cap_debug_set: unknown key %u", key);
    }
}

int cap_debug_get(CapContext* c, uint32_t key, uint64_t* value)
{
    if (!c || !value) return fail(CAP_ERR_INVALID_ARG, "cap_debug_get: NULL argument");
    switch (key)
    {
    case CAP_DEBUG_QUEUE_CAPACITY_DIV: *value = c->debug_capacity_div; return CAP_OK;
    case CAP_DEBUG_WIDE_DEPTH_LIMIT: *value = c->debug_wide_depth_limit; return CAP_OK;
    case CAP_DEBUG_FAIL_LANE1: *value = c->debug_fail_lane ? 1u : 0u; return CAP_OK;
    case CAP_DEBUG_LANES_USED: *value = c->lanes_last_render; return CAP_OK;
    case CAP_DEBUG_SELFTEST_DIV:
    {
        HIP_TRY(hipSetDevice(c->device));
        unsigned long long h[3];
        if (int e = count_on_device(c, h, [&](unsigned long long* d) { launch_div_selftest(c->stream, d); })) return e;
        // positive control: every normal float once + 2^30 operand pairs must have been compared
        const unsigned long long expected = (0x7f7fffffull - 0x00800000ull + 1ull) + (1ull << 30);
        if (h[2] != expected) return fail(CAP_ERR_HIP, "cap_debug_get: the division self-test compared %llu of %llu cases", h[2], expected);
        *value = h[0] + h[1];
        return CAP_OK;
    }
    case CAP_DEBUG_SELFTEST_SHADE_UNARY:
    case CAP_DEBUG_SELFTEST_SHADE_DIV2:
    {
        HIP_TRY(hipSetDevice(c->device));
        unsigned long long h[2];
        if (int e = count_on_device(c, h, [&](unsigned long long* d) { launch_shade_forms_selftest(c->stream, d, key == CAP_DEBUG_SELFTEST_SHADE_DIV2 ? 1u : 0u); }))
            return e;
        // positive control: two square roots per normal float from 2^-96 on + 3 special operands, the normalize range [2^-3, 4],
        // x / pi over [0, 2] and f over at least half of it; at least 2^30 pairs inside ortho_vector's guard
        const unsigned long long floats_sqrt = 0x7f7fffffull - ((127ull - 96ull) << 23) + 1ull;
        const unsigned long long least = key == CAP_DEBUG_SELFTEST_SHADE_DIV2 ? (1ull << 30) : 2ull * floats_sqrt + 3ull + (5ull << 23) + 1ull + 0x40000001ull + (8ull << 23);
        if (h[1] < least) return fail(CAP_ERR_HIP, "cap_debug_get: the shading self-test compared %llu of at least %llu cases", h[1], least);
        *value = h[0];
        return CAP_OK;
    }
    case CAP_DEBUG_SHADE_TAME:
        if (!c->bvh_ready || c->bvh_stale) return fail(CAP_ERR_STATE, "cap_debug_get: BVH not built or stale");
        *value = c->shade_tame ? 1u : 0u;
        return CAP_OK;
    case CAP_DEBUG_CAMERA_CULL: *value = c->last_cull_camera_pairs; return CAP_OK;
    case CAP_DEBUG_MARK_FORM:
        if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_debug_get: BVH not built");
        *value = ((uint64_t)c->last_mark_form << 8) | c->tri_ids_dense;
        return CAP_OK;
    case CAP_DEBUG_SAMPLE_TABLE: *value = c->last_sample_table; return CAP_OK;
    case CAP_DEBUG_SELFTEST_SAMPLE_TABLE:
    {
        const CapContext::LastTerms& lt = c->last_terms;
        if (!c->last_sample_table || !lt.frames) return fail(CAP_ERR_STATE, "cap_debug_get: the last cap_render built no sample table");
        HIP_TRY(hipSetDevice(c->device));
        if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
        unsigned long long h[2];
        if (int e = count_on_device(c, h, [&](unsigned long long* d) {
                launch_sample_terms_selftest(c->stream, c->bluenoise.p, lt.frames, lt.n_slots, lt.num_bounces, c->lane[lt.lane].terms.p, d);
            }))
            return e;
        const unsigned long long expected = (unsigned long long)lt.n_slots * lt.num_bounces * 4096ull;
        if (h[1] != expected) return fail(CAP_ERR_HIP, "cap_debug_get: the sample table self-test compared %llu of %llu entries", h[1], expected);
        *value = (h[0] << 32) | (expected >> 12);  // mismatches << 32 | (bounce, slot) rows compared
        return CAP_OK;
    }
    case CAP_DEBUG_CAMERA_TABLE: *value = c->last_camera_table; return CAP_OK;
    case CAP_DEBUG_SELFTEST_CAMERA_TABLE:
    {
        const CapContext::LastCamera& lc = c->last_camera;
        if (!c->last_camera_table || !lc.frames) return fail(CAP_ERR_STATE, "cap_debug_get: the last cap_render built no camera table");
        HIP_TRY(hipSetDevice(c->device));
        if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
        // the launch arguments the table was built with (camera, screen and scene as they are now: ask right after the render)
        ShadeArgs sa{};
        sa.scene = scene_dev(c), sa.cam = camera_dev(c->camera), sa.screen = c->screen, sa.frames = lc.frames, sa.n_slots = lc.n_slots;
        sa.cull_camera_pairs = c->last_cull_camera_pairs;
        LaunchCfg     cfg{c->stream, (uint32_t)c->cu_count * 6u, 0u, (uint32_t)c->cu_count};
        float4* const tab = c->lane[lc.lane].camera.p;
        unsigned long long h[2];
        if (int e = count_on_device(c, h, [&](unsigned long long* d) {
                launch_camera_vertices(cfg, bvh_dev(c, c->lane[lc.lane]), sa, lc.n_slots, tab, tab + (size_t)lc.n_groups * c->screen.pixels_padded, d);
            }))
            return e;
        const unsigned long long expected = (unsigned long long)lc.n_slots * c->screen.pixels_padded;
        if (h[1] != expected) return fail(CAP_ERR_HIP, "cap_debug_get: the camera table self-test compared %llu of %llu entries", h[1], expected);
        *value = (h[0] << 32) | ((uint64_t)lc.n_groups << 16) | lc.n_slots;  // mismatches << 32 | groups << 16 | slots compared
        return CAP_OK;
    }
    case CAP_DEBUG_GROUP_WALK: *value = c->last_group_walk; return CAP_OK;
    case CAP_DEBUG_CAMERA_TABLE_REUSED: *value = c->last_camera_reused; return CAP_OK;
    case CAP_DEBUG_GRAY_ENTRIES: *value = c->last_gray_entries; return CAP_OK;
    case CAP_DEBUG_SKY_PLANE: *value = c->last_sky.form; return CAP_OK;
    case CAP_DEBUG_SKY_PLANE_NONZERO:
    {
        const CapContext::LastSky& ls = c->last_sky;
        const size_t               n  = (size_t)ls.n_slots * c->screen.pixels_padded;
        if (!ls.form || !n || c->lane[ls.lane].pl_sky.n < n) return fail(CAP_ERR_STATE, "cap_debug_get: the last cap_render wrote no sky plane");
        HIP_TRY(hipSetDevice(c->device));
        if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
        unsigned long long h[1];
        if (int e = count_on_device(c, h, [&](unsigned long long* d) { launch_sky_nonzero(c->stream, c->lane[ls.lane].pl_sky.p, n, d); })) return e;
        *value = h[0];
        return CAP_OK;
    }
    case CAP_DEBUG_SELFTEST_GRAY:
    {
        const CapContext::LastQueues& lq = c->last_queues;
        if (!lq.valid || c->last_gray_entries) return fail(CAP_ERR_STATE, "cap_debug_get: the last cap_render left no 48-byte extension queues (small-scene path, CAP_NO_GRAY_ENTRIES)");
        HIP_TRY(hipSetDevice(c->device));
        if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
        // Bounce b appends to queue (b & 1) ^ 1 and the last bounce appends nothing: the last two appending bounces' entries are intact,
        // and so are their counter lines (cleared by the next batch).
        const CapContext::Lane& L = c->lane[lq.lane];
        const CounterLayout     lay{lq.num_bounces};
        unsigned long long      h[2];
        if (int e = count_on_device(c, h, [&](unsigned long long* d) {
                for (uint32_t back = 1; back <= 2 && back <= lq.num_bounces && lq.num_bounces - back >= lq.first_writer; ++back)
                {
                    const uint32_t b = lq.num_bounces - back, po = (b & 1u) ^ 1u;
                    launch_gray_selftest(c->stream, RayQueue{L.q_org[po].p, L.q_dir[po].p, L.q_thr[po].p, lay.ext(L.counters.p, b), lq.class_capacity, nullptr}, d);
                }
            }))
            return e;
        *value = (h[0] << 32) | std::min<unsigned long long>(h[1], 0xffffffffull);
        return CAP_OK;
    }
    case CAP_DEBUG_NEE_PAIRS:
        if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_debug_get: BVH not built");
        *value = ((uint64_t)(c->fan_pairs_nee.p ? c->fan_pair_nee_count : c->fan_pair_count) << 32) | c->fan_pair_count;
        return CAP_OK;
    case CAP_DEBUG_QUEUE_CANARY_BEHIND: return canary_count(c, true, value);
    case CAP_DEBUG_QUEUE_CANARY_USED: return canary_count(c, false, value);
    case CAP_DEBUG_WIDE_IN_USE:
        if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_debug_get: BVH not built");
        *value = bvh_dev(c, c->lane[0]).wide8_ok;
        return CAP_OK;
    default:
        if (key >= CAP_DEBUG_SWITCH_BASE && key < CAP_DEBUG_SWITCH_BASE + SW_COUNT)
        {
            *value = (uint64_t)c->sw.v[key - CAP_DEBUG_SWITCH_BASE];
            return CAP_OK;
        }
        return fail(CAP_ERR_INVALID_ARG, "cap_debug_get: unknown key %u", key);
    }
}

int cap_set_bvh_build(CapContext* c, uint32_t mode)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_set_bvh_build: ctx is NULL");
    if (mode > CAP_BVH_BUILD_SAH_DEVICE) return fail(CAP_ERR_INVALID_ARG, "cap_set_bvh_build: unknown mode %u", mode);
    c->bvh_build_mode = mode;
    return CAP_OK;
}

int cap_set_traversal(CapContext* c, uint32_t mode)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_set_traversal: ctx is NULL");
    if (mode > CAP_TRAVERSAL_EXHAUSTIVE) return fail(CAP_ERR_INVALID_ARG, "cap_set_traversal: unknown mode %u", mode);
    c->traversal_mode = mode;
    return CAP_OK;
}

int cap_accum_reset(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_accum_reset: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (c->accum.p) HIP_TRY(hipMemsetAsync(c->accum.p, 0, sizeof(float4) * c->accum.n, c->stream));
    c->frames_accumulated = 0;
    return CAP_OK;
}

int cap_accum_import(CapContext* c, const float* sum_rgba, uint64_t frames)
{
    if (!c || !sum_rgba) return fail(CAP_ERR_INVALID_ARG, "cap_accum_import: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_accum_import: resolution not set");
    HIP_TRY(hipSetDevice(c->device));
    if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    const size_t npix = (size_t)c->screen.width * c->screen.height;
    HIP_TRY(c->image_tmp.ensure(npix));
    HIP_TRY(c->accum.ensure(c->screen.pixels_padded));
    HIP_TRY(hipMemcpyAsync(c->image_tmp.p, sum_rgba, sizeof(float4) * npix, hipMemcpyHostToDevice, c->stream));
    LaunchCfg cfg{c->stream, (uint32_t)c->cu_count * 8u, 32};
    launch_tile(cfg, c->screen, c->image_tmp.p, c->accum.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // the host buffer is borrowed for the duration of the call only
    c->frames_accumulated = frames;
    return CAP_OK;
}

int cap_sync(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_sync: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return sync_and_collect(c);
}

int cap_readback(CapContext* c, CapBufferKind kind, float* dst)
{
    if (!c || !dst) return fail(CAP_ERR_INVALID_ARG, "cap_readback: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_readback: resolution not set");
    HIP_TRY(hipSetDevice(c->device));
    if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    const size_t npix = (size_t)c->screen.width * c->screen.height;
    HIP_TRY(c->image_tmp.ensure(npix));
    HIP_TRY(hipMemsetAsync(c->image_tmp.p, 0, sizeof(float4) * npix, c->stream));
    LaunchCfg cfg{c->stream, (uint32_t)c->cu_count * 8u, 32};
    const bool is_aov = kind <= CAP_BUF_COMBINED || kind == CAP_BUF_INDIRECT_LOWRES;
    if (is_aov && !c->aov_valid) return fail(CAP_ERR_STATE, "cap_readback: no frame rendered with CAP_RENDER_AOV");
    if (!is_aov && !c->accum.p) return fail(CAP_ERR_STATE, "cap_readback: nothing rendered");
    const AovPlanes aov = aov_planes(c);
    switch (kind)
    {
    case CAP_BUF_GBUFFER_GEO: launch_untile(cfg, c->screen, c->aov_geo.p, nullptr, nullptr, 0, c->image_tmp.p); break;
    case CAP_BUF_NORMAL_DEPTH: launch_untile(cfg, c->screen, c->aov_nd.p, nullptr, nullptr, 0, c->image_tmp.p); break;
    case CAP_BUF_DIRECT: launch_untile(cfg, c->screen, aov.direct, nullptr, nullptr, 0, c->image_tmp.p); break;
    case CAP_BUF_ALBEDO: launch_untile(cfg, c->screen, aov.albedo, nullptr, nullptr, 0, c->image_tmp.p); break;
    case CAP_BUF_INDIRECT: launch_untile(cfg, c->screen, aov.color, nullptr, nullptr, 0, c->image_tmp.p); break;
    case CAP_BUF_COMBINED:
        launch_untile(cfg, c->screen, aov.color, aov.albedo, aov.direct, 1, c->image_tmp.p);
        break;
    case CAP_BUF_ACCUM_SUM: launch_untile(cfg, c->screen, c->accum.p, nullptr, nullptr, 0, c->image_tmp.p); break;
    case CAP_BUF_ACCUM_MEAN: launch_untile(cfg, c->screen, c->accum.p, nullptr, nullptr, 2, c->image_tmp.p); break;
    case CAP_BUF_INDIRECT_LOWRES:
    {
        if (!c->aov_lowres) return fail(CAP_ERR_STATE, "cap_readback: the last CAP_RENDER_AOV frame was not rendered with CAP_RENDER_LOWRES_INDIRECT");
        launch_untile(cfg, c->screen, aov.color, nullptr, nullptr, 0, c->image_tmp.p);
        HIP_TRY(c->post_itemp.ensure(npix));
        launch_decimate2x(c->stream, c->image_tmp.p, c->screen.width, c->screen.height, (c->aov_frame % 4u) / 2u, (c->aov_frame % 4u) % 2u,
                          c->post_itemp.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst, c->post_itemp.p, sizeof(float4) * (npix / 4), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return CAP_OK;
    }
    default: return fail(CAP_ERR_INVALID_ARG, "cap_readback: unknown buffer kind %d", (int)kind);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, c->image_tmp.p, sizeof(float4) * npix, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CAP_OK;
}

int cap_stats_get(CapContext* c, CapStats* out)
{
    if (!c || !out) return fail(CAP_ERR_INVALID_ARG, "cap_stats_get: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    *out = c->stats;
    return CAP_OK;
}

int cap_stats_reset(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_stats_reset: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    c->stats = CapStats{};
    if (c->shaded_counter.p) HIP_TRY(hipMemsetAsync(c->shaded_counter.p, 0, kGuardWords * sizeof(uint64_t), c->stream));  // ordered on the context's stream
    return CAP_OK;
}

int cap_tile_buffer_floats(CapContext* c, size_t* out_floats)
{
    if (!c || !out_floats) return fail(CAP_ERR_INVALID_ARG, "cap_tile_buffer_floats: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_tile_buffer_floats: resolution not set");
    *out_floats = (size_t)c->screen.pixels_padded * 4;
    return CAP_OK;
}

int cap_resolve_tiles(CapContext* c, float* device_dst)
{
    if (!c || !device_dst) return fail(CAP_ERR_INVALID_ARG, "cap_resolve_tiles: NULL argument");
    if (!c->accum.p) return fail(CAP_ERR_STATE, "cap_resolve_tiles: nothing rendered");
    HIP_TRY(hipSetDevice(c->device));
    LaunchCfg cfg{c->stream, (uint32_t)c->cu_count * 8u, 32};
    launch_tiles_mean(cfg, c->accum.p, c->screen.pixels_padded, reinterpret_cast<float4*>(device_dst));
    HIP_TRY(hipGetLastError());
    return CAP_OK;
}

int cap_assemble_tiles(CapContext* c, const float* device_src, uint32_t shard_count, float* device_image)
{
    if (!c || !device_src || !device_image) return fail(CAP_ERR_INVALID_ARG, "cap_assemble_tiles: NULL argument");
    if (shard_count != c->screen.shard_count) return fail(CAP_ERR_INVALID_ARG, "cap_assemble_tiles: shard_count %u != context's %u", shard_count, c->screen.shard_count);
    HIP_TRY(hipSetDevice(c->device));
    LaunchCfg cfg{c->stream, (uint32_t)c->cu_count * 8u, 32};
    launch_assemble(cfg, c->screen, reinterpret_cast<const float4*>(device_src), shard_count, reinterpret_cast<float4*>(device_image));
    HIP_TRY(hipGetLastError());
    return CAP_OK;
}
}  // extern "C"
