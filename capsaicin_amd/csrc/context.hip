// context.hip — the context behind the C ABI of include/capsaicin_hip.h: creation, settings, the working sets of a render, the
// per-batch wavefront loop (the MI355X counterpart of RaytracingSystem::Run, reference
// src/systems/raytracing_system.cpp:230-318, ray passes only), readback, statistics.
//
// The product path is HIP only: every entry point that needs the GPU fails with CAP_ERR_HIP when no device or
// kernel is available; there is no CPU fallback.
//
// The rest of the ABI by role: ctx_scene.hip (uploads, light table), ctx_bvh.hip (builds, refit, objects, instances), ctx_query.hip (ray
// queries), ctx_post.hip (reconstruction chain), ctx_comm.hip (RCCL frame exchange); cap_context.h is what they share.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "cap_context.h"
#include "cap_near.h"
#include "cap_wide.h"
#include "query_ranges.h"

namespace
{
thread_local std::string g_error;

// camera rays take the per-lane wide kernel instead of the packet walk from this many triangles per pixel on (measured: cap_render;
// 1.0 until the walk's node step was rewritten in round 6 -- at 1.0 the walk now wins by 6 % of the step, at 2.0 the two are level)
constexpr double kPrimaryWideTrianglesPerPixel = 2.0;
// shadow rays take the lane-refill kernel from this many bytes of wide nodes + intersection records on (measured: cap_render).
// Round 6: never by default.  Until the per-chunk kernel's traversal was compiled per light octant (docs/experiments.md (86)) the refill
// kernel won by 3 % from 512 MiB of tree on; now the per-chunk kernel wins by 6 - 8 % at 8.4 M and 16.8 M triangles (1.5 GB of tree),
// as it always did below.  CAP_ANY_REFILL=1 still selects the refill kernel (tests/test_fallback_kernels_gpu.py keeps it honest).
constexpr uint64_t kAnyRefillTreeBytes = ~0ull;

// guard block of a context (ShadeArgs::shaded_counter): {-, malformed path ids seen by shade, by trace_any, last offender, appends
// beyond a class's capacity, -, -, -}
constexpr size_t kGuardWords = 8;
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
        const uint32_t D = pc.second & 0xffffu;
        const bool     queued = (pc.second >> 16) == 0u;  // false: the batch's shadow rays were traced where they were generated
        const size_t per = (size_t)kQueueClasses * kCounterStride;
        for (uint32_t b = 0; b <= D; ++b)
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
struct StageTimer
{
    CapContext* c;
    TimedSpan   sp;
    bool        on;
    StageTimer(CapContext* ctx, int stage, bool enabled = true, int also = ST_NONE) : c(ctx), on(enabled)
    {
        if (!on) return;
        sp.stage = stage;
        sp.also  = also;
        sp.a     = get_event(c);
        sp.b     = get_event(c);
        (void)hipEventRecord(sp.a, c->stream);
    }
    ~StageTimer()
    {
        if (!on) return;
        (void)hipEventRecord(sp.b, c->stream);
        c->spans.push_back(sp);
    }
};

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

// lighting.h:20-33 + camera.h:41, evaluated once per frame on the host with the shared arithmetic contract
FrameConst frame_const(uint32_t frame_count, bool lowres_indirect)
{
    FrameConst f{};
    halton23(frame_count, f.jitter_x, f.jitter_y);
    f.frame_count = frame_count;
    // rt_indirect.hlsl:55-56: sp_offset = ((frame % 4) / 2, (frame % 4) % 2)
    f.lowres_sel = lowres_indirect ? (4u | (((frame_count % 4u) / 2u) << 1) | ((frame_count % 4u) % 2u)) : 0u;
    const float t = 2.0f * 3.14f * (float)(frame_count % 4096) / 4096.0f;
    float       st, ct;
    sincos_c(t, st, ct);
    const v3 dir = normalize3(mk3(40.0f * st, 100.0f, 40.0f * ct));
    f.light_dir[0] = dir.x, f.light_dir[1] = dir.y, f.light_dir[2] = dir.z;
    f.light_intensity[0] = 1.0f * (2.0f * 14.0f + 0.0f);
    f.light_intensity[1] = 1.0f * (2.0f * 12.0f + 0.0f);
    f.light_intensity[2] = 1.0f * (2.0f * 10.0f + (2.0f + 2.0f * ct));
    return f;
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

// Element counts of one lane's working set for `slots` frame slots and `bounces` bounces: what ensure_lane allocates, and what
// cap_render tests to learn whether a call grows a lane (growing frees the old buffers, so the streams are drained first)
struct LaneSizes
{
    size_t planes, queues, rings, counters, terms, camera;
};

LaneSizes lane_sizes(const CapContext* c, uint32_t slots, uint32_t bounces, bool sample_table, uint32_t camera_groups)
{
    LaneSizes z;
    z.planes = (size_t)slots * c->screen.pixels_padded;
    z.queues = z.planes + (size_t)kQueueClasses * 64;  // queue regions round up to whole chunks per class
    // the shadow queue's memory also holds the fused kernels' per-wave survivor rings (ShadeArgs::wave_ring): 128 entries for
    // every wave of the largest persistent grid (8 workgroups per CU)
    z.rings = std::max(z.queues, (size_t)std::max(c->cu_count, 1) * 8 * (kBlock / 64) * 128);
    // queue counters (ext + shadow share words) + chunk-grab counters of the fused and of the any-hit launch, per bounce
    z.counters = (3 * (size_t)(bounces + 1) + 1) * kQueueClasses * kCounterStride;  // + 1: the camera rays' identity queue
    // the table of direction-sample terms (ShadeArgs::sample_terms): 4096 entries per frame slot and sampling bounce, 32 MB at 64 x 8
    z.terms = sample_table ? (size_t)slots * bounces * 4096 : 0;
    // the table of camera vertices (launch_camera_vertices): two planes of one entry per (jitter group, padded pixel), 0.5 GB at 8 groups of 1080p
    z.camera = 2 * (size_t)camera_groups * c->screen.pixels_padded;
    return z;
}

bool lane_grows(const CapContext::Lane& L, const LaneSizes& z) { return L.pl_color.n < z.planes || L.counters.n < z.counters || L.terms.n < z.terms || L.camera.n < z.camera; }

int ensure_lane(CapContext* c, CapContext::Lane& L, uint32_t slots, uint32_t bounces, bool sample_table, uint32_t camera_groups)
{
    const LaneSizes z = lane_sizes(c, slots, bounces, sample_table, camera_groups);
    for (DevBuf<float4>* b : {&L.hits, &L.q_org[0], &L.q_org[1], &L.q_dir[0], &L.q_dir[1], &L.q_thr[0], &L.q_thr[1], &L.s_dir})
        HIP_TRY(b->ensure(z.queues));
    for (DevBuf<float4>* b : {&L.s_org, &L.s_con}) HIP_TRY(b->ensure(z.rings));
    for (DevBuf<float4>* b : {&L.pl_color, &L.pl_direct, &L.pl_albedo}) HIP_TRY(b->ensure(z.planes));
    HIP_TRY(L.counters.ensure(z.counters));
    if (z.terms) HIP_TRY(L.terms.ensure(z.terms));
    if (z.camera) HIP_TRY(L.camera.ensure(z.camera));
    // as much spill as lane 0, whose area cap_bvh_build allocates (for lane 0 itself: nothing to do)
    if (c->lane[0].stack_spill.n) HIP_TRY(L.stack_spill.ensure(c->lane[0].stack_spill.n));
    return CAP_OK;
}

// what a render needs beside its lanes: the AOV frame's geometry planes, the guard block, the accumulation buffer
int ensure_frame_buffers(CapContext* c)
{
    HIP_TRY(c->aov_geo.ensure(c->screen.pixels_padded));
    HIP_TRY(c->aov_nd.ensure(c->screen.pixels_padded));
    if (!c->shaded_counter.p)
    {
        HIP_TRY(c->shaded_counter.ensure(kGuardWords));
        HIP_TRY(hipMemsetAsync(c->shaded_counter.p, 0, kGuardWords * sizeof(uint64_t), c->stream));
    }
    if (!c->accum.p || c->accum.n < c->screen.pixels_padded)
    {
        HIP_TRY(c->accum.ensure(c->screen.pixels_padded));
        HIP_TRY(hipMemsetAsync(c->accum.p, 0, sizeof(float4) * c->screen.pixels_padded, c->stream));
        c->frames_accumulated = 0;
    }
    return CAP_OK;
}

// the second lane's stream and the events that order the two lanes
int ensure_lane_streams(CapContext* c)
{
    if (!c->stream2)
    {
        // (A/B switch: the second lane's stream priority -- streams of different priority never share a hardware queue)
        if (c->sw.v[SW_LANE1_PRIORITY] >= 0)
            HIP_TRY(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, (int)c->sw.v[SW_LANE1_PRIORITY]));
        else
            HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    }
    c->lane[1].stream = c->stream2;
    for (hipEvent_t* e : {&c->lane_ev[0], &c->lane_ev[1], &c->fork_ev, &c->join_ev})
        if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return CAP_OK;
}

// How cap_render cuts a call into batches.
struct BatchPolicy
{
    uint32_t slots;               // frame slots of a batch (the last one may fill fewer)
    bool     two_lanes;           // consecutive batches alternate between the two lanes
    bool     lane1_failed_before; // two_lanes, but a second working set of this size could not be allocated earlier
};

// Reads the context and changes nothing (it may ask the device how much memory is free).  tree_path: the render goes through the
// tree kernels, not the small-scene fused ones.
BatchPolicy batch_policy(const CapContext* c, uint32_t n_frames, uint32_t num_bounces, uint32_t flags, bool tree_path)
{
    const uint32_t Ppad = c->screen.pixels_padded;
    // paths in flight per batch; measured on the headline workload (tools/batch_sweep.sh, end of round 2): 8 Mi 31.0 ms, 16 Mi 25.5,
    // 32 Mi 22.1, 64 Mi 21.2, 128 Mi 21.1 per step -- every launch has a fixed cost (grid start, tables, tail) that fewer, larger
    // batches amortise; 64 Mi paths are ~14 GB of queues and planes
    uint64_t       budget = c->max_batch_paths ? c->max_batch_paths : (uint64_t)64 << 20;
    if (!c->max_batch_paths && (uint64_t)n_frames * Ppad > budget)
    {
        // Twice that when the card has the room (round 6, docs/experiments.md (88)): the tree path has 27 launches per batch, most of
        // them short, and gains 1.7 % (the 262 k hall at 128 spp: 92.1 -> 90.5 ms; round 4 measured 101.2 -> 99.4 and kept 64 Mi for
        // its 14 GB per lane), the small-scene path 1.0 % (headline 20.22 -> 20.01 ms).  Taken when the working set is already that
        // large or the device reports room for it with a margin -- 128 Mi paths are ~28 GB per lane of the card's 288, and the tree
        // path runs two lanes; cap_set_batch_paths overrides either way.
        const uint64_t big       = (uint64_t)128 << 20;
        const uint64_t big_slots = std::max<uint64_t>(1, std::min<uint64_t>(big / std::max(1u, Ppad), kMaxFrameSlots));
        bool           room      = c->lane[0].pl_color.n >= big_slots * Ppad && (!tree_path || c->lane[1].pl_color.n >= big_slots * Ppad);
        if (!room)
        {
            size_t free_b = 0, total_b = 0;
            room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 3u * big_slots * Ppad * 256u;  // ~208 B per path and lane
        }
        if (room) budget = big;
    }
    uint32_t       slots  = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(budget / std::max(1u, Ppad), kMaxFrameSlots));
    slots                 = std::min(slots, n_frames);
    // Two lanes (CapContext::Lane): consecutive batches alternate between two working sets on two streams, so that the tail of
    // one batch's launch -- the last chunks, a workgroup at a time, with most of the chip idle -- is filled by the other batch's
    // next launch instead of waiting for the stream's next kernel (measured with two contexts side by side, tools/dual_test.py:
    // 21.0 -> 20.55 ms per step on the headline, 3.30 -> 3.05 ms for shard 0 of 8, 28.3 -> 27.1 ms on the 262 k scene).  A call
    // that fits one batch is cut in two halves when the halves are still large.  Per-stage timers need one stream.
    const bool no_two_lanes = c->sw.on(SW_NO_TWO_LANES);  // A/B switch
    // Only on the tree path: its bounces are three launches each, and from the third bounce on they are short (the 262 k scene: 27
    // launches per batch, the last 15 under 0.2 ms each) -- 28.3 -> 26.4 ms per 32 spp.  The small-scene path's nine long fused
    // launches gain nothing measurable (20.45 -> 20.25 ms with the context's own stream, 20.56 -> 20.9 beside a torch stream).
    bool two_lanes = !no_two_lanes && tree_path && c->bvh_info.stack_entries != 0 && !(flags & CAP_RENDER_GBUFFER_FEEDBACK) &&
                     !(flags & CAP_RENDER_LOWRES_INDIRECT) && n_frames >= 2;
    if (two_lanes && slots >= n_frames)
    {
        const uint64_t split_min = (uint64_t)c->sw.get(SW_LANE_SPLIT_MIN, (int64_t)4 << 20);  // A/B switch (shard 0 of 8 of the 262 k scene: 4.55 -> 4.35 ms with halves of 4 Mi paths)
        if ((uint64_t)n_frames * Ppad >= split_min)
            slots = (n_frames + 1) / 2;
        else
            two_lanes = false;
    }
    // (per-stage timers and launch tracing need one stream: the batches keep the size the two lanes gave them -- so that a stage-timed
    // render launches what the plain one does -- and run one after the other on lane 0)
    if ((flags & CAP_RENDER_STAGE_TIMERS) || c->sw.on(SW_TRACE_LAUNCHES)) two_lanes = false;
    // (cap_render does not try a second working set of a size that has failed, or a larger one, again at once: see there)
    const bool failed_before =
        two_lanes && c->lane1_failed_paths && (uint64_t)slots * Ppad >= c->lane1_failed_paths && num_bounces >= c->lane1_failed_bounces;
    return BatchPolicy{slots, two_lanes, failed_before};
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
    "CAP_W8_GRID", "CAP_AUTO_SAH_TRIANGLES", "CAP_NO_NEE_PAIR_CULL", "CAP_RAYGEN_KERNEL", "CAP_NO_PLANE_CODE", "CAP_SAMPLE_TABLE", "CAP_NO_CAMERA_TABLE"};

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
// word; after a render with undersized sub-queues every entry BEHIND the last class's sub-queue must still hold it.
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
    DevBuf<unsigned long long> dbuf;  // (released on every path: ADVICE r5)
    HIP_TRY(dbuf.ensure(1));
    unsigned long long* d = dbuf.p;
    HIP_TRY(hipMemsetAsync(d, 0, sizeof(*d), c->stream));
    const size_t used = std::min((size_t)kQueueClasses * c->last_class_capacity, L.q_org[0].n);
    for (int k = 0; k < 2; ++k)
        for (DevBuf<float4>* b : {&L.q_org[k], &L.q_dir[k], &L.q_thr[k]})
        {
            const size_t lo = behind ? used : 0, hi = behind ? b->n : used;
            if (hi > lo) hipLaunchKernelGGL(k_canary_count, dim3(512), dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(b->p), lo, hi, d);
        }
    HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *value = h;
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
        DevBuf<unsigned long long> d;  // (released on every path: ADVICE r5)
        unsigned long long         h[3] = {0, 0, 0};
        HIP_TRY(d.ensure(3));
        HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(h), c->stream));
        launch_div_selftest(c->stream, d.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
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
        DevBuf<unsigned long long> d;
        unsigned long long         h[2] = {0, 0};
        HIP_TRY(d.ensure(2));
        HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(h), c->stream));
        launch_shade_forms_selftest(c->stream, d.p, key == CAP_DEBUG_SELFTEST_SHADE_DIV2 ? 1u : 0u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
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
        DevBuf<unsigned long long> d;
        unsigned long long         h[2] = {0, 0};
        HIP_TRY(d.ensure(2));
        HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(h), c->stream));
        launch_sample_terms_selftest(c->stream, c->bluenoise.p, lt.frames, lt.n_slots, lt.num_bounces, c->lane[lt.lane].terms.p, d.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
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
        DevBuf<unsigned long long> d;
        unsigned long long         h[2] = {0, 0};
        HIP_TRY(d.ensure(2));
        HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(h), c->stream));
        // the launch arguments the table was built with (camera, screen and scene as they are now: ask right after the render)
        ShadeArgs sa{};
        sa.scene = scene_dev(c), sa.cam = camera_dev(c->camera), sa.screen = c->screen, sa.frames = lc.frames, sa.n_slots = lc.n_slots;
        sa.cull_camera_pairs = c->last_cull_camera_pairs;
        LaunchCfg     cfg{c->stream, (uint32_t)c->cu_count * 6u, 0u, (uint32_t)c->cu_count};
        float4* const tab = c->lane[lc.lane].camera.p;
        launch_camera_vertices(cfg, bvh_dev(c, c->lane[lc.lane]), sa, lc.n_slots, tab, tab + (size_t)lc.n_groups * c->screen.pixels_padded, d.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const unsigned long long expected = (unsigned long long)lc.n_slots * c->screen.pixels_padded;
        if (h[1] != expected) return fail(CAP_ERR_HIP, "cap_debug_get: the camera table self-test compared %llu of %llu entries", h[1], expected);
        *value = (h[0] << 32) | ((uint64_t)lc.n_groups << 16) | lc.n_slots;  // mismatches << 32 | groups << 16 | slots compared
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

int cap_render(CapContext* c, uint32_t frame_begin, uint32_t n_frames, uint32_t num_bounces, uint32_t flags)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_render: ctx is NULL");
    if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_render: call cap_bvh_build first");
    if (c->bvh_stale) return fail(CAP_ERR_STATE, "cap_render: vertices changed; call cap_bvh_refit or cap_bvh_build");
    if (!c->camera_ready || !c->bluenoise_ready || !c->screen.width) return fail(CAP_ERR_STATE, "cap_render: camera, blue noise and resolution must be set");
    const bool ext = (flags & CAP_RENDER_EXT_MATERIALS) != 0;
    if (ext && !c->materials_ready) return fail(CAP_ERR_STATE, "cap_render: CAP_RENDER_EXT_MATERIALS needs cap_materials_upload (one material per mesh)");
    static_assert(sizeof(MaterialDev) == sizeof(CapMaterial), "material layouts must match");
    if (num_bounces > 255) return fail(CAP_ERR_INVALID_ARG, "cap_render: num_bounces %u exceeds 255", num_bounces);
    if (!n_frames) return CAP_OK;
    HIP_TRY(hipSetDevice(c->device));
    c->last_mark_form   = 0;
    c->last_sample_table = 0;
    c->last_terms        = CapContext::LastTerms{};
    const bool feedback = (flags & CAP_RENDER_GBUFFER_FEEDBACK) != 0;
    if (feedback)
    {
        // the branch reads the previous frame's reconstruction output: one frame per call, the whole image on this context
        if (ext) return fail(CAP_ERR_UNSUPPORTED, "cap_render: CAP_RENDER_GBUFFER_FEEDBACK is defined for the reference shading model only");
        if (n_frames != 1) return fail(CAP_ERR_INVALID_ARG, "cap_render: CAP_RENDER_GBUFFER_FEEDBACK renders one frame per call (n_frames is %u)", n_frames);
        // sharded contexts: the previous frame's output reaches the non-root ranks through cap_feedback_import
        if (!c->prev_camera_ready) return fail(CAP_ERR_STATE, "cap_render: CAP_RENDER_GBUFFER_FEEDBACK needs cap_prev_camera_set");
        if (c->post_w != c->screen.width || c->post_h != c->screen.height)
            if (int e = cap_post_reset(c)) return e;  // first frame: cleared histories, every vertex is a disocclusion
    }

    const bool lowres = (flags & CAP_RENDER_LOWRES_INDIRECT) != 0;
    if (lowres)
    {
        // the half-resolution indirect image only exists per frame (2x2 interleave over four frames): nothing to accumulate
        if (ext) return fail(CAP_ERR_UNSUPPORTED, "cap_render: CAP_RENDER_LOWRES_INDIRECT is defined for the reference shading model only");
        if (n_frames != 1) return fail(CAP_ERR_INVALID_ARG, "cap_render: CAP_RENDER_LOWRES_INDIRECT renders one frame per call (n_frames is %u)", n_frames);
        if ((c->screen.width | c->screen.height) & 1u) return fail(CAP_ERR_INVALID_ARG, "cap_render: CAP_RENDER_LOWRES_INDIRECT needs even width and height (%ux%u)", c->screen.width, c->screen.height);
    }

    // Which traversal path the render takes, decided here once: the small-scene kernels (closest hit and shading fused in one
    // launch per bounce, every triangle tested) or the tree path.  stack_entries == 0 selects the former in the launchers.
    if (c->traversal_mode == CAP_TRAVERSAL_EXHAUSTIVE && c->tri_count > 4096)
        return fail(CAP_ERR_UNSUPPORTED, "cap_render: exhaustive traversal refused for %u triangles", c->tri_count);
    const bool     tree_path     = c->traversal_mode == CAP_TRAVERSAL_EXHAUSTIVE ? false
                                                                                 : !(c->traversal_mode == CAP_TRAVERSAL_AUTO && c->tri_count <= kExhaustiveMax);
    const uint32_t stack_entries = tree_path ? c->bvh_info.stack_entries : 0u;
    const bool     fused         = stack_entries == 0;  // small-scene path: closest hit and shading in one kernel per bounce

    const uint32_t    Ppad      = c->screen.pixels_padded;
    const BatchPolicy policy    = batch_policy(c, n_frames, num_bounces, flags, tree_path);
    const uint32_t    slots     = policy.slots;
    bool              two_lanes = policy.two_lanes;
    // No host synchronisation with the previous call: everything it still uses is either ordered behind it on the stream (queues,
    // counters, planes) or lives in another slot of the constants ring.  Only a long backlog of unread events / counters is
    // drained (what cap_sync / cap_stats_get do anyway), and a growing allocation (which frees the old buffers).
    if (c->spans.size() > 2048 || c->pending.size() > 64 || c->post_marks.size() > 256)
        if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    // Direction-sample terms from a per-batch table (ShadeArgs::sample_terms): decided once per call, for every launch of every batch.
    // Rebuilt by every batch and never kept across calls: frame_begin advances from call to call in real use.
    // A/B switch CAP_SAMPLE_TABLE: 0 never, 1 whenever the kernels have the form (which is also the product's choice).
    const bool sample_table = fused && !ext && !feedback && num_bounces >= 1 && c->sw.get(SW_SAMPLE_TABLE, 1) != 0 &&
                              trace_shade_has_table_form(bvh_dev(c, c->lane[0]), scene_dev(c));
    c->last_sample_table = sample_table ? 1u : 0u;
    // Bounce 0 inside bounce 1's launch, from a table of camera vertices (launch_camera_vertices, launch_trace_shade's camera_head): decided
    // once per call.  The lean table kernels of an untextured scene in an accumulate-only render, whose colour plane carries the first
    // vertex's code and whose shadow rays go through the wave rings -- the conditions of albedo_in_w, code_in_color, inline_probe and
    // wave_ring below, which a batch repeats for itself (the rings' size is the one it alone knows).  A/B switch CAP_NO_CAMERA_TABLE.
    const bool camera_table = sample_table && !lowres && !(flags & CAP_RENDER_AOV) && !c->sw.on(SW_NO_CAMERA_TABLE) && !c->sw.on(SW_NO_ALBEDO_IN_W) &&
                              !c->sw.on(SW_NO_PLANE_CODE) && !c->sw.on(SW_NO_INLINE_PROBE) && !c->sw.on(SW_NO_WAVE_RING) && c->debug_capacity_div <= 1 &&
                              c->texture_host.empty() && trace_shade_has_code_form(bvh_dev(c, c->lane[0]), scene_dev(c));
    c->last_camera_table = 0;
    c->last_camera       = CapContext::LastCamera{};
    // Jitter groups: the slots of a batch by the bits of (jitter_x, jitter_y).  slot_group[f]: the group of frame f within its batch,
    // numbered in order of first appearance; group_first[batch start + g]: the first slot of group g.  A group need not be contiguous.
    std::vector<uint32_t> slot_group, group_first, batch_groups;
    uint32_t              camera_groups = 0;
    if (camera_table)
    {
        slot_group.resize(n_frames), group_first.assign(n_frames, 0u);
        for (uint32_t done = 0; done < n_frames; done += slots)
        {
            const uint32_t ns = std::min(slots, n_frames - done);
            uint32_t       ng = 0;
            for (uint32_t s = 0; s < ns; ++s)
            {
                float sx, sy, gx, gy;  // frame_const()'s jitter
                halton23(frame_begin + done + s, sx, sy);
                uint32_t g = 0;
                for (; g < ng; ++g)
                {
                    halton23(frame_begin + done + group_first[done + g], gx, gy);
                    if (memcmp(&gx, &sx, sizeof(float)) == 0 && memcmp(&gy, &sy, sizeof(float)) == 0) break;
                }
                if (g == ng) group_first[done + ng++] = s;
                slot_group[done + s] = g;
            }
            batch_groups.push_back(ng);
            camera_groups = std::max(camera_groups, ng);
        }
    }
    const LaneSizes need = lane_sizes(c, slots, num_bounces, sample_table, camera_groups);
    if (lane_grows(c->lane[0], need) || !c->accum.p || c->accum.n < Ppad) HIP_TRY(hipStreamSynchronize(c->stream));
    if (ensure_lane(c, c->lane[0], slots, num_bounces, sample_table, camera_groups) != CAP_OK || ensure_frame_buffers(c) != CAP_OK) return CAP_ERR_HIP;
    if (policy.lane1_failed_before)
    {
        // this size has already failed: one lane, without asking again -- except every 32nd time, and at once when the device reports
        // room for it (memory can come back without any call on this context: another context closed, a co-tenant left)
        size_t free_b = 0, total_b = 0;
        const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > (size_t)slots * Ppad * 256u;  // a working set is ~208 B per path
        if (!room && (++c->lane1_retry_tick % 32u) != 0u)
        {
            two_lanes = false;
            ++c->stats.lane1_dropped;
        }
    }
    if (two_lanes)
    {
        if (lane_grows(c->lane[1], need))
        {
            HIP_TRY(hipStreamSynchronize(c->stream));  // growing frees the old buffers
            if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
        }
        if (c->debug_fail_lane || ensure_lane(c, c->lane[1], slots, num_bounces, sample_table, camera_groups) != CAP_OK || ensure_lane_streams(c) != CAP_OK)
        {
            // the second working set doubles the batch's memory (~28 GB at the default budget): without it the batches of this call
            // simply run one after the other on lane 0 -- counted in CapStats::lane1_dropped, and not tried again at this
            // size until something is freed
            (void)hipGetLastError();
            c->lane[1] = CapContext::Lane{};
            c->lane1_failed_paths = (uint64_t)slots * Ppad, c->lane1_failed_bounces = num_bounces;  // (ensure_lane's size depends on both)
            ++c->stats.lane1_dropped;
            two_lanes = false;
        }
    }
    c->lanes_last_render = two_lanes ? 2u : 1u;
    const uint32_t ring = c->frames_next;
    c->frames_next      = (c->frames_next + 1) % CapContext::kFrameRing;
    if (!c->frames_event[ring]) HIP_TRY(hipEventCreateWithFlags(&c->frames_event[ring], hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(c->frames_event[ring]));  // the call that used this slot kFrameRing calls ago: long done
    if (c->frames_ring[ring].n < n_frames)
    {
        // (a larger buffer: the old one of this slot is idle by the event above)
        HIP_TRY(c->frames_ring[ring].ensure(n_frames));
    }
    if (c->frames_pinned_n[ring] < n_frames)
    {
        if (c->frames_pinned[ring]) HIP_TRY(hipHostFree(c->frames_pinned[ring]));
        c->frames_pinned[ring] = nullptr;
        HIP_TRY(hipHostMalloc((void**)&c->frames_pinned[ring], sizeof(FrameConst) * n_frames, hipHostMallocDefault));
        c->frames_pinned_n[ring] = n_frames;
    }
    for (uint32_t f = 0; f < n_frames; ++f)
    {
        FrameConst& fc = c->frames_pinned[ring][f] = frame_const(frame_begin + f, lowres);
        // the two words nothing else reads in memory: the slot's jitter group, and the first slot of the group of this number
        if (camera_table) memcpy(&fc.pad1, &slot_group[f], 4), memcpy(&fc.pad2, &group_first[f], 4);
    }
    HIP_TRY(hipMemcpyAsync(c->frames_ring[ring].p, c->frames_pinned[ring], sizeof(FrameConst) * n_frames, hipMemcpyHostToDevice, c->stream));
    const bool st = (flags & CAP_RENDER_STAGE_TIMERS) != 0;
    if (c->textures_dirty)
    {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->textures.ensure(std::max<size_t>(1, c->texture_host.size())));
        if (!c->texture_host.empty())
            HIP_TRY(hipMemcpy(c->textures.p, c->texture_host.data(), sizeof(TextureDev) * c->texture_host.size(), hipMemcpyHostToDevice));
        c->textures_dirty = false;
    }

    // Persistent grids must be fully resident: a workgroup that cannot be co-scheduled runs as a second round after the first
    // waves retire and doubles the kernel's tail.  blocks_per_cu is therefore the residency the kernels are built for
    // (launch bounds in kernels.hip and small_scene.hip), not the 8 a register-light kernel could reach.
    uint32_t blocks_per_cu = fused ? 6u : (stack_entries <= 32 ? 5u : 2u);  // measured: 4..8 within 4 %, 6 best
    if (c->sw.v[SW_BLOCKS_PER_CU] >= 0) blocks_per_cu = (uint32_t)std::max<int64_t>(1, c->sw.v[SW_BLOCKS_PER_CU]);
    const SceneDev  scene = scene_dev(c);
    const CameraDev cam   = camera_dev(c->camera);
    const uint32_t  D     = num_bounces;
    std::unique_ptr<StageTimer> total(new StageTimer(c, ST_COUNT));  // its destructor closes the span on every exit path

    const uint32_t n_batches = (n_frames + slots - 1) / slots;
    // Every way out of this function after the fork -- the early returns of HIP_TRY and of the launch tracing included -- leaves the
    // context's stream, the one callers order cap_sync / cap_readback / buffer growth behind, waiting for lane 1 (an error
    // between fork and join used to leave lane-1 work running that nothing waited for).
    struct LaneJoin
    {
        CapContext* c;
        bool        armed = false;
        ~LaneJoin()
        {
            if (!armed) return;
            if (hipEventRecord(c->join_ev, c->stream2) != hipSuccess || hipStreamWaitEvent(c->stream, c->join_ev, 0) != hipSuccess)
                (void)hipStreamSynchronize(c->stream2);
        }
    } lane_join{c};
    if (two_lanes)
    {
        // lane 1 starts behind everything queued on the context's stream so far (the frame constants' upload, earlier calls)
        HIP_TRY(hipEventRecord(c->fork_ev, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->stream2, c->fork_ev, 0));
        lane_join.armed = true;
    }
    hipEvent_t last_resolve = nullptr;  // the accumulation buffer takes the batches in frame order, whichever lane ran them
    uint32_t   batch        = 0;

    for (uint32_t done = 0; done < n_frames; done += slots, ++batch)
    {
        const uint32_t    lane = two_lanes ? ((n_batches - 1u - batch) & 1u) : 0u;  // the last batch on lane 0
        CapContext::Lane& L    = c->lane[lane];
        const BvhDev      bvh  = bvh_dev(c, L);
        LaunchCfg         cfg{L.stream, (uint32_t)c->cu_count * blocks_per_cu, stack_entries, (uint32_t)c->cu_count};
        cfg.sw = &c->sw;
        const uint32_t ns = std::min(slots, n_frames - done);
        const FrameConst* frames = c->frames_ring[ring].p + done;
        const size_t   per_queue     = (size_t)kQueueClasses * kCounterStride;  // counter words of one queue
        // per bounce and class one 64-bit word: low half = extension entries, high half = shadow entries (one atomic serves both)
        const size_t   counter_words = (size_t)(D + 1) * per_queue;
        HIP_TRY(hipMemsetAsync(L.counters.p, 0, sizeof(uint32_t) * 3 * counter_words, L.stream));
        uint32_t*      ext_count = L.counters.p;
        uint32_t*      sh_count  = L.counters.p + 1;
        uint32_t*      work_shade = L.counters.p + counter_words;      // + b * per_queue: grab counters of bounce b's fused launch
        uint32_t*      work_any   = L.counters.p + 2 * counter_words;  // ... and of its any-hit launch
        const uint32_t total_chunks   = ns * (Ppad >> 6);
        uint32_t       class_capacity = ((total_chunks + kQueueClasses - 1) / kQueueClasses) * 64u;
        // (tests of the append guard: sub-queues deliberately too small -- the appends beyond them must be dropped and counted)
        if (c->debug_capacity_div > 1) class_capacity = std::max(64u, (class_capacity / c->debug_capacity_div) & ~63u);
        c->last_class_capacity = class_capacity;
        const bool     last_batch = done + ns >= n_frames;
        const uint32_t aov_slot   = ((flags & CAP_RENDER_AOV) && last_batch) ? ns - 1 : ~0u;
        const uint32_t max_count  = ns * Ppad;

        ShadeArgs sa{};
        sa.scene = scene, sa.cam = cam, sa.screen = c->screen, sa.frames = frames;
        if (!fused) sa.hits = L.hits.p;  // (fused: the same word is sample_terms, set per bounce)
        sa.planes = Planes{L.pl_color.p, L.pl_direct.p, L.pl_albedo.p, c->aov_geo.p, c->aov_nd.p};
        sa.n_slots = ns, sa.num_bounces = D, sa.max_count = max_count, sa.aov_slot = aov_slot, sa.shaded_counter = c->shaded_counter.p;
        {
            // Screen-space culling of bounce 0 inverts primary_dir (camera.h:39-63) with the transpose of (right, up, forward), which is
            // the inverse only for an orthonormal basis.  With G = the basis' Gram matrix and skew = max |G - I|, a ray through the
            // sensor point (cx, cy, f) projects to (G c).x / (G c).z * f instead of cx: off by at most
            //   skew * (f + 2 |cx| + |cy| + |cx| (|cx| + |cy|) / f)  <=  skew * (f + sx + sy / 2 + (sx + sy) sx / (4 f))
            // on the sensor (|cx| <= sx / 2, |cy| <= sy / 2), i.e. skew * width * (f / sx + 1 + sy / (2 sx) + (sx + sy) / (4 f)) pixels,
            // and likewise in y.  The tiles' test (small_scene.hip stage_camera_pairs) grows every bound by kCameraCullPad = 2 pixels for this, the
            // rounding of the projection and nothing else (the jitter stays inside its pixel): the cull is on only while the worst-case
            // shift on the sensor is at most an eighth of that pad.  The rest is for vertices off the sensor, whose error grows with
            // the tangent of their angle to the axis (|cy| / f = 5, 79 degrees: five times the shift; tests/test_pair_culls_gpu.py C7
            // renders both at 0.24 pixels).  A telephoto lens or a wide image tightens the tolerance (f / sx = 500 at 72 pixels: 7e-6); a basis made by
            // normalising cross products (skew ~1e-7) passes up to f / sx * width ~ 2e6.  Beyond the tolerance every tile tests every pair.
            const bool no_cull = c->sw.on(SW_NO_CAMERA_CULL);  // A/B switch
            auto dotf = [](const float* x, const float* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
            const CapCameraData& cd = c->camera;
            const float skew = std::max({std::fabs(dotf(cd.right, cd.up)), std::fabs(dotf(cd.right, cd.forward)), std::fabs(dotf(cd.up, cd.forward)),
                                         std::fabs(dotf(cd.right, cd.right) - 1.f), std::fabs(dotf(cd.up, cd.up) - 1.f),
                                         std::fabs(dotf(cd.forward, cd.forward) - 1.f)});
            const double f = cd.focal_length, sx = cd.sensor_size[0], sy = cd.sensor_size[1];
            const double shift_x = (double)skew * c->screen.width * (f / sx + 1.0 + sy / (2.0 * sx) + (sx + sy) / (4.0 * f));
            const double shift_y = (double)skew * c->screen.height * (f / sy + 1.0 + sx / (2.0 * sy) + (sx + sy) / (4.0 * f));
            const bool   ortho   = skew < 1e-4f && shift_x <= 0.125 * (double)kCameraCullPad && shift_y <= 0.125 * (double)kCameraCullPad;  // (NaN: off)
            sa.cull_camera_pairs = (ortho && !no_cull) ? 1u : 0u;
            c->last_cull_camera_pairs = sa.cull_camera_pairs;
        }
        // Nobody reads this batch's planes but the resolve (plane read-backs and the reconstruction chain need CAP_RENDER_AOV)
        const bool no_albedo_w = c->sw.on(SW_NO_ALBEDO_IN_W);  // A/B switch
        sa.albedo_in_w = (!no_albedo_w && !feedback && !lowres && !(flags & CAP_RENDER_AOV) && (ext || scene.texture_count == 0)) ? 1u : 0u;  // (the EXT model's first-vertex albedo is 1: it folds kd into the throughput)
        // ... and on the small-scene path the constants bounce 0 would write into `direct` stay unwritten (ShadeArgs::code_in_color).  The
        // EXT model is left out: its bounce 0 adds emission to `direct` and its shadow rays are traced inline, so it keeps two planes.
        const bool no_plane_code = c->sw.on(SW_NO_PLANE_CODE);  // A/B switch
        sa.code_in_color = (sa.albedo_in_w && fused && !ext && !no_plane_code && trace_shade_has_code_form(bvh, scene)) ? 1u : 0u;
        if (feedback)  // g_color_history = combined_history[(frame_count + 1) % 2], raytracing_system.cpp:1754-1759
            sa.fb = FeedbackDev{camera_dev(c->prev_camera), c->post_prev_nd.p, c->post_chist[(frame_begin + 1) % 2].p};
        const bool no_inline_nee = c->sw.on(SW_NO_INLINE_NEE);  // A/B switch
        sa.inline_nee = (ext && fused && !no_inline_nee) ? 1u : 0u;
        const bool no_inline_probe = c->sw.on(SW_NO_INLINE_PROBE);  // A/B switch
        sa.inline_probe = (!ext && !feedback && fused && !no_inline_probe && c->tri_count <= kExhaustiveMax && bvh.fan_pair_count >= 1 &&
                           bvh.fan_pair_count <= kExhaustiveMax / 2)
                              ? 1u
                              : 0u;
        const bool no_wave_ring = c->sw.on(SW_NO_WAVE_RING);  // A/B switch
        sa.wave_ring = (sa.inline_probe && !no_wave_ring && (size_t)cfg.grid_blocks * (kBlock / 64) * 128 <= std::min(L.s_org.n, L.s_con.n)) ? 1u : 0u;  // (a grid beyond what ensure_lane sized the rings for: CAP_BLOCKS_PER_CU)
        LaunchCfg cfg_any    = cfg;
        cfg_any.any_no_probe = sa.inline_probe;
        bool primary_shaded = false;  // tree path: bounce 0's shading done by the camera-ray kernel
        // Camera rays of a DENSE scene.  The packet walk (one node sequence per 8x8-pixel tile) is the fast form while a tile's 64
        // rays meet few triangles: 9.3 per packet on the 262 k-triangle hall at 1080p (0.13 triangles per pixel).  At 16.8 M
        // triangles (8 per pixel) a tile covers hundreds of leaves, every lane pays for every one of them, and the stage was 7.2 of the
        // big_variant's 24 ms: there the rays go through k_trace_closest8 like extension rays do, one lane each.  Same hit rule, same
        // bits.  The wide view's padding budget assumes ray origins inside the scene bounds (wide_builder.cpp): a camera outside them
        // keeps the packet walk.
        // Shadow rays of the reference model where the tree is far beyond the caches: the wide view with lane refill instead of chunk
        // by chunk (trace8.hip k_trace_any8_refill).  Measured per 8 spp at 1080p, any-hit stage (tools/primary_ab.py): 262 k triangles
        // (21 MB of wide nodes and intersection records) 1.89 -> 1.99 ms, 4.2 M (325 MB) 3.02 -> 3.02, 16.8 M (1.3 GB) 5.46 -> 4.01:
        // lanes are throughput only where a step's round trip ends in HBM.  The switch sits at twice the 256-MiB Infinity Cache;
        // A/B: CAP_ANY_REFILL=0|1.
        bool any_refill = false;
        if (!fused && !ext && bvh.wide8_ok && c->tri_count > kExhaustiveMax)
        {
            const int force = (int)c->sw.v[SW_ANY_REFILL];
            const uint64_t tree_bytes = (uint64_t)c->wide8_nodes * kWideNodeStride * 4u + (uint64_t)c->tri_count * 64u;
            any_refill = force >= 0 ? force != 0 : tree_bytes >= kAnyRefillTreeBytes;
        }
        bool primary_wide = false;
        if (!fused && bvh.wide8_ok && c->tri_count > kExhaustiveMax)
        {
            const int force = (int)c->sw.v[SW_PRIMARY_WIDE];  // A/B switch: 0 never, 1 whenever allowed
            bool inside = true;
            for (int k = 0; k < 3; ++k)
                inside = inside && c->camera.position[k] >= c->bvh_info.bounds_lo[k] && c->camera.position[k] <= c->bvh_info.bounds_hi[k];
            const double per_pixel = (double)c->tri_count / std::max(1.0, (double)c->screen.width * c->screen.height);
            primary_wide = inside && (force >= 0 ? force != 0 : per_pixel >= kPrimaryWideTrianglesPerPixel);
        }
        if (sample_table)
        {
            launch_sample_terms(L.stream, scene.bluenoise, frames, ns, D, L.terms.p);
            c->last_terms = CapContext::LastTerms{frames, ns, D, lane};
            if (trace_launch(c, "sample_terms batch %u", batch)) return fail(CAP_ERR_HIP, "sample_terms failed");
        }
        // The camera-vertex form of this batch: bounce 0's rays once per jitter group into the table, its per-slot remainder at the head of
        // bounce 1's launch; no bounce-0 launch and no any-hit launch.  No gate on the slots per group: with ONE slot per group, where no
        // camera ray is shared, the form is still the faster one -- 1080p, tools/camera_table_small.py, ms per render off -> on: 1 slot
        // depth 1 0.1515 -> 0.1316, depth 2 0.2164 -> 0.1976; 2 slots 0.2261 -> 0.2017 and 0.3241 -> 0.2992 (docs/experiments.md (104)).
        const bool     camera_head = camera_table && sa.code_in_color && sa.wave_ring;
        const uint32_t n_groups    = camera_head ? batch_groups[batch] : 0u;
        float4* const  tab_p = L.camera.p, *const tab_n = L.camera.p + (size_t)n_groups * Ppad;
        if (camera_head)
        {
            StageTimer t(c, ST_PRIMARY, st);
            launch_camera_vertices(cfg, bvh, sa, n_groups, tab_p, tab_n);
            c->last_camera = CapContext::LastCamera{frames, ns, n_groups, lane};
            // every CapStats field keeps its value between the two forms: bounce 0's shadow rays are still one any-hit pass of the batch,
            // traced inside the fused launch instead of by a launch of their own
            ++c->stats.launches_trace_any;
            if (trace_launch(c, "camera_vertices batch %u", batch)) return fail(CAP_ERR_HIP, "camera_vertices failed");
        }
        c->last_camera_table = camera_head ? 1u : 0u;
        for (uint32_t b = camera_head ? 1u : 0u; b <= D; ++b)
        {
            const int pi = (int)(b & 1u), po = pi ^ 1;
            sa.bounce    = b;
            // bounce b's [slot][4096] block; the last bounce samples nothing and reads nothing, but takes the same form of kernel
            if (fused) sa.sample_terms = sample_table ? L.terms.p + (size_t)(b < D ? b : 0u) * ns * 4096 : nullptr;
            // (inline_nee: no shadow entries are written, so the shadow queue's two 16-byte planes carry the paths' gathered radiance)
            sa.in        = RayQueue{L.q_org[pi].p, L.q_dir[pi].p, L.q_thr[pi].p, b ? ext_count + (b - 1) * per_queue : nullptr, class_capacity,
                                    pi ? L.s_dir.p : L.s_org.p};
            sa.out       = RayQueue{L.q_org[po].p, L.q_dir[po].p, L.q_thr[po].p, ext_count + b * per_queue, class_capacity,
                                    po ? L.s_dir.p : L.s_org.p};
            sa.shadow    = ShadowQueue{L.s_org.p, L.s_dir.p, L.s_con.p, sh_count + b * per_queue, class_capacity};
            sa.work      = work_shade + b * per_queue;
            const bool head = camera_head && b == 1;
            // (the input queue of that launch is bounce 0's identity queue: its three planes carry the table and bounce 0's sample terms)
            if (head) sa.in = RayQueue{tab_p, tab_n, L.terms.p, ext_count, class_capacity, nullptr};
            if (fused)
            {
                StageTimer t(c, b == 0 ? ST_PRIMARY : ST_CLOSEST, st);
                const uint32_t form = launch_trace_shade(cfg, bvh, sa, ext, feedback, head);
                if (b) ++c->stats.launches_trace_closest, c->last_mark_form = form;
                if (trace_launch(c, "trace_shade bounce %u batch %u", b, batch)) return fail(CAP_ERR_HIP, "trace_shade failed");
            }
            else
            {
                if (b == 0)
                {
                    {
                        StageTimer t(c, ST_PRIMARY, st);
                        if (primary_wide)
                        {
                            // dense scene: camera rays as an identity queue through the wide per-lane kernel (see above)
                            const uint32_t id_cap = (((max_count + kQueueClasses - 1) / kQueueClasses) + 63u) & ~63u;
                            const RayQueue idq{L.q_org[0].p, L.q_dir[0].p, nullptr, L.counters.p + 3 * counter_words, id_cap, nullptr};
                            if (c->sw.on(SW_RAYGEN_KERNEL) || bvh.tri_count == 0)  // A/B switch: the identity queue written out by its own kernel
                            {
                                launch_raygen_identity(cfg, cam, c->screen, frames, ns, idq);
                                launch_trace_closest8(cfg, bvh, idq, max_count, L.hits.p, sa.work);
                            }
                            else
                                launch_trace_closest8_camera(cfg, bvh, idq, max_count, L.hits.p, sa.work, cam, c->screen, frames, ns);
                        }
                        else
                        {
                            primary_shaded = launch_primary_shade(cfg, bvh, sa, L.hits.p, ext);
                            if (!primary_shaded) launch_trace_primary(cfg, bvh, cam, c->screen, frames, ns, L.hits.p, sa.work);
                        }
                    }
                    if (aov_slot != ~0u) launch_geo_aov(cfg, scene, L.hits.p + (size_t)aov_slot * Ppad, Ppad, c->aov_geo.p);
                }
                if (b != 0 || !primary_shaded)
                {
                    StageTimer t(c, ST_SHADE, st, b == 0 ? ST_DIRECT : ST_NONE);
                    launch_shade(cfg, sa, ext, feedback);
                    ++c->stats.launches_shade;
                }
            }
            if (!sa.inline_nee && !(fused && sa.wave_ring && b != 0))
            {
                StageTimer t(c, ST_ANY, st, b == 0 ? ST_DIRECT : ST_NONE);
                if (any_refill)
                    launch_trace_any8_refill(cfg_any, bvh, sa.shadow, max_count, b == 0 ? L.pl_direct.p : L.pl_color.p, Ppad, ns, c->shaded_counter.p,
                                             work_any + b * per_queue, frames);
                else
                    launch_trace_any(cfg_any, bvh, sa.shadow, max_count, b == 0 ? L.pl_direct.p : L.pl_color.p, Ppad, ns, c->shaded_counter.p,
                                     work_any + b * per_queue, /* next-event estimation: most shadow rays reach the light */ ext, frames,
                                     (b == 0 && sa.code_in_color) ? L.pl_color.p : nullptr);
                ++c->stats.launches_trace_any;
                if (trace_launch(c, "trace_any bounce %u batch %u", b, batch)) return fail(CAP_ERR_HIP, "trace_any failed");
            }
            if (!fused && b < D)
            {
                StageTimer t(c, ST_CLOSEST, st);
                if (bvh.wide8_ok)  // bounce b + 1's slot of the fused kernels' grab counters is free on this path
                    launch_trace_closest8(cfg, bvh, sa.out, max_count, L.hits.p, work_shade + (b + 1) * per_queue);
                else
                    launch_trace_closest(cfg, bvh, sa.out, max_count, L.hits.p);
                ++c->stats.launches_trace_closest;
            }
        }
        if (!lowres)
        {
            StageTimer t(c, ST_RESOLVE, st);
            if (two_lanes && last_resolve) HIP_TRY(hipStreamWaitEvent(L.stream, last_resolve, 0));  // frame order of the additions
            launch_resolve(cfg, sa.planes, ns, Ppad, c->accum.p, sa.albedo_in_w != 0u, scene.kd_untextured, sa.code_in_color != 0u);
            if (two_lanes)
            {
                HIP_TRY(hipEventRecord(c->lane_ev[lane], L.stream));
                last_resolve = c->lane_ev[lane];
            }
        }
        // queue lengths of this batch -> pinned host memory, summed at the next sync
        uint32_t* pinned = nullptr;
        if (!c->pinned_pool.empty())
        {
            pinned = c->pinned_pool.back();
            c->pinned_pool.pop_back();
        }
        else
            HIP_TRY(hipHostMalloc((void**)&pinned, sizeof(uint32_t) * 2 * 256 * kQueueClasses * kCounterStride, hipHostMallocDefault));
        HIP_TRY(hipMemcpyAsync(pinned, L.counters.p, sizeof(uint32_t) * counter_words, hipMemcpyDeviceToHost, L.stream));
        c->pending.push_back({pinned, D | (sa.inline_nee ? 1u << 16 : 0u)});
        HIP_TRY(hipGetLastError());

        // primary rays: one per valid pixel per frame
        uint64_t valid = 0;
        for (uint32_t lt = 0; lt < c->screen.local_tiles; ++lt)
        {
            const uint32_t gt = lt * c->screen.shard_count + c->screen.shard_index;
            const uint32_t ty = gt / c->screen.tiles_x, tx = gt % c->screen.tiles_x;
            const uint32_t w = std::min(kTileDim, c->screen.width - tx * kTileDim), h = std::min(kTileDim, c->screen.height - ty * kTileDim);
            valid += (uint64_t)w * h;
        }
        c->stats.rays_primary += valid * ns;
        c->stats.frames += ns;
        if (!lowres) c->frames_accumulated += ns;
        c->last_slots = ns;
        c->aov_valid  = aov_slot != ~0u;
        c->aov_lowres = lowres;
        c->aov_frame  = frame_begin + done + ns - 1;
        // the next batch reuses counters/frames: serialise on the stream (already), and bound the event backlog
        if (c->spans.size() > 4096)
        {
            total.reset();
            if (two_lanes) HIP_TRY(hipStreamSynchronize(c->stream2));
            if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
            total.reset(new StageTimer(c, ST_COUNT));
        }
    }
    if (two_lanes)
    {
        // the context's stream -- the one callers order their work behind -- ends the call behind lane 1 as well
        HIP_TRY(hipEventRecord(c->join_ev, c->stream2));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->join_ev, 0));
        lane_join.armed = false;
    }
    total.reset();
    HIP_TRY(hipEventRecord(c->frames_event[ring], c->stream));
    return CAP_OK;
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
