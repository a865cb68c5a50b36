// ctx_render.hip — cap_render, the MI355X counterpart of RaytracingSystem::Run (reference src/systems/raytracing_system.cpp:230-318, ray
// passes only).  A call is cut up in four steps, each its own function below (DESIGN.md "How a render is cut up"):
//   plan    plan_render + plan_forms: everything the call decides, into a RenderPlan that is read-only from then on
//   lanes   ensure_lanes: the one or two batch working sets (CapContext::Lane), with the fallback to one
//   batch   render_batch: the launch sequence of one batch of frame slots on its lane
//   bounce  fused_bounce (small-scene path: closest hit and shading in one launch) or tree_bounce + tree_next_hits, and shadow_rays
//
// The product path is HIP only: a missing device or kernel is CAP_ERR_HIP; there is no CPU fallback.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "cap_context.h"
#include "cap_wide.h"

namespace
{
// camera rays take the per-lane wide kernel instead of the packet walk from this many triangles per pixel on (measured: cap_render;
// 1.0 until the walk's node step was rewritten in round 6 -- at 1.0 the walk now wins by 6 % of the step, at 2.0 the two are level)
constexpr double kPrimaryWideTrianglesPerPixel = 2.0;
// shadow rays take the lane-refill kernel from this many bytes of wide nodes + intersection records on (measured: cap_render).
// Round 6: never by default.  Until the per-chunk kernel's traversal was compiled per light octant (docs/experiments.md (86)) the refill
// kernel won by 3 % from 512 MiB of tree on; now the per-chunk kernel wins by 6 - 8 % at 8.4 M and 16.8 M triangles (1.5 GB of tree),
// as it always did below.  CAP_ANY_REFILL=1 still selects the refill kernel (tests/test_fallback_kernels_gpu.py keeps it honest).
constexpr uint64_t kAnyRefillTreeBytes = ~0ull;

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
    // (ensure_lanes does not try a second working set of a size that has failed, or a larger one, again at once: see there)
    const bool failed_before =
        two_lanes && c->lane1_failed_paths && (uint64_t)slots * Ppad >= c->lane1_failed_paths && num_bounces >= c->lane1_failed_bounces;
    return BatchPolicy{slots, two_lanes, failed_before};
}

// Everything a cap_render call decides, decided once: plan_render fills the first part before anything is allocated, ensure_lanes
// settles two_lanes, plan_forms the fields that read the working sets; from then on the plan is read-only.  Each field's condition is
// written in exactly one place (DESIGN.md "How a render is cut up" has the table, and why none of them can differ between two
// batches or two lanes of a call).
struct RenderPlan
{
    uint32_t frame_begin = 0, n_frames = 0, num_bounces = 0, flags = 0;
    bool     ext = false, feedback = false, lowres = false, aov = false, stage_timers = false;  // the decoded flags
    // Which traversal path the render takes: the small-scene kernels (closest hit and shading fused in one launch per bounce, every
    // triangle tested) or the tree path.  stack_entries == 0 selects the former in the launchers.
    bool     tree_path = false, fused = false;
    uint32_t stack_entries = 0;
    uint32_t slots = 0, n_batches = 0;  // batch_policy's cut; n_batches == 0: nothing to render
    bool     two_lanes = false;         // batch_policy's wish until ensure_lanes, from then on what the call does
    bool     lane1_failed_before = false;
    uint32_t blocks_per_cu = 0;
    bool     sample_table = false;      // direction-sample terms from a per-batch table (ShadeArgs::sample_terms)
    bool     camera_table = false;      // the call sizes and groups for the camera-vertex table (camera_head: it also fits the rings)
    bool     gray_entries = false;      // the extension queues hold 32-byte entries, one throughput word (launch_trace_shade's gray)
    bool     sky_plane = false;         // the sky term as one store into Planes::sky, added by the resolve (launch_trace_shade's sky_plane); plan_render: the call sizes for it, plan_forms: it runs
    // Jitter groups: the slots of a batch by the bits of (jitter_x, jitter_y).  slot_group[f]: the group of frame f within its batch,
    // numbered in order of first appearance; group_first[batch start + g]: the first slot of group g.  A group need not be contiguous.
    // slot_order[batch start + k]: the batch's slots sorted by group, stable; batch_walk_m[batch]: the slots per group if every group
    // of the batch has as many (every 64-frame batch: 8), else 0 -- the head kernels' group walk (cap_device.h head_chunk) or slot-major.
    std::vector<uint32_t> slot_group, group_first, batch_groups, batch_walk_m;
    std::vector<uint8_t>  slot_order;
    uint32_t camera_groups = 0;         // the most groups of any batch (what sizes Lane::camera)
    uint32_t cull_camera_pairs = 0, albedo_in_w = 0, code_in_color = 0, inline_nee = 0, inline_probe = 0;  // ShadeArgs' words of the same names
    bool     ring_form = false;         // the shadow rays of the probing kernels may go through the wave rings, if those are large enough
    uint64_t valid_pixels = 0;          // of one frame on this shard: one primary ray each
    // plan_forms: what reads the working sets
    uint32_t wave_ring = 0;
    bool     camera_head = false, any_refill = false, primary_wide = false;
};

// One batch of a call: frames [first, first + ns) of it on `lane`.
struct Batch
{
    uint32_t          lane, first, ns, index, groups;  // groups: jitter groups of its slots (camera_head only, else 0)
    bool              last;
    const FrameConst* frames;                          // its frame constants on the device
};

// Element counts of one lane's working set for a plan: what ensure_lane allocates, and what ensure_lanes tests to learn whether a
// call grows a lane (growing frees the old buffers, so the streams are drained first)
struct LaneSizes
{
    size_t planes, queues, rings, counters, terms, camera, sky;
};

LaneSizes lane_sizes(const CapContext* c, const RenderPlan& p)
{
    LaneSizes z;
    z.planes = (size_t)p.slots * c->screen.pixels_padded;
    z.queues = z.planes + (size_t)kQueueClasses * 64;  // queue regions round up to whole chunks per class
    // the shadow queue's memory also holds the fused kernels' per-wave survivor rings (ShadeArgs::wave_ring): 128 entries for
    // every wave of the largest persistent grid (8 workgroups per CU)
    z.rings = std::max(z.queues, (size_t)std::max(c->cu_count, 1) * 8 * (kBlock / 64) * 128);
    z.counters = CounterLayout{p.num_bounces}.total();
    // the table of direction-sample terms (ShadeArgs::sample_terms): 4096 entries per frame slot and sampling bounce, 32 MB at 64 x 8
    z.terms = p.sample_table ? (size_t)p.slots * p.num_bounces * 4096 : 0;
    // the table of camera vertices (launch_camera_vertices): two planes of one entry per (jitter group, padded pixel), 0.5 GB at 8 groups of 1080p
    z.camera = 2 * (size_t)p.camera_groups * c->screen.pixels_padded;
    // the sky plane (Planes::sky): one float per path, 0.53 GB at 64 slots of 1080p
    z.sky = p.sky_plane ? z.planes : 0;
    return z;
}

bool lane_grows(const CapContext::Lane& L, const LaneSizes& z) { return L.pl_color.n < z.planes || L.counters.n < z.counters || L.terms.n < z.terms || L.camera.n < z.camera || L.pl_sky.n < z.sky; }

int ensure_lane(CapContext* c, CapContext::Lane& L, const LaneSizes& z)
{
    for (DevBuf<float4>* b : {&L.hits, &L.q_org[0], &L.q_org[1], &L.q_dir[0], &L.q_dir[1], &L.q_thr[0], &L.q_thr[1], &L.s_dir})
        HIP_TRY(b->ensure(z.queues));
    for (DevBuf<float4>* b : {&L.s_org, &L.s_con}) HIP_TRY(b->ensure(z.rings));
    for (DevBuf<float4>* b : {&L.pl_color, &L.pl_direct, &L.pl_albedo}) HIP_TRY(b->ensure(z.planes));
    HIP_TRY(L.counters.ensure(z.counters));
    if (z.terms) HIP_TRY(L.terms.ensure(z.terms));
    if (z.camera) HIP_TRY(L.camera.ensure(z.camera));
    if (z.sky) HIP_TRY(L.pl_sky.ensure(z.sky));
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

// The jitter groups of every batch of the plan (RenderPlan::slot_group): frame_const()'s jitter, compared bit for bit.
void jitter_groups(RenderPlan& p)
{
    p.slot_group.resize(p.n_frames), p.group_first.assign(p.n_frames, 0u), p.slot_order.resize(p.n_frames);
    for (uint32_t done = 0; done < p.n_frames; done += p.slots)
    {
        const uint32_t ns = std::min(p.slots, p.n_frames - done);
        uint32_t       ng = 0;
        for (uint32_t s = 0; s < ns; ++s)
        {
            float sx, sy, gx, gy;
            halton23(p.frame_begin + done + s, sx, sy);
            uint32_t g = 0;
            for (; g < ng; ++g)
            {
                halton23(p.frame_begin + done + p.group_first[done + g], gx, gy);
                if (memcmp(&gx, &sx, sizeof(float)) == 0 && memcmp(&gy, &sy, sizeof(float)) == 0) break;
            }
            if (g == ng) p.group_first[done + ng++] = s;
            p.slot_group[done + s] = g;
        }
        uint32_t at = 0, m = ns / ng;
        for (uint32_t g = 0; g < ng; ++g)
        {
            const uint32_t from = at;
            for (uint32_t s = 0; s < ns; ++s)
                if (p.slot_group[done + s] == g) p.slot_order[done + at++] = (uint8_t)s;  // (ns <= kMaxFrameSlots = 64)
            if (at - from != m) m = 0;
        }
        p.batch_groups.push_back(ng), p.batch_walk_m.push_back(m);
        p.camera_groups = std::max(p.camera_groups, ng);
    }
}

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
bool cull_camera_pairs(const CapContext* c)
{
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
    return ortho && !no_cull;
}

// Plan, part (a): validates the call and decides everything its sizes depend on.  Reads the context and changes nothing (like
// batch_policy, which it calls; it selects the context's device for that).  n_batches == 0 with CAP_OK: nothing to render.
int plan_render(const CapContext* c, uint32_t frame_begin, uint32_t n_frames, uint32_t num_bounces, uint32_t flags, RenderPlan& p)
{
    if (!c->bvh_ready) return fail(CAP_ERR_STATE, "cap_render: call cap_bvh_build first");
    if (c->bvh_stale) return fail(CAP_ERR_STATE, "cap_render: vertices changed; call cap_bvh_refit or cap_bvh_build");
    if (!c->camera_ready || !c->bluenoise_ready || !c->screen.width) return fail(CAP_ERR_STATE, "cap_render: camera, blue noise and resolution must be set");
    p.frame_begin = frame_begin, p.n_frames = n_frames, p.num_bounces = num_bounces, p.flags = flags;
    p.ext = (flags & CAP_RENDER_EXT_MATERIALS) != 0, p.feedback = (flags & CAP_RENDER_GBUFFER_FEEDBACK) != 0;
    p.lowres = (flags & CAP_RENDER_LOWRES_INDIRECT) != 0, p.aov = (flags & CAP_RENDER_AOV) != 0, p.stage_timers = (flags & CAP_RENDER_STAGE_TIMERS) != 0;
    const bool ext = p.ext, feedback = p.feedback, lowres = p.lowres;
    if (ext && !c->materials_ready) return fail(CAP_ERR_STATE, "cap_render: CAP_RENDER_EXT_MATERIALS needs cap_materials_upload (one material per mesh)");
    static_assert(sizeof(MaterialDev) == sizeof(CapMaterial), "material layouts must match");
    if (num_bounces > 255) return fail(CAP_ERR_INVALID_ARG, "cap_render: num_bounces %u exceeds 255", num_bounces);
    if (!n_frames) return CAP_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (feedback)
    {
        // the branch reads the previous frame's reconstruction output: one frame per call, the whole image on this context
        if (ext) return fail(CAP_ERR_UNSUPPORTED, "cap_render: CAP_RENDER_GBUFFER_FEEDBACK is defined for the reference shading model only");
        if (n_frames != 1) return fail(CAP_ERR_INVALID_ARG, "cap_render: CAP_RENDER_GBUFFER_FEEDBACK renders one frame per call (n_frames is %u)", n_frames);
        // sharded contexts: the previous frame's output reaches the non-root ranks through cap_feedback_import
        if (!c->prev_camera_ready) return fail(CAP_ERR_STATE, "cap_render: CAP_RENDER_GBUFFER_FEEDBACK needs cap_prev_camera_set");
    }
    if (lowres)
    {
        // the half-resolution indirect image only exists per frame (2x2 interleave over four frames): nothing to accumulate
        if (ext) return fail(CAP_ERR_UNSUPPORTED, "cap_render: CAP_RENDER_LOWRES_INDIRECT is defined for the reference shading model only");
        if (n_frames != 1) return fail(CAP_ERR_INVALID_ARG, "cap_render: CAP_RENDER_LOWRES_INDIRECT renders one frame per call (n_frames is %u)", n_frames);
        if ((c->screen.width | c->screen.height) & 1u) return fail(CAP_ERR_INVALID_ARG, "cap_render: CAP_RENDER_LOWRES_INDIRECT needs even width and height (%ux%u)", c->screen.width, c->screen.height);
    }
    if (c->traversal_mode == CAP_TRAVERSAL_EXHAUSTIVE && c->tri_count > 4096)
        return fail(CAP_ERR_UNSUPPORTED, "cap_render: exhaustive traversal refused for %u triangles", c->tri_count);
    p.tree_path     = c->traversal_mode == CAP_TRAVERSAL_EXHAUSTIVE ? false : !(c->traversal_mode == CAP_TRAVERSAL_AUTO && c->tri_count <= kExhaustiveMax);
    p.stack_entries = p.tree_path ? c->bvh_info.stack_entries : 0u;
    p.fused         = p.stack_entries == 0;  // small-scene path: closest hit and shading in one kernel per bounce
    const bool fused = p.fused;

    const BatchPolicy policy = batch_policy(c, n_frames, num_bounces, flags, p.tree_path);
    p.slots = policy.slots, p.two_lanes = policy.two_lanes, p.lane1_failed_before = policy.lane1_failed_before;
    p.n_batches = (n_frames + p.slots - 1) / p.slots;
    // Persistent grids must be fully resident: a workgroup that cannot be co-scheduled runs as a second round after the first
    // waves retire and doubles the kernel's tail.  blocks_per_cu is therefore the residency the kernels are built for
    // (launch bounds in kernels.hip and small_scene.hip), not the 8 a register-light kernel could reach.
    p.blocks_per_cu = fused ? 6u : (p.stack_entries <= 32 ? 5u : 2u);  // measured: 4..8 within 4 %, 6 best
    if (c->sw.v[SW_BLOCKS_PER_CU] >= 0) p.blocks_per_cu = (uint32_t)std::max<int64_t>(1, c->sw.v[SW_BLOCKS_PER_CU]);

    // (the two has_*_form questions read the triangle count and the scene's tame bit: nothing of a lane, nothing a render changes)
    const BvhDev   bvh   = bvh_dev(c, c->lane[0]);
    const SceneDev scene = scene_dev(c);
    // Direction-sample terms from a per-batch table: for every launch of every batch.  Rebuilt by every batch and never kept across
    // calls: frame_begin advances from call to call in real use.
    // A/B switch CAP_SAMPLE_TABLE: 0 never, 1 whenever the kernels have the form (which is also the product's choice).
    p.sample_table = fused && !ext && !feedback && num_bounces >= 1 && c->sw.get(SW_SAMPLE_TABLE, 1) != 0 && trace_shade_has_table_form(bvh, scene);
    // 32-byte extension entries: the table kernels on a scene without textures, where a throughput's three components are equal in every
    // bit.  For every launch of every batch: an entry of one form means nothing to a kernel of the other.  A/B switch CAP_NO_GRAY_ENTRIES.
    p.gray_entries = p.sample_table && trace_shade_has_gray_form(bvh, scene) && !c->sw.on(SW_NO_GRAY_ENTRIES);
    p.cull_camera_pairs = cull_camera_pairs(c) ? 1u : 0u;
    // Nobody reads a batch's planes but the resolve (plane read-backs and the reconstruction chain need CAP_RENDER_AOV)
    const bool no_albedo_w = c->sw.on(SW_NO_ALBEDO_IN_W);  // A/B switch
    p.albedo_in_w = (!no_albedo_w && !feedback && !lowres && !p.aov && (ext || scene.texture_count == 0)) ? 1u : 0u;  // (the EXT model's first-vertex albedo is 1: it folds kd into the throughput)
    // ... and on the small-scene path the constants bounce 0 would write into `direct` stay unwritten (ShadeArgs::code_in_color).  The
    // EXT model is left out: its bounce 0 adds emission to `direct` and its shadow rays are traced inline, so it keeps two planes.
    const bool no_plane_code = c->sw.on(SW_NO_PLANE_CODE);  // A/B switch
    p.code_in_color = (p.albedo_in_w && fused && !ext && !no_plane_code && trace_shade_has_code_form(bvh, scene)) ? 1u : 0u;
    const bool no_inline_nee = c->sw.on(SW_NO_INLINE_NEE);  // A/B switch
    p.inline_nee = (ext && fused && !no_inline_nee) ? 1u : 0u;
    // the producer of a shadow ray probes it against the pairs in LDS: where the model has the form, and where the pairs fit
    const bool no_inline_probe = c->sw.on(SW_NO_INLINE_PROBE);  // A/B switch
    const bool probe_form      = !ext && !feedback && fused && !no_inline_probe;
    p.inline_probe = (probe_form && c->tri_count <= kExhaustiveMax && bvh.fan_pair_count >= 1 && bvh.fan_pair_count <= kExhaustiveMax / 2) ? 1u : 0u;
    const bool no_wave_ring = c->sw.on(SW_NO_WAVE_RING);  // A/B switch
    p.ring_form = probe_form && !no_wave_ring;
    // Bounce 0 inside bounce 1's launch, from a table of camera vertices (launch_camera_vertices, launch_trace_shade's camera_head):
    // the lean table kernels in a render whose colour plane carries the first vertex's code and whose shadow rays may go through the
    // wave rings.  This much sizes the table and groups the slots; whether the rings hold the grid is plan_forms' to say (camera_head).
    // A/B switch CAP_NO_CAMERA_TABLE.
    p.camera_table = p.sample_table && p.code_in_color && p.ring_form && !c->sw.on(SW_NO_CAMERA_TABLE) && c->debug_capacity_div <= 1;
    if (p.camera_table) jitter_groups(p);
    // The sky term of an escaping path as one store into a write-only plane, added by the resolve, instead of three float atomics on
    // the colour plane: the 32-byte kernels of a batch whose first launch is the head (it zeroes the plane) and whose resolve is the
    // coded one (it adds the term).  code_in_color implies albedo_in_w, whose unused `albedo` word of Planes carries the plane, and no
    // AOV.  This much sizes the plane; like camera_head, whether it runs is plan_forms' to say.  A/B switch CAP_NO_SKY_PLANE.
    p.sky_plane = p.gray_entries && p.camera_table && p.code_in_color && !c->sw.on(SW_NO_SKY_PLANE);

    // primary rays: one per valid pixel per frame
    for (uint32_t lt = 0; lt < c->screen.local_tiles; ++lt)
    {
        const uint32_t gt = lt * c->screen.shard_count + c->screen.shard_index;
        const uint32_t ty = gt / c->screen.tiles_x, tx = gt % c->screen.tiles_x;
        const uint32_t w = std::min(kTileDim, c->screen.width - tx * kTileDim), h = std::min(kTileDim, c->screen.height - ty * kTileDim);
        p.valid_pixels += (uint64_t)w * h;
    }
    return CAP_OK;
}

// The plan's working sets: lane 0, the frame buffers, and lane 1 if the plan wants two lanes -- or the fallback to one, which
// settles p.two_lanes.  No host synchronisation with the previous call but where an allocation grows (which frees the old buffers).
int ensure_lanes(CapContext* c, RenderPlan& p)
{
    const uint32_t  Ppad = c->screen.pixels_padded;
    const LaneSizes need = lane_sizes(c, p);
    if (lane_grows(c->lane[0], need) || !c->accum.p || c->accum.n < Ppad) HIP_TRY(hipStreamSynchronize(c->stream));
    if (ensure_lane(c, c->lane[0], need) != CAP_OK || ensure_frame_buffers(c) != CAP_OK) return CAP_ERR_HIP;
    if (p.lane1_failed_before)
    {
        // this size has already failed: one lane, without asking again -- except every 32nd time, and at once when the device reports
        // room for it (memory can come back without any call on this context: another context closed, a co-tenant left)
        size_t free_b = 0, total_b = 0;
        const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > (size_t)p.slots * Ppad * 256u;  // a working set is ~208 B per path
        if (!room && (++c->lane1_retry_tick % 32u) != 0u)
        {
            p.two_lanes = false;
            ++c->stats.lane1_dropped;
        }
    }
    if (p.two_lanes)
    {
        if (lane_grows(c->lane[1], need))
        {
            HIP_TRY(hipStreamSynchronize(c->stream));  // growing frees the old buffers
            if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
        }
        if (c->debug_fail_lane || ensure_lane(c, c->lane[1], need) != CAP_OK || ensure_lane_streams(c) != CAP_OK)
        {
            // the second working set doubles the batch's memory (~28 GB at the default budget): without it the batches of this call
            // simply run one after the other on lane 0 -- counted in CapStats::lane1_dropped, and not tried again at this
            // size until something is freed
            (void)hipGetLastError();
            c->lane[1] = CapContext::Lane{};
            c->lane1_failed_paths = (uint64_t)p.slots * Ppad, c->lane1_failed_bounces = p.num_bounces;  // (ensure_lane's size depends on both)
            ++c->stats.lane1_dropped;
            p.two_lanes = false;
        }
    }
    return CAP_OK;
}

// Plan, part (b): the forms that read the working sets, fixed once the lanes are ensured.  What they read is the same for every
// batch: the rings are lane 0's (the fused path never runs two lanes), and bvh_dev's wide8_ok asks a lane only whether it has a
// spill area, which ensure_lane gives lane 1 exactly when lane 0 has one.
void plan_forms(const CapContext* c, RenderPlan& p)
{
    const CapContext::Lane& L   = c->lane[0];
    const BvhDev            bvh = bvh_dev(c, L);
    // (a grid beyond what ensure_lane sized the rings for -- CAP_BLOCKS_PER_CU -- unless an earlier, larger call left larger rings)
    p.wave_ring = (p.inline_probe && p.ring_form && (size_t)((uint32_t)c->cu_count * p.blocks_per_cu) * (kBlock / 64) * 128 <= std::min(L.s_org.n, L.s_con.n)) ? 1u : 0u;
    // The camera-vertex form: bounce 0's rays once per jitter group into the table, its per-slot remainder at the head of bounce 1's
    // launch; no bounce-0 launch and no any-hit launch.  No gate on the slots per group: with ONE slot per group, where no camera ray
    // is shared, the form is still the faster one -- 1080p, tools/camera_table_small.py, ms per render off -> on: 1 slot depth 1
    // 0.1515 -> 0.1316, depth 2 0.2164 -> 0.1976; 2 slots 0.2261 -> 0.2017 and 0.3241 -> 0.2992 (docs/experiments.md (104)).
    p.camera_head = p.camera_table && p.wave_ring;
    p.sky_plane   = p.sky_plane && p.camera_head;  // (gray_entries && camera_head && code_in_color, the switch off)
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
    const bool wide_tree = !p.fused && bvh.wide8_ok && c->tri_count > kExhaustiveMax;
    if (wide_tree && !p.ext)
    {
        const int force = (int)c->sw.v[SW_ANY_REFILL];
        const uint64_t tree_bytes = (uint64_t)c->wide8_nodes * kWideNodeStride * 4u + (uint64_t)c->tri_count * 64u;
        p.any_refill = force >= 0 ? force != 0 : tree_bytes >= kAnyRefillTreeBytes;
    }
    if (wide_tree)
    {
        const int force = (int)c->sw.v[SW_PRIMARY_WIDE];  // A/B switch: 0 never, 1 whenever allowed
        bool inside = true;
        for (int k = 0; k < 3; ++k)
            inside = inside && c->camera.position[k] >= c->bvh_info.bounds_lo[k] && c->camera.position[k] <= c->bvh_info.bounds_hi[k];
        const double per_pixel = (double)c->tri_count / std::max(1.0, (double)c->screen.width * c->screen.height);
        p.primary_wide = inside && (force >= 0 ? force != 0 : per_pixel >= kPrimaryWideTrianglesPerPixel);
    }
}

// The call's frame constants into the next slot of the ring, through pinned staging; *ring: the slot taken.
int upload_frame_constants(CapContext* c, const RenderPlan& p, uint32_t* ring_out)
{
    const uint32_t ring = *ring_out = c->frames_next;
    c->frames_next      = (c->frames_next + 1) % CapContext::kFrameRing;
    if (!c->frames_event[ring]) HIP_TRY(hipEventCreateWithFlags(&c->frames_event[ring], hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(c->frames_event[ring]));  // the call that used this slot kFrameRing calls ago: long done
    if (c->frames_ring[ring].n < p.n_frames)
    {
        // (a larger buffer: the old one of this slot is idle by the event above)
        HIP_TRY(c->frames_ring[ring].ensure(p.n_frames));
    }
    if (c->frames_pinned_n[ring] < p.n_frames)
    {
        if (c->frames_pinned[ring]) HIP_TRY(hipHostFree(c->frames_pinned[ring]));
        c->frames_pinned[ring] = nullptr;
        HIP_TRY(hipHostMalloc((void**)&c->frames_pinned[ring], sizeof(FrameConst) * p.n_frames, hipHostMallocDefault));
        c->frames_pinned_n[ring] = p.n_frames;
    }
    for (uint32_t f = 0; f < p.n_frames; ++f)
    {
        FrameConst& fc = c->frames_pinned[ring][f] = frame_const(p.frame_begin + f, p.lowres);
        // the two words nothing else reads in memory: the slot's jitter group, and the first slot of the group of this number
        if (p.camera_table) memcpy(&fc.pad1, &p.slot_group[f], 4), memcpy(&fc.pad2, &p.group_first[f], 4);
    }
    HIP_TRY(hipMemcpyAsync(c->frames_ring[ring].p, c->frames_pinned[ring], sizeof(FrameConst) * p.n_frames, hipMemcpyHostToDevice, c->stream));
    return CAP_OK;
}

// What a bounce's launches share: the batch's lane and its counters, the launch configuration and tree view of that lane.
struct BatchRun
{
    CapContext::Lane& L;
    BvhDev            bvh;
    LaunchCfg         cfg;
    CounterLayout     lay;
};

// Bounce b of the small-scene path: closest hit and shading in one launch (bounce 1 with the camera vertices at its head, if `head`).
int fused_bounce(CapContext* c, const RenderPlan& p, const Batch& bt, const BatchRun& r, const ShadeArgs& sa, bool head)
{
    StageTimer     t(c, sa.bounce == 0 ? ST_PRIMARY : ST_CLOSEST, p.stage_timers);
    const uint32_t form = launch_trace_shade(r.cfg, r.bvh, sa, p.ext, p.feedback, head, p.gray_entries, p.sky_plane);
    if (sa.bounce) ++c->stats.launches_trace_closest, c->last_mark_form = form;
    if (trace_launch(c, "trace_shade bounce %u batch %u", sa.bounce, bt.index)) return fail(CAP_ERR_HIP, "trace_shade failed");
    return CAP_OK;
}

// Bounce b of the tree path up to its shading: the camera rays (bounce 0) and the shade launch, unless the camera-ray kernel shaded.
void tree_bounce(CapContext* c, const RenderPlan& p, const Batch& bt, const BatchRun& r, const ShadeArgs& sa)
{
    CapContext::Lane& L = r.L;
    const uint32_t    Ppad = c->screen.pixels_padded;
    bool              primary_shaded = false;  // bounce 0's shading done by the camera-ray kernel
    if (sa.bounce == 0)
    {
        {
            StageTimer t(c, ST_PRIMARY, p.stage_timers);
            if (p.primary_wide)
            {
                // dense scene: camera rays as an identity queue through the wide per-lane kernel (plan_forms)
                const uint32_t id_cap = (((sa.max_count + kQueueClasses - 1) / kQueueClasses) + 63u) & ~63u;
                const RayQueue idq{L.q_org[0].p, L.q_dir[0].p, nullptr, r.lay.identity(L.counters.p), id_cap, nullptr};
                if (c->sw.on(SW_RAYGEN_KERNEL) || r.bvh.tri_count == 0)  // A/B switch: the identity queue written out by its own kernel
                {
                    launch_raygen_identity(r.cfg, sa.cam, c->screen, bt.frames, bt.ns, idq);
                    launch_trace_closest8(r.cfg, r.bvh, idq, sa.max_count, L.hits.p, sa.work);
                }
                else
                    launch_trace_closest8_camera(r.cfg, r.bvh, idq, sa.max_count, L.hits.p, sa.work, sa.cam, c->screen, bt.frames, bt.ns);
            }
            else
            {
                primary_shaded = launch_primary_shade(r.cfg, r.bvh, sa, L.hits.p, p.ext);
                if (!primary_shaded) launch_trace_primary(r.cfg, r.bvh, sa.cam, c->screen, bt.frames, bt.ns, L.hits.p, sa.work);
            }
        }
        if (sa.aov_slot != ~0u) launch_geo_aov(r.cfg, sa.scene, L.hits.p + (size_t)sa.aov_slot * Ppad, Ppad, c->aov_geo.p);
    }
    if (!primary_shaded)
    {
        StageTimer t(c, ST_SHADE, p.stage_timers, sa.bounce == 0 ? ST_DIRECT : ST_NONE);
        launch_shade(r.cfg, sa, p.ext, p.feedback);
        ++c->stats.launches_shade;
    }
}

// The shadow rays bounce b queued, either path: one any-hit launch, into the plane the bounce's light goes to.
int shadow_rays(CapContext* c, const RenderPlan& p, const Batch& bt, const BatchRun& r, const ShadeArgs& sa)
{
    CapContext::Lane& L = r.L;
    const uint32_t    b = sa.bounce, Ppad = c->screen.pixels_padded;
    StageTimer        t(c, ST_ANY, p.stage_timers, b == 0 ? ST_DIRECT : ST_NONE);
    LaunchCfg         cfg_any = r.cfg;
    cfg_any.any_no_probe      = p.inline_probe;
    float4* const   plane = b == 0 ? L.pl_direct.p : L.pl_color.p;
    uint32_t* const work  = r.lay.work_any(L.counters.p, b);
    if (p.any_refill)
        launch_trace_any8_refill(cfg_any, r.bvh, sa.shadow, sa.max_count, plane, Ppad, bt.ns, c->shaded_counter.p, work, bt.frames);
    else
        launch_trace_any(cfg_any, r.bvh, sa.shadow, sa.max_count, plane, Ppad, bt.ns, c->shaded_counter.p, work,
                         /* next-event estimation: most shadow rays reach the light */ p.ext, bt.frames, (b == 0 && p.code_in_color) ? L.pl_color.p : nullptr);
    ++c->stats.launches_trace_any;
    if (trace_launch(c, "trace_any bounce %u batch %u", b, bt.index)) return fail(CAP_ERR_HIP, "trace_any failed");
    return CAP_OK;
}

// Tree path: the closest hits of the rays bounce b queued, for bounce b + 1 to shade.
void tree_next_hits(CapContext* c, const RenderPlan& p, const BatchRun& r, const ShadeArgs& sa)
{
    StageTimer t(c, ST_CLOSEST, p.stage_timers);
    if (r.bvh.wide8_ok)  // bounce b + 1's slot of the fused kernels' grab counters is free on this path
        launch_trace_closest8(r.cfg, r.bvh, sa.out, sa.max_count, r.L.hits.p, r.lay.work_shade(r.L.counters.p, sa.bounce + 1));
    else
        launch_trace_closest(r.cfg, r.bvh, sa.out, sa.max_count, r.L.hits.p);
    ++c->stats.launches_trace_closest;
}

// What the camera-vertex table of batch `bt` is built from (CapContext::CameraTableKey), and whether two such keys name one table.
CapContext::CameraTableKey camera_table_key(const CapContext* c, const RenderPlan& p, const Batch& bt, const BvhDev& bvh, const ShadeArgs& sa)
{
    CapContext::CameraTableKey k;
    k.valid = true, k.cam = sa.cam, k.screen = sa.screen, k.n_groups = bt.groups, k.lane = bt.lane, k.cull_camera_pairs = sa.cull_camera_pairs;
    k.tri_count = bvh.tri_count, k.fan_pair_count = bvh.fan_pair_count, k.fan_single_count = bvh.fan_single_count, k.tri_ids_dense = bvh.tri_ids_dense;
    memcpy(&k.kd_untextured, &sa.scene.kd_untextured, 4);
    for (uint32_t g = 0; g < bt.groups && g < kMaxFrameSlots; ++g)
    {
        float jx, jy;
        halton23(p.frame_begin + bt.first + p.group_first[bt.first + g], jx, jy);  // frame_const()'s jitter of the group's first slot
        memcpy(&k.jitter[g][0], &jx, 4), memcpy(&k.jitter[g][1], &jy, 4);
    }
    k.table = c->lane[bt.lane].camera.p, k.table_n = c->lane[bt.lane].camera.n;
    k.records[0] = sa.scene.shade_tris, k.records[1] = bvh.tris_by_id, k.records[2] = bvh.fan_pairs, k.records[3] = bvh.fan_singles;
    k.scene_generation = c->scene_generation;
    return k;
}
bool same_camera_table(const CapContext::CameraTableKey& a, const CapContext::CameraTableKey& b)
{
    return a.valid && b.valid && memcmp(&a.cam, &b.cam, sizeof(CameraDev)) == 0 && memcmp(&a.screen, &b.screen, sizeof(ScreenDev)) == 0 &&
           a.n_groups == b.n_groups && a.lane == b.lane && a.cull_camera_pairs == b.cull_camera_pairs && a.tri_count == b.tri_count &&
           a.fan_pair_count == b.fan_pair_count && a.fan_single_count == b.fan_single_count && a.tri_ids_dense == b.tri_ids_dense &&
           a.kd_untextured == b.kd_untextured && memcmp(a.jitter, b.jitter, sizeof(a.jitter)) == 0 && a.table == b.table && a.table_n == b.table_n &&
           memcmp(a.records, b.records, sizeof(a.records)) == 0 && a.scene_generation == b.scene_generation;
}

// One batch: the launch sequence of its frame slots on its lane.  call_args: the ShadeArgs words that hold for the whole call.
// last_resolve: the accumulation buffer takes the batches in frame order, whichever lane ran them.
int render_batch(CapContext* c, const RenderPlan& p, const Batch& bt, const ShadeArgs& call_args, hipEvent_t& last_resolve)
{
    CapContext::Lane& L    = c->lane[bt.lane];
    const uint32_t    Ppad = c->screen.pixels_padded, D = p.num_bounces, ns = bt.ns;
    BatchRun          r{L, bvh_dev(c, L), LaunchCfg{L.stream, (uint32_t)c->cu_count * p.blocks_per_cu, p.stack_entries, (uint32_t)c->cu_count},
               CounterLayout{D}};
    r.cfg.sw = &c->sw;
    // (the three sections; the identity queue's counters behind them are not cleared here)
    HIP_TRY(hipMemsetAsync(L.counters.p, 0, sizeof(uint32_t) * 3 * r.lay.section(), L.stream));
    const uint32_t total_chunks   = ns * (Ppad >> 6);
    uint32_t       class_capacity = ((total_chunks + kQueueClasses - 1) / kQueueClasses) * 64u;
    // (tests of the append guard: sub-queues deliberately too small -- the appends beyond them must be dropped and counted)
    if (c->debug_capacity_div > 1) class_capacity = std::max(64u, (class_capacity / c->debug_capacity_div) & ~63u);
    c->last_class_capacity = class_capacity;

    ShadeArgs sa = call_args;
    sa.frames    = bt.frames;
    if (!p.fused) sa.hits = L.hits.p;  // (fused: the same word is sample_terms, set per bounce)
    sa.planes = Planes{L.pl_color.p, L.pl_direct.p, {L.pl_albedo.p}, c->aov_geo.p, c->aov_nd.p};
    if (p.sky_plane) sa.planes.sky = L.pl_sky.p, c->last_sky = CapContext::LastSky{1u, ns, bt.lane};  // (albedo_in_w: nobody reads `albedo`)
    sa.n_slots = ns, sa.max_count = ns * Ppad, sa.aov_slot = (p.aov && bt.last) ? ns - 1 : ~0u;

    if (p.sample_table)
    {
        launch_sample_terms(L.stream, sa.scene.bluenoise, bt.frames, ns, D, L.terms.p);
        c->last_terms = CapContext::LastTerms{bt.frames, ns, D, bt.lane};
        if (trace_launch(c, "sample_terms batch %u", bt.index)) return fail(CAP_ERR_HIP, "sample_terms failed");
    }
    float4* const tab_p = L.camera.p, *const tab_n = L.camera.p + (size_t)bt.groups * Ppad;
    if (p.camera_head)
    {
        StageTimer t(c, ST_PRIMARY, p.stage_timers);
        // The table depends on the slots through their groups' jitters alone, and any 64 consecutive frames hold the same eight: while
        // the camera stands still -- progressive accumulation -- every batch of every call would build the table the lane already holds.
        // Built only where its inputs differ from what the lane's table was built from.  A/B switch CAP_NO_TABLE_REUSE.
        const CapContext::CameraTableKey key = camera_table_key(c, p, bt, r.bvh, sa);
        CapContext::CameraTableKey&      have = c->camera_key[bt.lane];
        const bool reuse = !c->sw.on(SW_NO_TABLE_REUSE) && same_camera_table(have, key);
        if (!reuse)
        {
            have.valid = false;  // (until the launch is known to be queued)
            launch_camera_vertices(r.cfg, r.bvh, sa, bt.groups, tab_p, tab_n);
        }
        c->last_camera_reused = reuse ? 1u : 0u;
        c->last_camera = CapContext::LastCamera{bt.frames, ns, bt.groups, bt.lane};
        // every CapStats field keeps its value between the two forms: bounce 0's shadow rays are still one any-hit pass of the batch,
        // traced inside the fused launch instead of by a launch of their own
        ++c->stats.launches_trace_any;
        if (trace_launch(c, "camera_vertices batch %u", bt.index)) return fail(CAP_ERR_HIP, "camera_vertices failed");
        have = key;  // (a launch that could not be queued fails the call at the batch's end, and a failed call drops every key)
    }
    c->last_camera_table = p.camera_head ? 1u : 0u;
    // The order of bounce 0's chunks in the head kernel: the group walk where every jitter group of the batch has m slots, else (and under
    // the A/B switch CAP_NO_GROUP_WALK) slot-major, which is m = 1 with the identity order.
    HeadWalk walk{};
    if (p.camera_head)
    {
        const uint32_t m = c->sw.on(SW_NO_GROUP_WALK) ? 0u : p.batch_walk_m[bt.index];
        uint8_t        identity[kMaxFrameSlots];
        for (uint32_t s = 0; s < kMaxFrameSlots; ++s) identity[s] = (uint8_t)s;
        walk = head_walk(m ? m : 1u, Ppad >> 6, m ? &p.slot_order[bt.first] : identity, ns);
        c->last_group_walk = m;
    }
    // (the reference model's 48-byte queues of this batch, for CAP_DEBUG_SELFTEST_GRAY: under camera_head bounce 0 appends nothing)
    c->last_queues = CapContext::LastQueues{D, p.camera_head ? 1u : 0u, class_capacity, bt.lane, p.fused && !p.ext && !p.gray_entries};
    for (uint32_t b = p.camera_head ? 1u : 0u; b <= D; ++b)
    {
        const int pi = (int)(b & 1u), po = pi ^ 1;
        sa.bounce    = b;
        // bounce b's [slot][4096] block; the last bounce samples nothing and reads nothing, but takes the same form of kernel
        if (p.fused) sa.sample_terms = p.sample_table ? L.terms.p + (size_t)(b < D ? b : 0u) * ns * 4096 : nullptr;
        // (inline_nee: no shadow entries are written, so the shadow queue's two 16-byte planes carry the paths' gathered radiance)
        sa.in     = RayQueue{L.q_org[pi].p, L.q_dir[pi].p, L.q_thr[pi].p, b ? r.lay.ext(L.counters.p, b - 1) : nullptr, class_capacity, pi ? L.s_dir.p : L.s_org.p};
        sa.out    = RayQueue{L.q_org[po].p, L.q_dir[po].p, L.q_thr[po].p, r.lay.ext(L.counters.p, b), class_capacity, po ? L.s_dir.p : L.s_org.p};
        sa.shadow = ShadowQueue{L.s_org.p, L.s_dir.p, L.s_con.p, r.lay.shadow(L.counters.p, b), class_capacity};
        sa.work   = r.lay.work_shade(L.counters.p, b);
        const bool head = p.camera_head && b == 1;
        // (gray_entries: the same buffers; the two queues' thr_pid planes are neither read nor written, and an entry's words are RayQueue's
        // 32-byte layout)
        // (the input queue of that launch is bounce 0's identity queue: its three planes carry the table and bounce 0's sample terms)
        if (head) sa.in = RayQueue{tab_p, tab_n, L.terms.p, r.lay.ext(L.counters.p, 0), class_capacity, nullptr};
        if (head) sa.walk = walk;
        if (p.fused)
        {
            if (int e = fused_bounce(c, p, bt, r, sa, head)) return e;
        }
        else
            tree_bounce(c, p, bt, r, sa);
        // (no launch where the shading kernel traced its shadow rays itself: the EXT model inline, the rings' kernels from bounce 1 on)
        if (!p.inline_nee && !(p.fused && p.wave_ring && b != 0))
            if (int e = shadow_rays(c, p, bt, r, sa)) return e;
        if (!p.fused && b < D) tree_next_hits(c, p, r, sa);
    }
    if (!p.lowres)
    {
        StageTimer t(c, ST_RESOLVE, p.stage_timers);
        if (p.two_lanes && last_resolve) HIP_TRY(hipStreamWaitEvent(L.stream, last_resolve, 0));  // frame order of the additions
        launch_resolve(r.cfg, sa.planes, ns, Ppad, c->accum.p, p.albedo_in_w != 0u, sa.scene.kd_untextured, p.code_in_color != 0u, p.sky_plane);
        if (p.two_lanes)
        {
            HIP_TRY(hipEventRecord(c->lane_ev[bt.lane], L.stream));
            last_resolve = c->lane_ev[bt.lane];
        }
    }
    // queue lengths of this batch -> pinned host memory, summed at the next sync
    uint32_t* pinned = nullptr;
    if (!c->pinned_pool.empty())
    {
        pinned = c->pinned_pool.back();
        c->pinned_pool.pop_back();
    }
    else  // sized for the deepest call there can be, not for this one: pooled buffers serve later calls of other depths
        HIP_TRY(hipHostMalloc((void**)&pinned, sizeof(uint32_t) * CounterLayout{255}.section(), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(pinned, L.counters.p, sizeof(uint32_t) * r.lay.section(), hipMemcpyDeviceToHost, L.stream));
    c->pending.push_back({pinned, BatchCounted{D, p.inline_nee == 0u}});
    HIP_TRY(hipGetLastError());

    c->stats.rays_primary += p.valid_pixels * ns;
    c->stats.frames += ns;
    if (!p.lowres) c->frames_accumulated += ns;
    c->last_slots = ns;
    c->aov_valid  = sa.aov_slot != ~0u;
    c->aov_lowres = p.lowres;
    c->aov_frame  = p.frame_begin + bt.first + ns - 1;
    return CAP_OK;
}
}  // namespace

static int render_call(CapContext* c, uint32_t frame_begin, uint32_t n_frames, uint32_t num_bounces, uint32_t flags);
extern "C" int cap_render(CapContext* c, uint32_t frame_begin, uint32_t n_frames, uint32_t num_bounces, uint32_t flags)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_render: ctx is NULL");
    const int e = render_call(c, frame_begin, n_frames, num_bounces, flags);
    // a call that was refused or failed vouches for no table: the next one builds
    if (e != CAP_OK) c->camera_key[0].valid = c->camera_key[1].valid = false;
    return e;
}
static int render_call(CapContext* c, uint32_t frame_begin, uint32_t n_frames, uint32_t num_bounces, uint32_t flags)
{
    RenderPlan p;
    if (int e = plan_render(c, frame_begin, n_frames, num_bounces, flags, p)) return e;
    if (!p.n_batches) return CAP_OK;
    // the debug state of a call (cap_debug_get), from the plan; what a batch leaves is reset until the first batch writes it
    c->last_mark_form = 0, c->last_sample_table = p.sample_table ? 1u : 0u, c->last_cull_camera_pairs = p.cull_camera_pairs;
    c->last_terms = CapContext::LastTerms{}, c->last_camera_table = 0, c->last_camera = CapContext::LastCamera{}, c->last_group_walk = 0, c->last_camera_reused = 0;
    c->last_gray_entries = p.gray_entries ? 1u : 0u, c->last_queues = CapContext::LastQueues{}, c->last_sky = CapContext::LastSky{};
    if (p.feedback && (c->post_w != c->screen.width || c->post_h != c->screen.height))
        if (int e = cap_post_reset(c)) return e;  // first frame: cleared histories, every vertex is a disocclusion
    // No host synchronisation with the previous call: everything it still uses is either ordered behind it on the stream (queues,
    // counters, planes) or lives in another slot of the constants ring.  Only a long backlog of unread events / counters is
    // drained (what cap_sync / cap_stats_get do anyway), and a growing allocation (ensure_lanes).
    if (c->spans.size() > 2048 || c->pending.size() > 64 || c->post_marks.size() > 256)
        if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    if (int e = ensure_lanes(c, p)) return e;
    plan_forms(c, p);
    c->lanes_last_render = p.two_lanes ? 2u : 1u;
    uint32_t ring = 0;
    if (int e = upload_frame_constants(c, p, &ring)) return e;
    if (c->textures_dirty)
    {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->textures.ensure(std::max<size_t>(1, c->texture_host.size())));
        if (!c->texture_host.empty())
            HIP_TRY(hipMemcpy(c->textures.p, c->texture_host.data(), sizeof(TextureDev) * c->texture_host.size(), hipMemcpyHostToDevice));
        c->textures_dirty = false;
    }
    // the ShadeArgs words of the whole call; render_batch adds its lane's buffers and its slots
    ShadeArgs call_args{};
    call_args.scene = scene_dev(c), call_args.cam = camera_dev(c->camera), call_args.screen = c->screen;
    call_args.num_bounces = num_bounces, call_args.shaded_counter = c->shaded_counter.p;
    call_args.cull_camera_pairs = p.cull_camera_pairs, call_args.albedo_in_w = p.albedo_in_w, call_args.code_in_color = p.code_in_color;
    call_args.inline_nee = p.inline_nee, call_args.inline_probe = p.inline_probe, call_args.wave_ring = p.wave_ring;
    if (p.feedback)  // g_color_history = combined_history[(frame_count + 1) % 2], raytracing_system.cpp:1754-1759
        call_args.fb = FeedbackDev{camera_dev(c->prev_camera), c->post_prev_nd.p, c->post_chist[(frame_begin + 1) % 2].p};
    std::unique_ptr<StageTimer> total(new StageTimer(c, ST_COUNT));  // its destructor closes the span on every exit path

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
    if (p.two_lanes)
    {
        // lane 1 starts behind everything queued on the context's stream so far (the frame constants' upload, earlier calls)
        HIP_TRY(hipEventRecord(c->fork_ev, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->stream2, c->fork_ev, 0));
        lane_join.armed = true;
    }
    hipEvent_t last_resolve = nullptr;
    for (uint32_t k = 0, done = 0; done < n_frames; done += p.slots, ++k)
    {
        const uint32_t ns = std::min(p.slots, n_frames - done);
        const Batch    bt{p.two_lanes ? ((p.n_batches - 1u - k) & 1u) : 0u,  // the last batch on lane 0
                       done, ns, k, p.camera_head ? p.batch_groups[k] : 0u, done + ns >= n_frames, c->frames_ring[ring].p + done};
        if (int e = render_batch(c, p, bt, call_args, last_resolve)) return e;
        // the next batch reuses counters/frames: serialise on the stream (already), and bound the event backlog
        if (c->spans.size() > 4096)
        {
            total.reset();
            if (p.two_lanes) HIP_TRY(hipStreamSynchronize(c->stream2));
            if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
            total.reset(new StageTimer(c, ST_COUNT));
        }
    }
    if (p.two_lanes)
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
