// ctx_post.hip — the reconstruction chain behind cap_post_*: its images and histories, the AOV tile exchange of sharded contexts, the
// feedback import / export (kernels: post.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cap_context.h"

extern "C" {

void cap_post_settings_default(CapPostSettings* out)
{
    if (!out) return;
    *out = CapPostSettings{1, 1, 1, 128.0f, 3.0f, 3.0f, 64.0f, 2.0f, 3.0f, 0.975f, 0.9f, 0, 0, 0, 0};
}

int cap_post_reset(CapContext* c)
{
    if (!c) return fail(CAP_ERR_INVALID_ARG, "cap_post_reset: ctx is NULL");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_post_reset: resolution not set");
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = (size_t)c->screen.width * c->screen.height;
    DevBuf<float4>* all[] = {&c->post_in[0],   &c->post_in[1],   &c->post_in[2],   &c->post_in[3],  &c->post_ihist[0], &c->post_ihist[1],
                             &c->post_mhist[0], &c->post_mhist[1], &c->post_chist[0], &c->post_chist[1], &c->post_prev_nd, &c->post_itemp,
                             &c->post_temp[0],  &c->post_temp[1], &c->post_normals};
    for (DevBuf<float4>* b : all)
    {
        HIP_TRY(b->ensure(npix));
        HIP_TRY(hipMemsetAsync(b->p, 0, sizeof(float4) * npix, c->stream));  // the reference's textures start cleared
    }
    c->post_w = c->screen.width, c->post_h = c->screen.height;
    c->post_last_dst = -1;
    return CAP_OK;
}

// Common tail of cap_post_frame / cap_post_frame_gathered: the chain on post_in[0..3] (row-major, assembled from the ranks'
// gathered tiles), or -- `tiled` -- on this context's own tile-ordered planes
struct PostTiledInputs
{
    const float4 *indirect, *direct, *albedo, *normal_depth;
};
static int run_post_chain(CapContext* c, const CapPostSettings* s, uint32_t frame_count, const CapCameraData* prev_camera,
                          const PostTiledInputs* tiled = nullptr)
{
    PostChainArgs a{};
    a.settings = PostSettingsDev{s->gather, s->denoise, s->eaw5, s->eaw_normal_sigma, s->eaw_depth_sigma, s->eaw_luma_sigma, s->gather_normal_sigma,
                                 s->gather_depth_sigma, s->gather_luma_sigma, s->temporal_upscale_feedback, s->taa_feedback, s->lowres_indirect,
                                 s->disable_variance ? 0 : 1, s->fast_weights, s->output};
    a.width = c->screen.width, a.height = c->screen.height, a.frame_count = frame_count;
    a.camera = camera_dev(c->camera), a.prev_camera = camera_dev(*prev_camera);
    a.indirect = c->post_in[0].p, a.direct = c->post_in[1].p, a.albedo = c->post_in[2].p, a.normal_depth = c->post_in[3].p;
    if (tiled)
    {
        a.tiled = c->screen.tiles_x, a.screen = c->screen;
        a.tiled_indirect = tiled->indirect, a.tiled_normal_depth = tiled->normal_depth, a.indirect_rowmajor = c->post_in[0].p;
        a.direct = tiled->direct, a.albedo = tiled->albedo, a.normal_depth = nullptr;
    }
    for (int k = 0; k < 2; ++k)
        a.indirect_history[k] = c->post_ihist[k].p, a.moments_history[k] = c->post_mhist[k].p, a.combined_history[k] = c->post_chist[k].p,
        a.temp[k] = c->post_temp[k].p;
    a.prev_normal_depth = c->post_prev_nd.p, a.indirect_temp = c->post_itemp.p, a.normals = c->post_normals.p;
    // one timestamp per pass boundary, like the reference's AllocateTimestampQueryPair per pass (raytracing_system.cpp:1023-1035)
    struct Marks
    {
        CapContext* c;
        hipEvent_t  e[6];
    } marks{c, {}};
    a.mark_user = &marks;
    a.mark      = [](void* user, int pass) {
        Marks* m   = static_cast<Marks*>(user);
        m->e[pass] = get_event(m->c);
        (void)hipEventRecord(m->e[pass], m->c->stream);
    };
    launch_post_chain(c->stream, a);
    std::swap(c->post_prev_nd, c->post_normals);  // this frame's decoded normal/depth image is the next frame's previous one
    c->post_marks.push_back({marks.e[0], marks.e[1], marks.e[2], marks.e[3], marks.e[4], marks.e[5]});
    HIP_TRY(hipGetLastError());
    ++c->stats.post_frames;
    c->post_last_dst = (int)(frame_count % 2);
    return CAP_OK;
}

int cap_aov_tile_buffer_floats(CapContext* c, size_t* out_floats)
{
    if (!c || !out_floats) return fail(CAP_ERR_INVALID_ARG, "cap_aov_tile_buffer_floats: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_aov_tile_buffer_floats: resolution not set");
    *out_floats = (size_t)c->screen.pixels_padded * 4 * 4;
    return CAP_OK;
}

int cap_resolve_aov_tiles(CapContext* c, float* device_dst)
{
    if (!c || !device_dst) return fail(CAP_ERR_INVALID_ARG, "cap_resolve_aov_tiles: NULL argument");
    if (!c->aov_valid) return fail(CAP_ERR_STATE, "cap_resolve_aov_tiles: no frame rendered with CAP_RENDER_AOV");
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t Ppad  = c->screen.pixels_padded;
    const AovPlanes aov  = aov_planes(c);
    const size_t   bytes = sizeof(float4) * (size_t)Ppad;
    float4*        dst   = reinterpret_cast<float4*>(device_dst);
    // the four inputs of the chain, in its order (cap_post_frame): indirect, direct, albedo, normal/depth
    const float4* src[4] = {aov.color, aov.direct, aov.albedo, c->aov_nd.p};
    for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(dst + (size_t)k * Ppad, src[k], bytes, hipMemcpyDeviceToDevice, c->stream));
    return CAP_OK;
}

int cap_post_frame_gathered(CapContext* c, const CapPostSettings* s, uint32_t frame_count, const CapCameraData* prev_camera,
                            const float* device_gathered, uint32_t shard_count)
{
    if (!c || !s || !prev_camera || !device_gathered) return fail(CAP_ERR_INVALID_ARG, "cap_post_frame_gathered: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_post_frame_gathered: resolution not set");
    if (shard_count != c->screen.shard_count)
        return fail(CAP_ERR_INVALID_ARG, "cap_post_frame_gathered: shard_count %u != context's %u", shard_count, c->screen.shard_count);
    const bool lowres = s->lowres_indirect != 0;
    if (lowres && ((c->screen.width | c->screen.height) & 1u))
        return fail(CAP_ERR_INVALID_ARG, "cap_post_frame_gathered: lowres_indirect needs even width and height (%ux%u)", c->screen.width, c->screen.height);
    if (!(s->eaw_luma_sigma > 0.0f) || !(s->gather_luma_sigma > 0.0f)) return fail(CAP_ERR_INVALID_ARG, "cap_post_frame_gathered: luma sigmas must be > 0");
    if (s->output < CAP_OUTPUT_COMBINED || s->output > CAP_OUTPUT_VARIANCE) return fail(CAP_ERR_INVALID_ARG, "cap_post_frame_gathered: output %d is not one of CAP_OUTPUT_*", s->output);
    HIP_TRY(hipSetDevice(c->device));
    if (c->post_w != c->screen.width || c->post_h != c->screen.height)
        if (int e = cap_post_reset(c)) return e;
    const uint32_t Ppad = c->screen.pixels_padded;
    LaunchCfg      cfg{c->stream, (uint32_t)c->cu_count * 8u, 32};
    const float4*  g = reinterpret_cast<const float4*>(device_gathered);
    for (int k = lowres ? 1 : 0; k < 4; ++k) launch_assemble(cfg, c->screen, g + (size_t)k * Ppad, shard_count, c->post_in[k].p, (size_t)4 * Ppad);
    if (lowres)
    {
        // output_indirect_ is the (W/2, H/2) image of the pixels at this frame's interleave offset, as in cap_post_frame
        HIP_TRY(c->image_tmp.ensure((size_t)c->screen.width * c->screen.height));
        launch_assemble(cfg, c->screen, g, shard_count, c->image_tmp.p, (size_t)4 * Ppad);
        launch_decimate2x(c->stream, c->image_tmp.p, c->screen.width, c->screen.height, (frame_count % 4u) / 2u, (frame_count % 4u) % 2u,
                          c->post_in[0].p);
    }
    return run_post_chain(c, s, frame_count, prev_camera);
}

int cap_feedback_buffer_floats(CapContext* c, size_t* out_floats)
{
    if (!c || !out_floats) return fail(CAP_ERR_INVALID_ARG, "cap_feedback_buffer_floats: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_feedback_buffer_floats: resolution not set");
    *out_floats = (size_t)c->screen.width * c->screen.height * 4 * 2;
    return CAP_OK;
}

int cap_feedback_export(CapContext* c, float* device_dst)
{
    if (!c || !device_dst) return fail(CAP_ERR_INVALID_ARG, "cap_feedback_export: NULL argument");
    if (c->post_last_dst < 0 || c->post_w != c->screen.width || c->post_h != c->screen.height)
        return fail(CAP_ERR_STATE, "cap_feedback_export: the chain has not run at this resolution");
    HIP_TRY(hipSetDevice(c->device));
    const size_t npix = (size_t)c->post_w * c->post_h;
    float4*      dst  = reinterpret_cast<float4*>(device_dst);
    HIP_TRY(hipMemcpyAsync(dst, c->post_chist[c->post_last_dst].p, sizeof(float4) * npix, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dst + npix, c->post_prev_nd.p, sizeof(float4) * npix, hipMemcpyDeviceToDevice, c->stream));
    return CAP_OK;
}

int cap_feedback_import(CapContext* c, const float* device_src, uint32_t frame_count)
{
    if (!c || !device_src) return fail(CAP_ERR_INVALID_ARG, "cap_feedback_import: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_feedback_import: resolution not set");
    HIP_TRY(hipSetDevice(c->device));
    if (c->post_w != c->screen.width || c->post_h != c->screen.height)
        if (int e = cap_post_reset(c)) return e;
    const size_t  npix = (size_t)c->post_w * c->post_h;
    const float4* src  = reinterpret_cast<const float4*>(device_src);
    // what cap_render(frame_count + 1, CAP_RENDER_GBUFFER_FEEDBACK) reads: combined_history[(frame_count + 2) % 2] and the previous normal/depth
    HIP_TRY(hipMemcpyAsync(c->post_chist[frame_count % 2].p, src, sizeof(float4) * npix, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->post_prev_nd.p, src + npix, sizeof(float4) * npix, hipMemcpyDeviceToDevice, c->stream));
    return CAP_OK;
}

int cap_post_frame(CapContext* c, const CapPostSettings* s, uint32_t frame_count, const CapCameraData* prev_camera)
{
    if (!c || !s || !prev_camera) return fail(CAP_ERR_INVALID_ARG, "cap_post_frame: NULL argument");
    if (!c->screen.width) return fail(CAP_ERR_STATE, "cap_post_frame: resolution not set");
    if (c->screen.shard_count != 1) return fail(CAP_ERR_UNSUPPORTED, "cap_post_frame: needs an unsharded context (shard_count is %u)", c->screen.shard_count);
    if (!c->aov_valid) return fail(CAP_ERR_STATE, "cap_post_frame: no frame rendered with CAP_RENDER_AOV");
    if (!(s->eaw_luma_sigma > 0.0f) || !(s->gather_luma_sigma > 0.0f)) return fail(CAP_ERR_INVALID_ARG, "cap_post_frame: luma sigmas must be > 0");
    if (s->output < CAP_OUTPUT_COMBINED || s->output > CAP_OUTPUT_VARIANCE) return fail(CAP_ERR_INVALID_ARG, "cap_post_frame: output %d is not one of CAP_OUTPUT_*", s->output);
    HIP_TRY(hipSetDevice(c->device));
    if (c->post_w != c->screen.width || c->post_h != c->screen.height)
        if (int e = cap_post_reset(c)) return e;
    const AovPlanes aov = aov_planes(c);
    LaunchCfg       cfg{c->stream, (uint32_t)c->cu_count * 8u, 32};
    const bool lowres = s->lowres_indirect != 0;
    if (lowres != c->aov_lowres)
        return fail(CAP_ERR_STATE, "cap_post_frame: settings.lowres_indirect is %d but the frame was rendered %s CAP_RENDER_LOWRES_INDIRECT",
                    (int)lowres, c->aov_lowres ? "with" : "without");
    if (lowres && frame_count != c->aov_frame)
        return fail(CAP_ERR_INVALID_ARG, "cap_post_frame: frame_count %u is not the rendered frame %u (it selects the 2x2 interleave offset)", frame_count, c->aov_frame);
    if (lowres)
    {
        // output_indirect_ is the (W/2, H/2) image of the pixels at sp_offset (raytracing_system.cpp:499-512)
        HIP_TRY(c->image_tmp.ensure((size_t)c->screen.width * c->screen.height));
        launch_untile(cfg, c->screen, aov.color, nullptr, nullptr, 0, c->image_tmp.p);
        launch_decimate2x(c->stream, c->image_tmp.p, c->screen.width, c->screen.height, (frame_count % 4u) / 2u, (frame_count % 4u) % 2u,
                          c->post_in[0].p);
    }
    // the chain takes the render's tile-ordered planes as they are (PostChainArgs::tiled): its first kernel untiles the indirect
    // plane and decodes the normals in one pass, Combine reads direct / albedo in tile order
    PostTiledInputs ti{lowres ? nullptr : aov.color, aov.direct, aov.albedo, c->aov_nd.p};
    return run_post_chain(c, s, frame_count, prev_camera, &ti);
}

int cap_post_readback(CapContext* c, float* dst)
{
    if (!c || !dst) return fail(CAP_ERR_INVALID_ARG, "cap_post_readback: NULL argument");
    if (c->post_last_dst < 0) return fail(CAP_ERR_STATE, "cap_post_readback: cap_post_frame has not run");
    HIP_TRY(hipSetDevice(c->device));
    if (sync_and_collect(c) != CAP_OK) return CAP_ERR_HIP;
    HIP_TRY(hipMemcpy(dst, c->post_chist[c->post_last_dst].p, sizeof(float4) * (size_t)c->post_w * c->post_h, hipMemcpyDeviceToHost));
    return CAP_OK;
}
}  // extern "C"
