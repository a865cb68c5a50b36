// planes.hip — image-plane kernels of the wavefront path tracer: resolve into the accumulator, tile / untile, shard assembly and
// the geometry AOV.
#include "cap_kernels.h"

#include <algorithm>

namespace cap
{
// ------------------------------------------------------------------------------------------------
// Accumulate / exchange
// ------------------------------------------------------------------------------------------------
// combine_illumination.hlsl:29 per frame, then a plain running fp32 sum in frame order.
// ALBEDO_IN_W (ShadeArgs::albedo_in_w): no albedo plane; direct.w says which of the four constant albedos the path's first vertex has
// (the form with the code in color.w is k_resolve_coded below)
template <bool ALBEDO_IN_W>
__global__ __launch_bounds__(kBlock) void k_resolve(Planes planes, uint32_t n_slots, uint32_t Ppad, float4* accum, float kd_untextured)
{
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < Ppad; pl += gridDim.x * kBlock)
    {
        float4 acc = accum[pl];
        for (uint32_t s = 0; s < n_slots; ++s)
        {
            const size_t idx = (size_t)s * Ppad + pl;
            const float4 c = planes.color[idx], d = planes.direct[idx];
            float4       al;
            if (ALBEDO_IN_W)
            {
                const float k = d.w == 1.0f ? 1.0f : (d.w == 2.0f ? kd_untextured : 0.0f);
                al            = make_float4(k, k, k, 0.f);
            }
            else
                al = planes.albedo[idx];
            acc.x = acc.x + (c.x * al.x + d.x);
            acc.y = acc.y + (c.y * al.y + d.y);
            acc.z = acc.z + (c.z * al.z + d.z);
            acc.w = acc.w + 1.0f;
        }
        accum[pl] = acc;
    }
}

// ShadeArgs::code_in_color: the code is color.w -- 0 padding, 1 sky, 2 the untextured kd, 3 black, and + 4 where the bounce-0 any-hit
// launch stored a contribution into `direct`.  Everything else `direct` would hold is a constant the code names (zeros; the sky's
// (0.7, 0.7, 0.85)), so the plane is loaded only under the flag: the same expression on the same values as k_resolve<true>, and an
// entry of `direct` that an earlier batch left behind is not looked at.
// The slots of a pixel go eight at a time: the eight colour loads, then the `direct` loads they ask for, all in flight together (a
// slot-by-slot loop would chain two round trips per slot), then the additions in slot order.
__global__ __launch_bounds__(kBlock) void k_resolve_coded(Planes planes, uint32_t n_slots, uint32_t Ppad, float4* accum, float kd_untextured)
{
    constexpr uint32_t kGroup = 8;
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < Ppad; pl += gridDim.x * kBlock)
    {
        float4 acc = accum[pl];
        for (uint32_t s0 = 0; s0 < n_slots; s0 += kGroup)
        {
            float4 c[kGroup], d[kGroup];
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k)
            {
                c[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s0 + k < n_slots) c[k] = planes.color[(size_t)(s0 + k) * Ppad + pl];
            }
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k)
            {
                d[k] = c[k].w == kCodeSky ? make_float4(0.7f, 0.7f, 0.85f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (c[k].w >= kCodeLit) d[k] = planes.direct[(size_t)(s0 + k) * Ppad + pl];  // (never on a slot behind n_slots: its c is 0)
            }
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k)
                if (s0 + k < n_slots)
                {
                    const float code = c[k].w >= kCodeLit ? c[k].w - kCodeLit : c[k].w;
                    const float al   = code == kCodeSky ? 1.0f : (code == kCodeKd ? kd_untextured : 0.0f);
                    acc.x = acc.x + (c[k].x * al + d[k].x);
                    acc.y = acc.y + (c[k].y * al + d[k].y);
                    acc.z = acc.z + (c[k].z * al + d[k].z);
                    acc.w = acc.w + 1.0f;
                }
        }
        accum[pl] = acc;
    }
}

// The sky-plane form (launch_trace_shade's sky_plane): k_resolve_coded, and the sky term of every path added here.  planes.sky holds the
// throughput of a path that escaped at bounce >= 1 and +0 for every other (cap_shade.h shade_vertex has the argument why the sums
// below are the bits the atomics on the colour plane left).  The eight sky loads of a group go out with its eight colour loads: no
// round trip is added.  t7 serves x and y as it does in the kernels' atomic form; the products stay products and the sums sums
// (-ffp-contract=off).
__global__ __launch_bounds__(kBlock) void k_resolve_coded_sky(Planes planes, uint32_t n_slots, uint32_t Ppad, float4* accum, float kd_untextured)
{
    constexpr uint32_t kGroup = 8;
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < Ppad; pl += gridDim.x * kBlock)
    {
        float4 acc = accum[pl];
        for (uint32_t s0 = 0; s0 < n_slots; s0 += kGroup)
        {
            float4 c[kGroup], d[kGroup];
            float  s[kGroup];
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k)
            {
                c[k] = make_float4(0.f, 0.f, 0.f, 0.f), s[k] = 0.0f;
                if (s0 + k < n_slots) c[k] = planes.color[(size_t)(s0 + k) * Ppad + pl], s[k] = planes.sky[(size_t)(s0 + k) * Ppad + pl];
            }
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k)
            {
                d[k] = c[k].w == kCodeSky ? make_float4(0.7f, 0.7f, 0.85f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (c[k].w >= kCodeLit) d[k] = planes.direct[(size_t)(s0 + k) * Ppad + pl];  // (never on a slot behind n_slots: its c is 0)
            }
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k)
                if (s0 + k < n_slots)
                {
                    const float code = c[k].w >= kCodeLit ? c[k].w - kCodeLit : c[k].w;
                    const float al   = code == kCodeSky ? 1.0f : (code == kCodeKd ? kd_untextured : 0.0f);
                    const float t7 = s[k] * 0.7f, t85 = s[k] * 0.85f;
                    const float cx = c[k].x + t7, cy = c[k].y + t7, cz = c[k].z + t85;
                    acc.x = acc.x + (cx * al + d[k].x);
                    acc.y = acc.y + (cy * al + d[k].y);
                    acc.z = acc.z + (cz * al + d[k].z);
                    acc.w = acc.w + 1.0f;
                }
        }
        accum[pl] = acc;
    }
}

void launch_resolve(const LaunchCfg& cfg, const Planes& planes, uint32_t n_slots, uint32_t Ppad, float4* accum, bool albedo_in_w,
                    float kd_untextured, bool code_in_color, bool sky_plane)
{
    uint32_t g = (Ppad + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    if (sky_plane)  // (the host's condition implies code_in_color)
        hipLaunchKernelGGL(k_resolve_coded_sky, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, planes, n_slots, Ppad, accum, kd_untextured);
    else if (code_in_color)
        hipLaunchKernelGGL(k_resolve_coded, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, planes, n_slots, Ppad, accum, kd_untextured);
    else if (albedo_in_w)
        hipLaunchKernelGGL(k_resolve<true>, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, planes, n_slots, Ppad, accum, kd_untextured);
    else
        hipLaunchKernelGGL(k_resolve<false>, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, planes, n_slots, Ppad, accum, kd_untextured);
}

// cap_debug_get(CAP_DEBUG_SKY_PLANE_NONZERO): the words of a sky plane that are not +0 (a -0 or a NaN counts: the head stores +0)
__global__ __launch_bounds__(kBlock) void k_sky_nonzero(const float* sky, size_t n, unsigned long long* out)
{
    unsigned long long m = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) m += f2u(sky[i]) != 0u ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) m += __shfl_down(m, off);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(out, m);
}

void launch_sky_nonzero(hipStream_t stream, const float* sky, size_t n, unsigned long long* out_device)
{
    if (!n) return;
    const size_t g = std::min<size_t>(4096, (n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_sky_nonzero, dim3((uint32_t)g), dim3(kBlock), 0, stream, sky, n, out_device);
}

__global__ __launch_bounds__(kBlock) void k_untile(ScreenDev sc, const float4* src, const float4* albedo, const float4* direct,
                                                   int kind, float4* image)
{
    const uint32_t n = sc.local_tiles * kTilePixels;
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < n; pl += gridDim.x * kBlock)
    {
        uint32_t x, y;
        if (!local_pixel_to_xy(sc, pl, x, y)) continue;
        float4 v = src[pl];
        if (kind == 1)
        {
            const float4 al = albedo[pl], d = direct[pl];
            // combine_illumination.hlsl:24,29 (indirect.w is forced to 1 before the multiply-add)
            v = make_float4(v.x * al.x + d.x, v.y * al.y + d.y, v.z * al.z + d.z, 1.0f * al.w + d.w);
        }
        else if (kind == 2)
        {
            v = make_float4(v.x / v.w, v.y / v.w, v.z / v.w, v.w);
        }
        image[(size_t)y * sc.width + x] = v;
    }
}

// four tile-ordered planes -> four row-major images in one pass (the reconstruction chain's inputs)
__global__ __launch_bounds__(kBlock) void k_untile4(ScreenDev sc, const float4* s0, const float4* s1, const float4* s2, const float4* s3,
                                                    float4* d0, float4* d1, float4* d2, float4* d3)
{
    const uint32_t n = sc.local_tiles * kTilePixels;
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < n; pl += gridDim.x * kBlock)
    {
        uint32_t x, y;
        if (!local_pixel_to_xy(sc, pl, x, y)) continue;
        const size_t o = (size_t)y * sc.width + x;
        if (s0) d0[o] = s0[pl];
        d1[o] = s1[pl], d2[o] = s2[pl], d3[o] = s3[pl];
    }
}

void launch_untile4(const LaunchCfg& cfg, const ScreenDev& screen, const float4* s0, const float4* s1, const float4* s2, const float4* s3,
                    float4* d0, float4* d1, float4* d2, float4* d3)
{
    uint32_t g = (screen.local_tiles * kTilePixels + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_untile4, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, screen, s0, s1, s2, s3, d0, d1, d2, d3);
}

void launch_untile(const LaunchCfg& cfg, const ScreenDev& screen, const float4* src, const float4* albedo, const float4* direct,
                   int plane_kind, float4* image)
{
    uint32_t g = (screen.local_tiles * kTilePixels + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_untile, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, screen, src, albedo, direct, plane_kind, image);
}

// row-major image -> this shard's tile-ordered buffer (the inverse of k_untile, kind 0); padding lanes and other shards' pixels: 0
__global__ __launch_bounds__(kBlock) void k_tile(ScreenDev sc, const float4* image, float4* dst)
{
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < sc.pixels_padded; pl += gridDim.x * kBlock)
    {
        uint32_t x, y;
        dst[pl] = local_pixel_to_xy(sc, pl, x, y) ? image[(size_t)y * sc.width + x] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

void launch_tile(const LaunchCfg& cfg, const ScreenDev& screen, const float4* image, float4* dst)
{
    uint32_t g = (screen.pixels_padded + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_tile, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, screen, image, dst);
}

__global__ __launch_bounds__(kBlock) void k_tiles_mean(const float4* accum, uint32_t Ppad, float4* dst)
{
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < Ppad; pl += gridDim.x * kBlock)
    {
        const float4 v = accum[pl];
        dst[pl] = v.w > 0.0f ? make_float4(v.x / v.w, v.y / v.w, v.z / v.w, v.w) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

void launch_tiles_mean(const LaunchCfg& cfg, const float4* accum, uint32_t Ppad, float4* dst)
{
    uint32_t g = (Ppad + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_tiles_mean, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, accum, Ppad, dst);
}

// gathered: [shard][shard_stride >= Ppad] tile-ordered pixels -> row-major image
__global__ __launch_bounds__(kBlock) void k_assemble(ScreenDev sc, const float4* gathered, uint32_t shard_count, size_t shard_stride, float4* image)
{
    const uint32_t total = sc.tile_count * kTilePixels;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock)
    {
        const uint32_t gt = i >> 6, w = i & 63u;
        const uint32_t shard = gt % shard_count, lt = gt / shard_count;
        const uint32_t ty = gt / sc.tiles_x, tx = gt - ty * sc.tiles_x;
        const uint32_t x = tx * kTileDim + (w & 7u), y = ty * kTileDim + (w >> 3);
        if (x < sc.width && y < sc.height)
            image[(size_t)y * sc.width + x] = gathered[(size_t)shard * shard_stride + lt * kTilePixels + w];
    }
}

void launch_assemble(const LaunchCfg& cfg, const ScreenDev& screen, const float4* gathered, uint32_t shard_count, float4* image,
                     size_t shard_stride)
{
    uint32_t g = (screen.tile_count * kTilePixels + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_assemble, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, screen, gathered, shard_count,
                       shard_stride ? shard_stride : (size_t)screen.pixels_padded, image);
}

// rt_primary_visibility.hlsl:46: (uv, asfloat(InstanceID), asfloat(PrimitiveIndex)); a miss keeps uv = 0, ids = ~0u (:41-43)
__global__ __launch_bounds__(kBlock) void k_geo_aov(SceneDev scene, const float4* hits, uint32_t Ppad, float4* out)
{
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < Ppad; pl += gridDim.x * kBlock)
    {
        const float4   h   = hits[pl];
        const uint32_t gid = f2u(h.z);
        if (gid == kInvalidId)
            out[pl] = make_float4(0.f, 0.f, u2f(kInvalidId), u2f(kInvalidId));
        else
        {
            const uint4 id = scene.tri_ids[gid];
            out[pl]        = make_float4(h.x, h.y, u2f(id.x), u2f(id.y));
        }
    }
}

void launch_geo_aov(const LaunchCfg& cfg, const SceneDev& scene, const float4* hits_slot, uint32_t Ppad, float4* aov_geo)
{
    uint32_t g = (Ppad + kBlock - 1) / kBlock;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_geo_aov, dim3(g ? g : 1), dim3(kBlock), 0, cfg.stream, scene, hits_slot, Ppad, aov_geo);
}
}  // namespace cap
