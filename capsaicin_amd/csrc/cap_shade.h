// cap_shade.h — what the three shading kernels share (k_shade and k_primary_shade in kernels.hip, k_trace_shade in
// small_scene.hip): sampling and textures, the queue appends, the per-vertex prefetch, and the shading bodies of the reference
// model (shade_vertex) and the EXT model (shade_vertex_ext).  Device code only.
#pragma once

#include "cap_exhaustive.h"
#include "cap_kernels.h"
#include "cap_reproject.h"
#include "cap_unscaled.h"

namespace cap
{
// ------------------------------------------------------------------------------------------------
// Shading
// ------------------------------------------------------------------------------------------------
// sampling.h:13-23 with the texel pre-divided by 255 on the host (identical fp32 quotient).
__device__ __forceinline__ void bluenoise4x4(const float2* tex, uint32_t x, uint32_t y, uint32_t count, float& s0, float& s1)
{
    const uint32_t px = (count % 16u) % 4u, py = (count % 16u) / 4u;
    const uint32_t sx = (x * 4u + px) % 256u, sy = (y * 4u + py) % 256u;
    const float2   t  = tex[sy * 256u + sx];
    const float    k  = 0.61803398875f * (float)(count / 16u);
    const float    a = t.x + k, b = t.y + k;
    s0 = a - floorf(a);
    s1 = b - floorf(b);
}

// sampling.h:91-111
// sampling.h:91-111.  The two branches do the same arithmetic on (n.z, n.y) or (n.y, n.x): selecting the operands first keeps
// the values bit for bit and spares a wave with both kinds of normals (any wave in a box scene) one sqrt and two divisions.
__device__ __forceinline__ v3 ortho_vector(v3 n)
{
    const bool  zn = fabsf(n.z) > 0.0f;
    const float a = zn ? n.z : n.y, b = zn ? n.y : n.x;
    const float k = sqrtf(fmaf(a, a, b * b));
    const float q1 = a / k, q2 = b / k;
    return zn ? mk3(0.0f, -q1, q2) : mk3(q1, -q2, 0.0f);
}

// sampling.h:113-132 with e = 1 (shading.h:26): pow(1 - r2, 1/2) == sqrt(1 - r2)
__device__ __forceinline__ v3 map_to_hemisphere(float r1, float r2, v3 n)
{
    v3       u = ortho_vector(n);
    const v3 v = cross3(u, n);
    u          = cross3(n, v);
    float sin_psi, cos_psi;
    sincos_c((2.0f * kPi) * r1, sin_psi, cos_psi);
    const float cos_theta = sqrtf(1.0f - r2);
    const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
    const float a = sin_theta * cos_psi, b = sin_theta * sin_psi;
    return normalize3(mk3(fmaf(n.x, cos_theta, fmaf(v.x, b, u.x * a)), fmaf(n.y, cos_theta, fmaf(v.y, b, u.y * a)),
                          fmaf(n.z, cos_theta, fmaf(v.z, b, u.z * a))));
}

// ---- the same shading arithmetic without the scaling steps of hipcc's sqrtf and `/` (cap_unscaled.h; the fused small-scene
// kernels of a scene with tame shading records, C::TAME).  Every form below gives the bits of the plain one on the
// range its operand is proven to lie in; cap_debug_get(CAP_DEBUG_SELFTEST_SHADE_UNARY / _DIV2) compares them on the device over
// exactly these ranges.  The proofs, operand by operand, are in DESIGN.md "fp32 arithmetic contract".
constexpr float kNormLo = 0.125f, kNormHi = 4.0f;  // |v|^2 of every vector normalize3_tame is given (tame records: [0.24, 2.01]; the sampled direction: 1 +- 1e-5)
__device__ __forceinline__ v3 normalize3_tame(v3 v)
{
    return v * div_unscaled(1.0f, sqrt_pos(dot3(v, v)));
}
// ortho_vector's operands (a, b, g = fmaf(a, a, b * b)) are inside the ranges of sqrt_pos and div2_unscaled: g in [2^-78, 2^80), so
// that k = sqrt(g) is in [2^-39, 2^40), and each of |a|, |b| zero or >= 2^-80 (both are <= k (1 + 2^-22) < 2^41).  A unit normal next
// to an axis fails it -- (1, 0, 1e-30): g underflows -- and so does one with a component below 2^-80 beside an ordinary one.
// Integer compares on the bit patterns: g >= +0 or NaN (above the upper bound), x - 1 wraps for a zero.
__device__ __forceinline__ bool ortho_in_range(float a, float b, float g)
{
    constexpr uint32_t kG0 = (127u - 78u) << 23, kG1 = (127u + 80u) << 23, kX0 = (127u - 80u) << 23;
    const uint32_t     xa = (f2u(a) & 0x7fffffffu) - 1u, xb = (f2u(b) & 0x7fffffffu) - 1u;
    return (f2u(g) - kG0 < kG1 - kG0) & ((xa < xb ? xa : xb) >= kX0 - 1u);
}
// The direction sample in two parts.  hemisphere_terms: what depends on the blue-noise pair alone -- the same for every vertex that
// draws (r1, r2), whatever it hit, which is what lets k_sample_terms (small_scene.hip) evaluate it once per (bounce, frame slot, position
// in the 64 x 64 blue-noise period) instead of once per vertex.  hemisphere_dir_tame: the tangent frame, the combination and the final
// normalize.  `terms` is a callable so that the per-vertex form evaluates it exactly where map_to_hemisphere_tame always has.
struct HemiTerms
{
    float ca, cb, cos_theta;  // sin_theta * cos_psi, sin_theta * sin_psi, cos_theta
};
__device__ __forceinline__ HemiTerms hemisphere_terms(float r1, float r2)
{
    float sin_psi, cos_psi;
    sincos_c((2.0f * kPi) * r1, sin_psi, cos_psi);
    // r2 = x - floorf(x) is in [0, 1 - 2^-24] (0 on lanes without a sample): 1 - r2 in [2^-24, 1].  cos_theta^2 rounds into [2^-24, 1],
    // so 1 - cos_theta^2 is 0 or in [2^-24, 1): the zero needs the fix-up
    const float cos_theta = sqrt_pos(1.0f - r2);
    const float sin_theta = sqrt_unscaled(1.0f - cos_theta * cos_theta);
    return HemiTerms{sin_theta * cos_psi, sin_theta * sin_psi, cos_theta};
}
template <class Terms>
__device__ __forceinline__ v3 hemisphere_dir_tame(v3 n, Terms terms)
{
    // ortho_vector under one wave-uniform guard: a wave with a lane outside it takes the plain forms for these three operations and
    // for the final normalize3 (whose operand is 1 +- 1e-5 only for a finite orthonormal frame)
    const bool  zn = fabsf(n.z) > 0.0f;
    const float a = zn ? n.z : n.y, b = zn ? n.y : n.x;
    const float g = fmaf(a, a, b * b);
#if defined(CAP_SHADE_ORTHO_PLAIN)  // A/B: ortho_vector and the final normalize3 as they were, no guard (capsaicin_amd/variants/orthoplain.flags)
    const bool fast = false;
#else
    const bool  fast = __ballot(!ortho_in_range(a, b, g)) == 0ull;
#endif
    float       q1, q2;
    if (fast)
        div2_unscaled(a, b, sqrt_pos(g), q1, q2);
    else
    {
        const float k = sqrtf(g);
        q1 = a / k, q2 = b / k;
    }
    v3       u = zn ? mk3(0.0f, -q1, q2) : mk3(q1, -q2, 0.0f);
    const v3 v = cross3(u, n);
    u          = cross3(n, v);
    const HemiTerms h = terms();
    const float     cos_theta = h.cos_theta, ca = h.ca, cb = h.cb;
    const v3    d = mk3(fmaf(n.x, cos_theta, fmaf(v.x, cb, u.x * ca)), fmaf(n.y, cos_theta, fmaf(v.y, cb, u.y * ca)),
                        fmaf(n.z, cos_theta, fmaf(v.z, cb, u.z * ca)));
    return fast ? normalize3_tame(d) : normalize3(d);
}
__device__ __forceinline__ v3 map_to_hemisphere_tame(float r1, float r2, v3 n)
{
    return hemisphere_dir_tame(n, [=] { return hemisphere_terms(r1, r2); });
}

// math_functions.h:36-47
__device__ __forceinline__ void oct_encode(v3 n, float& ox, float& oy)
{
    const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
    n             = mk3(n.x / s, n.y / s, n.z / s);
    ox = n.x, oy = n.y;
    if (!(n.z >= 0.0f))
    {
        ox = (1.0f - fabsf(n.y)) * (n.x >= 0.0f ? 1.0f : -1.0f);
        oy = (1.0f - fabsf(n.x)) * (n.y >= 0.0f ? 1.0f : -1.0f);
    }
    ox = ox * 0.5f + 0.5f;
    oy = oy * 0.5f + 0.5f;
}

__device__ __forceinline__ uint32_t wrap_texel(float f, uint32_t n)
{
    const float m = f - floorf(f / (float)n) * (float)n;
    int         i = (int)m;
    if (i < 0) i = 0;
    if ((uint32_t)i >= n) i = 0;
    return (uint32_t)i;
}

// SampleLevel(..., 0) bilinear + WRAP on RGBA8 (scene.h:57, raytracing_system.cpp:377)
__device__ __forceinline__ v3 sample_texture(const TextureDev& tex, float u, float v)
{
    const float    fx = fmaf(u, (float)tex.width, -0.5f), fy = fmaf(v, (float)tex.height, -0.5f);
    const float    x0f = floorf(fx), y0f = floorf(fy);
    const float    wx = fx - x0f, wy = fy - y0f;
    const uint32_t x0 = wrap_texel(x0f, tex.width), y0 = wrap_texel(y0f, tex.height);
    // One 16-byte load: a texture is stored as the bilinear footprint of every texel -- (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)
    // with WRAP applied, four RGBA8 words (cap_texture_upload).  Four scattered 4-byte loads per vertex were a quarter of the shade
    // stage's time on the textured scene (the stage is bound by the number of divergent addresses it sends);
    // the price is 4 x the texture memory.
    const uint4  fq   = reinterpret_cast<const uint4*>(tex.quads)[y0 * tex.width + x0];
    auto         rgba = [](uint32_t wd) { return make_uchar4((uint8_t)wd, (uint8_t)(wd >> 8), (uint8_t)(wd >> 16), (uint8_t)(wd >> 24)); };
    const uchar4 c00 = rgba(fq.x), c10 = rgba(fq.y), c01 = rgba(fq.z), c11 = rgba(fq.w);
    // byte / 255.0f without the division sequence: q = b * fl(1/255) is off by at most one ulp, and one residual step,
    // q + fl(b - 255 q) * fl(1/255), lands on the correctly rounded quotient for every one of the 256 bytes (checked exhaustively
    // in exact arithmetic: tests/test_oracle_kat.py::test_unorm8_is_the_division) -- 3 instructions instead of ~11
    auto unorm8 = [](uint8_t b) {
        const float r = 1.0f / 255.0f, fb = (float)b, q = fb * r;
        return fmaf(fmaf(-q, 255.0f, fb), r, q);
    };
    auto           lerp2 = [&](uint8_t a00, uint8_t a10, uint8_t a01, uint8_t a11) {
        const float f00 = unorm8(a00), f10 = unorm8(a10), f01 = unorm8(a01), f11 = unorm8(a11);
        const float top = fmaf(f10 - f00, wx, f00);
        const float bot = fmaf(f11 - f01, wx, f01);
        return fmaf(bot - top, wy, top);
    };
    return mk3(lerp2(c00.x, c10.x, c01.x, c11.x), lerp2(c00.y, c10.y, c01.y, c11.y), lerp2(c00.z, c10.z, c01.z, c11.z));
}

// Append one item per active lane to a device queue: one atomic per wave (64-lane ballot + popcount prefix).
__device__ __forceinline__ uint32_t wave_append(bool emit, uint32_t* counter)
{
    const unsigned long long mask = __ballot(emit);
    if (mask == 0ull) return 0;
    const uint32_t lane   = threadIdx.x & 63u;
    const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
    uint32_t       base   = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, (int)leader);
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// One path vertex: rt_direct_lighting.hlsl:38-83 (bounce 0) / one iteration of the rt_indirect.hlsl:91-174 loop, followed by
// the 64-lane compaction of the shadow ray and the extension ray into the class-`klass` sub-queues.  Called wave-uniformly
// (every lane of the wave, active or not) by the stand-alone shade kernel and by the fused trace+shade kernel.
//
// Everything the vertex needs that does not depend on the hit (pixel coordinates, the frame's light, the blue-noise sample) is
// fetched by shade_prefetch(); the fused kernel calls it BEFORE the triangle loop so that these dependent loads land under
// the loop's ALU work instead of in the latency-bound tail.
//
// C: what the calling kernel is, one type with constexpr bool members (kernels.hip ShadeStageCfg, small_scene.hip TraceShadeCfg):
//   FIRST    bounce 0: the vertex of a camera ray; it defines the planes' entries
//   EXT      the EXT shading model (shade_vertex_ext) instead of the reference's
//   FB       G-buffer feedback at bounce >= 1 (ShadeArgs::fb)
//   CARRY    extension-queue entries carry the blue-noise sample of the vertex they will find (see shade_prefetch)
//   SKY_RMW  the sky term goes to the plane by load-add-store instead of three float atomics (the stand-alone shade stage)
//   PROBE    the producer-side shadow probe and the per-wave ring (see ProbeArgs)
//   TAME     the scene's shading records are tame (SceneDev::shade_tame): square roots and divisions in their unscaled forms
//   LEAN     the lean per-chunk plumbing (see kChunkLean)
//   CODE     bounce 0 under ShadeArgs::code_in_color: the first vertex's code goes to color.w and the direct plane is not written
//   TAB      the direction sample's terms come from the batch's table (ShadeArgs::sample_terms) instead of being carried and computed
//   GRAY     the throughput is one float (C::Thr) and an extension entry two float4 (RayQueue, cap_device.h): an untextured scene, where
//            the three components are the same operations on the same operands at every bounce
//   SKYP     GRAY at bounce >= 1: the sky term is one store of the throughput into ShadeArgs::planes.sky, added by the resolve
// Text that serves both forms (small_scene_body.h) makes a throughput with thr_of<C::Thr>() -- the first of three equal components where
// it is one float -- and hands it to code written for three components through thr3().
template <class T>
__device__ __forceinline__ T thr_of(float x, float y, float z);
template <>
__device__ __forceinline__ v3 thr_of<v3>(float x, float y, float z) { return mk3(x, y, z); }
template <>
__device__ __forceinline__ float thr_of<float>(float x, float, float) { return x; }
__device__ __forceinline__ v3 thr3(v3 thr) { return thr; }
__device__ __forceinline__ v3 thr3(float thr) { return mk3(thr, thr, thr); }
struct ShadePre
{
    bool  valid;
    v3    L, I;    // lighting.h:20-33 of this path's frame
    float r1, r2;  // sampling.h:13-23 sample of (pixel, frame * 25 + bounce)
    float r3, r4, r5, r6;  // EXT only: B, A of the same texel; R, G of the texel of count + 7
    float r1n, r2n;        // CARRY only: the sample of the path's NEXT vertex (count + 1), handed on in the queue entry
                           // TAB: the sample itself is never fetched; (r1, r2, r1n) hold hemisphere_terms' (ca, cb, cos_theta) of it from the table
    bool  indirect_on;     // false for the three pixels of a 2x2 block that get no indirect sample this frame (LOWRES_INDIRECT)
};

// The per-frame constants of the batch (48 B x n_slots <= 3 KB) are staged in LDS once per workgroup: a path finds its frame's
// light and sample counter with a ~64-cycle ds_read instead of a global load that the blue-noise fetch would have to wait for.
__device__ __forceinline__ void stage_frames(const ShadeArgs& a, FrameConst* lds_frames)
{
    const uint32_t  words = a.n_slots * (uint32_t)(sizeof(FrameConst) / 4);
    const uint32_t* src   = reinterpret_cast<const uint32_t*>(a.frames);
    uint32_t*       dst   = reinterpret_cast<uint32_t*>(lds_frames);
    for (uint32_t i = threadIdx.x; i < words; i += kBlock) dst[i] = src[i];
    __syncthreads();
}

// Per-chunk plumbing of the fused small-scene kernels (LEAN: reference model, scene in LDS; docs/experiments.md (98)).  The vector
// instructions of a chunk that are neither the pair loop, phase 2, the shading arithmetic nor the probe were 15 % of the bounce >= 1
// kernel, and most of them produced what is the same for every path of a frame slot, the same at every bounce of a path, or never
// read.  -DCAP_CHUNK_PLAIN (capsaicin_amd/variants/chunkplain.flags) keeps the forms of round 8 for A/B runs.
#if defined(CAP_CHUNK_PLAIN)
constexpr bool kChunkLean = false;
#else
constexpr bool kChunkLean = true;
#endif

// A value nothing reads on the paths where it is not assigned: any register's content, no instruction (where `= 0` costs a v_mov per
// component and chunk).  Unspecified, not undefined: a lane may compute with it, as the probe does, as long as the result is discarded.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wuninitialized"
__device__ __forceinline__ float unread_f()
{
    float x;
    return x;
}
#pragma clang diagnostic pop
__device__ __forceinline__ v3 unread3() { return mk3(unread_f(), unread_f(), unread_f()); }

// What bluenoise4x4() makes of `count` alone: count = frame_count * 25 + bounce is the same for every path of a frame slot, so the
// workgroup computes it once per slot (the integer operations and the one fp32 multiply of bluenoise4x4, hence its bits) where it
// stages the frame constants, and a lane reads its slot's values instead of deriving them per vertex.
//  * count + 1 (CARRY: the sample of the path's next vertex, what every bounce needs) sits in the two pad words of the LDS copy of
//    FrameConst, next to the light it is read with: no LDS beyond the 3 KB that were there, one ds_read fewer per chunk.
//  * count itself is only needed where no sample is carried in, at bounce 0: a table of its own in that kernel.
struct SlotSample
{
    uint32_t off;  // (py << 8) | px: the texel inside the pixel's 4 x 4 block, as an address offset (<= 0x0303)
    float    k;    // 0.61803398875f * (float)(count / 16)
};
__device__ __forceinline__ uint32_t bluenoise_offset(uint32_t count) { return (((count % 16u) / 4u) << 8) | ((count % 16u) % 4u); }
__device__ __forceinline__ float    bluenoise_shift(uint32_t count) { return 0.61803398875f * (float)(count / 16u); }
// the pixel's part of the address: ((y * 4) % 256) * 256 + (x * 4) % 256.  px, py < 4 fill the two bits below each field, so
// bluenoise4x4's sy * 256 + sx is texel_base | offset.
__device__ __forceinline__ uint32_t bluenoise_base(uint32_t x, uint32_t y) { return ((y & 63u) << 10) | ((x & 63u) << 2); }
__device__ __forceinline__ void     bluenoise_at(const float2* tex, uint32_t base, uint32_t off, float k, float& s0, float& s1)
{
    const float2 t = tex[base | off];  // base <= 0xfcfc and off <= 0x0303 by construction (every staged row, also behind n_slots): inside the 256 x 256 texels whatever the path id holds
    const float  a = t.x + k, b = t.y + k;
    s0 = a - floorf(a);
    s1 = b - floorf(b);
}
// stage_frames() of the lean kernels.  All kMaxFrameSlots entries are defined (zeros behind n_slots), so that even a malformed path
// id finds an offset <= 0x0303 in its slot's row.
// TAB: no kernel reads a sample's constants (they went into the table, k_sample_terms): the rows are copied as they are.
template <bool FIRST, bool TAB = false>
__device__ __forceinline__ void stage_frames_samples(const ShadeArgs& a, FrameConst* lds_frames, SlotSample* lds_first)
{
    constexpr uint32_t kWords = (uint32_t)(sizeof(FrameConst) / 4);
    static_assert(kWords == 12 && offsetof(FrameConst, frame_count) == 8 && offsetof(FrameConst, pad1) == 28 && offsetof(FrameConst, pad2) == 44, "FrameConst layout");
    const uint32_t  words = (a.n_slots < kMaxFrameSlots ? a.n_slots : kMaxFrameSlots) * kWords;
    const uint32_t* src   = reinterpret_cast<const uint32_t*>(a.frames);
    uint32_t*       dst   = reinterpret_cast<uint32_t*>(lds_frames);
    for (uint32_t i = threadIdx.x; i < kMaxFrameSlots * kWords; i += kBlock)
    {
        uint32_t v = 0u;
        if (i < words)
        {
            const uint32_t sl = i / kWords, w = i - sl * kWords;
            v = src[i];
            if (!TAB && (w == 7u || w == 11u))
            {
                const uint32_t next = src[sl * kWords + 2u] * 25u + a.bounce + 1u;
                v = w == 7u ? bluenoise_offset(next) : f2u(bluenoise_shift(next));
            }
        }
        dst[i] = v;
    }
    if (FIRST && !TAB)
        for (uint32_t sl = threadIdx.x; sl < kMaxFrameSlots; sl += kBlock)
        {
            SlotSample ss = {0u, 0.0f};
            if (sl < a.n_slots)
            {
                const uint32_t count = a.frames[sl].frame_count * 25u + a.bounce;
                ss.off = bluenoise_offset(count), ss.k = bluenoise_shift(count);
            }
            lds_first[sl] = ss;
        }
    __syncthreads();
}

// CARRY (fused reference-model kernels): an extension ray's tmin / tmax are the constants kRayEps / kRayFar, so the two .w
// slots of its queue entry carry the blue-noise sample of the vertex it will find.  The vertex that emits the ray fetches
// that sample next to its other inputs, where nothing waits for it before the final stores; the vertex that receives it starts
// shading without a dependent global load.  carried_* = the .w slots of the entry this vertex came from (bounce >= 1).
// TAME: the last bounce emits no extension ray, so nothing reads the next vertex's sample
// LEAN (k_trace_shade; lds_first at bounce 0): the same values with less work per chunk.
//  * No defaults: on a lane without a vertex (valid == false) L, I and the samples are whatever the registers hold; shade_vertex reads
//    them on valid lanes only, and the probe's answer on the others is discarded.
//  * bounce >= 1: the only consumer of the pixel coordinates is the blue-noise address, i.e. x mod 64 and y mod 64, which come from
//    the tile's row and column mod 8 (tile_div: no run-time division).  The three bounds compares of local_pixel_to_xy are dropped:
//    the path was in bounds when bounce 0 emitted it, and for a malformed queue shade_vertex's own guard (slot >= n_slots ||
//    pl >= Ppad) is what keeps every plane index inside the planes -- plane_idx depends on slot and pl alone -- while the blue-noise
//    address is inside the texture for any path id (bluenoise_at).
//  * the sample constants of the slot come from where stage_frames_samples() put them.
template <class C>
__device__ __forceinline__ ShadePre shade_prefetch(const ShadeArgs& a, const FrameConst* lds_frames, bool active, uint32_t pid,
                                                   float carried_r1 = 0.f, float carried_r2 = 0.f, const SlotSample* lds_first = nullptr)
{
    ShadePre       s;
    const uint32_t slot = pid >> kPidShift, pl = pid & kPidMask;
    if constexpr (C::LEAN)
    {
        static_assert((C::CARRY != C::TAB) && !C::EXT, "LEAN: the reference model's fused kernels, the sample carried or from the table");
        const uint32_t    sl = slot < kMaxFrameSlots ? slot : 0;
        const FrameConst& fc = lds_frames[sl];
        uint32_t          base;  // TAB: the position in the 64 x 64 period, (y mod 64) << 6 | x mod 64, from the same bits
        s.indirect_on = true;
        if (C::FIRST)
        {
            uint32_t x = 0, y = 0;
            s.valid = active && local_pixel_to_xy(a.screen, pl, x, y);
            if (fc.lowres_sel & 4u) s.indirect_on = (x & 1u) == ((fc.lowres_sel >> 1) & 1u) && (y & 1u) == (fc.lowres_sel & 1u);
            base = C::TAB ? ((y & 63u) << 6) | (x & 63u) : bluenoise_base(x, y);
        }
        else
        {
            s.valid = active;
            const uint32_t gt = __umul24(pl >> 6, a.screen.shard_count) + a.screen.shard_index;  // 20-bit local tile, shard_count <= tile_count < 2^24
            const uint32_t ty = tile_div(gt, a.screen.tiles_x_mul, a.screen.tiles_x_shift);  // (a malformed gt >= 2^26: some other texel, discarded by the guard)
            // tx = gt - ty * tiles_x, of which only tx mod 8 is used: the low three bits of a product need those of its factors alone
            const uint32_t tx = gt + (ty & 7u) * ((0u - a.screen.tiles_x) & 7u);
            // x mod 64 = (tx mod 8) * 8 + (w & 7), y mod 64 = (ty mod 8) * 8 + (w >> 3) with w = pl & 63, placed as bluenoise_base() does
            base = C::TAB ? ((ty & 7u) << 9) | ((pl & 0x38u) << 3) | ((tx & 7u) << 3) | (pl & 7u)
                          : ((ty & 7u) << 13) | ((pl & 0x38u) << 7) | ((tx & 7u) << 5) | ((pl & 7u) << 2);
        }
        s.L = unread3(), s.I = unread3(), s.r1 = s.r2 = s.r1n = s.r2n = unread_f();
        s.r3 = s.r4 = s.r5 = s.r6 = 0.f;  // EXT only
        if (s.valid)
        {
            s.L = mk3(fc.light_dir[0], fc.light_dir[1], fc.light_dir[2]);
            s.I = mk3(fc.light_intensity[0], fc.light_intensity[1], fc.light_intensity[2]);
            if constexpr (C::TAB)
            {
                // one 16-byte load from this bounce's [slot][4096] block; every row below n_slots is defined, base < 4096 for any path id.
                // The last bounce samples nothing (TAME) and loads nothing
                if (a.bounce < a.num_bounces)
                {
                    const float4 q = a.sample_terms[((slot < a.n_slots ? slot : 0u) << 12) | base];
                    s.r1 = q.x, s.r2 = q.y, s.r1n = q.z;
                }
                return s;
            }
            if (C::FIRST)
            {
                const SlotSample ss = lds_first[sl];
                bluenoise_at(a.scene.bluenoise, base, ss.off, ss.k, s.r1, s.r2);  // rt_indirect.hlsl:149
            }
            else
                s.r1 = carried_r1, s.r2 = carried_r2;
            // the pad words of the LDS copy: the constants of count + 1 (stage_frames_samples)
            if (!C::TAME || a.bounce < a.num_bounces) bluenoise_at(a.scene.bluenoise, base, f2u(fc.pad1), fc.pad2, s.r1n, s.r2n);
        }
        return s;
    }
    uint32_t       x = 0, y = 0;
    s.valid = active && local_pixel_to_xy(a.screen, pl, x, y);
    s.L = mk3(0, 0, 0), s.I = mk3(0, 0, 0), s.r1 = 0.f, s.r2 = 0.f;
    s.r3 = s.r4 = s.r5 = s.r6 = 0.f;
    s.r1n = s.r2n = 0.f;
    s.indirect_on = true;
    if (s.valid)
    {
        const FrameConst fc = lds_frames[slot < kMaxFrameSlots ? slot : 0];
        if (fc.lowres_sel & 4u) s.indirect_on = (x & 1u) == ((fc.lowres_sel >> 1) & 1u) && (y & 1u) == (fc.lowres_sel & 1u);
        s.L = mk3(fc.light_dir[0], fc.light_dir[1], fc.light_dir[2]);
        s.I = mk3(fc.light_intensity[0], fc.light_intensity[1], fc.light_intensity[2]);
        const uint32_t count = fc.frame_count * 25u + a.bounce;
        if (C::CARRY && !C::FIRST)
            s.r1 = carried_r1, s.r2 = carried_r2;
        else
            bluenoise4x4(a.scene.bluenoise, x, y, count, s.r1, s.r2);  // rt_indirect.hlsl:149
        if (C::CARRY && (!C::TAME || a.bounce < a.num_bounces)) bluenoise4x4(a.scene.bluenoise, x, y, count + 1u, s.r1n, s.r2n);
        if (C::EXT)
        {
            bluenoise4x4(a.scene.bluenoise_ba, x, y, count, s.r3, s.r4);
            bluenoise4x4(a.scene.bluenoise, x, y, count + 7u, s.r5, s.r6);
        }
    }
    return s;
}

// Both queue appends of a wave with ONE device atomic: the extension and the shadow counter of a class sit in one 64-bit word
// (low half = extension entries, high half = shadow entries).
//
// Overflow guard (round 4).  A sub-queue's capacity is static because a path keeps the class it got at bounce 0 (cap_device.h); the
// appends used to rest on that argument alone, and anything that re-classifies paths -- the XCD-band experiment of round 3, any
// future sort -- would have written past the class's region, into its neighbour's entries or, for class 63, past the allocation.
// Now a lane whose slot lies beyond `capacity` does not store (emit_* comes back false for it), the wave that saw it bumps word 4
// of the guard block (CapStats::guard_append) and the consumers, which already clamp a class's count to its capacity, never read
// what was not written.  A run in which the guard fired has lost paths: bench.py and the tests treat it as a failure.
__device__ __forceinline__ void wave_append2(bool& emit_ext, bool& emit_shadow, uint32_t* counter_pair, uint32_t& ext_slot,
                                             uint32_t& shadow_slot, uint32_t capacity, uint64_t* guard)
{
    const unsigned long long me = __ballot(emit_ext), ms = __ballot(emit_shadow);
    ext_slot = shadow_slot = 0;
    if ((me | ms) == 0ull) return;
    const uint32_t lane   = threadIdx.x & 63u;
    const uint32_t leader = (uint32_t)__ffsll((long long)(me | ms)) - 1u;
    uint32_t       lo = 0, hi = 0;
    if (lane == leader)
    {
        const unsigned long long add = ((unsigned long long)__popcll(ms) << 32) | (unsigned long long)__popcll(me);
        const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(counter_pair), add);
        lo = (uint32_t)old, hi = (uint32_t)(old >> 32);
    }
    lo = __shfl(lo, (int)leader), hi = __shfl(hi, (int)leader);
    const unsigned long long below = (1ull << lane) - 1ull;
    ext_slot    = lo + (uint32_t)__popcll(me & below);
    shadow_slot = hi + (uint32_t)__popcll(ms & below);
    if (lo + (uint32_t)__popcll(me) > capacity || hi + (uint32_t)__popcll(ms) > capacity)  // wave-uniform, never true in a correct run
    {
        if (lane == leader)
        {
            atomicAdd((unsigned long long*)guard + 4, 1ull);
            guard[3] = ((uint64_t)lo << 32) | hi;
        }
        emit_ext    = emit_ext && ext_slot < capacity;
        emit_shadow = emit_shadow && shadow_slot < capacity;
    }
}

// Diagnostic build only (-DCAP_STAMPS): per-phase shader-clock sums of the fused kernel, see tools/stamps.py.
#ifdef CAP_STAMPS
static __device__ unsigned long long g_stamps[16];  // one per translation unit; only the fused kernel flushes, and cap_debug_stamps reads small_scene.hip's
struct Stamps
{
    unsigned long long last, acc[8], t_begin;
    __device__ void    start()
    {
        for (int i = 0; i < 8; ++i) acc[i] = 0;
        last    = __builtin_amdgcn_s_memtime();
        t_begin = __builtin_amdgcn_s_memrealtime();
    }
    __device__ void mark(int i, bool wait)
    {
#ifdef CAP_STAMPS_PHASES
        if (wait) __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0)
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[i] += now - last;
        last = now;
#endif
    }
    __device__ void flush()
    {
        if ((threadIdx.x & 63u) == 0)
            for (int i = 0; i < 8; ++i) atomicAdd(&g_stamps[i], acc[i]);
    }
};
#define STAMP(st, i, wait) (st).mark(i, wait)
#else
struct Stamps
{
    __device__ void start() {}
    __device__ void flush() {}
};
#define STAMP(st, i, wait) ((void)0)
#endif

// Probe (ShadeArgs::inline_probe, fused small-scene kernels): probe_rows = the PairPre rows of the probe pair per frame slot (two
// float4 each, LDS), probe_pairs = BvhDev::fan_pairs, probe_k the pair; n_probed counts the shadow rays the probe answered
// Ring (ShadeArgs::wave_ring): the survivors of the probe are not queued for another launch but parked in a ring of 128 entries
// that belongs to this wave alone (ring_org / ring_con: its slice of the shadow queue's memory); the kernel traces them 64 at a
// time itself (k_trace_shade trace_ring).  ring_head / ring_n are wave-uniform.
struct ProbeArgs
{
    const float4* rows  = nullptr;
    const float4* pairs = nullptr;
    uint32_t      k     = 0;
    float4*       ring_org = nullptr;
    float4*       ring_con = nullptr;
};
constexpr uint32_t kWaveRing = 128;  // <= 63 parked + <= 64 new
// TAME: the square roots and divisions of the vertex in their unscaled forms (map_to_hemisphere_tame and above), and nothing of the
// direction sample at the last bounce
// LEAN: p, dir and contrib exist only under the flag that stores them (emit_shadow: p, contrib; emit_ext: p, dir, thr); elsewhere they
// are whatever the registers hold.  The probe runs on all lanes and reads p: on a lane without a shadow ray its answer is discarded.
template <class C>
__device__ __forceinline__ void shade_vertex(const ShadeArgs& a, const float4* shade_tab, const ShadePre& pre, uint32_t klass,
                                             uint32_t pid, float4 hit, typename C::Thr thr, uint32_t& n_shaded, Stamps& st,
                                             const ProbeArgs probe = ProbeArgs(), uint32_t* n_probed = nullptr, uint32_t ring_head = 0,
                                             uint32_t* ring_n = nullptr)
{
    const uint32_t Ppad = a.screen.pixels_padded;
    const uint32_t slot = pid >> kPidShift, pl = pid & kPidMask;
    {
        const size_t plane_idx = (size_t)slot * Ppad + pl;
        bool         valid = pre.valid;
        if (valid && (slot >= a.n_slots || pl >= Ppad))
        {
            // never true for a well-formed queue; reported through CapStats::guard_* instead of faulting
            atomicAdd((unsigned long long*)a.shaded_counter + 1, 1ull);
            a.shaded_counter[3] = ((uint64_t)a.bounce << 32) | pid;
            valid = false;
        }
        const uint32_t gid = f2u(hit.z);

        bool   emit_shadow = false, emit_ext = false;
        v3     p = mk3(0, 0, 0), dir = mk3(0, 0, 0), contrib = mk3(0, 0, 0);
        if constexpr (C::LEAN) p = unread3(), dir = unread3(), contrib = unread3();

        if (C::FIRST && !valid)
        {
            // padding lane of a partial / absent tile: define the planes so the resolve adds exact zeros
            a.planes.color[plane_idx]  = make_float4(0, 0, 0, 0);  // CODE: code 0
            if (!C::CODE) a.planes.direct[plane_idx] = make_float4(0, 0, 0, 0);  // albedo_in_w: code 0
            if (!C::CODE && !a.albedo_in_w) a.planes.albedo[plane_idx] = make_float4(0, 0, 0, 0);
        }
        if (valid && gid == kInvalidId)
        {
            if (C::FIRST)
            {
                // rt_direct_lighting.hlsl:53-59, rt_indirect.hlsl:75-79
                a.planes.color[plane_idx]  = make_float4(0.f, 0.f, 0.f, 1.f);  // CODE: code 1, which is also what says (0.7, 0.7, 0.85)
                if (!C::CODE) a.planes.direct[plane_idx] = make_float4(0.7f, 0.7f, 0.85f, 1.f);  // albedo_in_w: code 1
                if (!C::CODE && !a.albedo_in_w) a.planes.albedo[plane_idx] = make_float4(1.f, 1.f, 1.f, 1.f);
                if (slot == a.aov_slot) a.planes.aov_normal_depth[pl] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            else
            {
                // rt_indirect.hlsl:94-99  color += throughput * sky.  Exactly one lane in the whole grid owns this path, so the
                // three no-return float atomics are plain IEEE adds in program order; unlike a load-add-store they do not make
                // the wave wait for the old value.
                // (A load-add-store here instead, as in k_trace_any: 16.4 -> 16.6 ms.)
                if constexpr (C::GRAY && C::SKYP)
                {
                    // The sky plane (TraceShadeCfg SKYP): the colour plane is not touched at all.  A path that escapes is finished --
                    // within this launch it has no vertex, hence no ring entry, and every earlier addition to its color.xyz was made
                    // by an earlier launch (in the head kernel: its bounce-0 ring entry writes `direct` and color.w only) -- so this
                    // term is the LAST addition its color.xyz would ever receive, and the whole term is one float.  The lane stores
                    // thr and k_resolve_coded_sky (planes.hip), which holds the path's colour entry in a register anyway, computes
                    // color.x + thr * 0.7f, color.y + thr * 0.7f, color.z + thr * 0.85f: the atomics' IEEE additions, on the same
                    // operands, after the same earlier ones.  (-ffp-contract=off, csrc/Makefile, keeps products and sums apart there
                    // as here.)  Every other path's entry holds the head's +0, and x + (+0) == x in every bit unless x is -0, which
                    // color.xyz never is: it starts at +0 (the head's store) and only receives contributions c * thr with
                    // c = ((I * kd) * kInvPi) * fmaxf(0, n.L) of a positive light and a kd >= 1e-5 (a smaller one is `black` and adds
                    // nothing) and thr a product of such kd and of quotients of fmaxf(., 0) terms: sums of non-negative numbers.  A NaN
                    // thr gives the NaN the atomic would have given: the same product enters the same addition.
                    a.planes.sky[plane_idx] = thr;
                }
                else if constexpr (C::GRAY)
                {
                    // thr.x * 0.7f and thr.y * 0.7f are one product
                    float*      c  = reinterpret_cast<float*>(a.planes.color + plane_idx);
                    const float t7 = thr * 0.7f;
                    atomicAdd(c + 0, t7);
                    atomicAdd(c + 1, t7);
                    atomicAdd(c + 2, thr * 0.85f);
                }
                else if (C::SKY_RMW)
                {
                    // the tree path's shade stage: three scattered float atomics per escaping ray are three 64-B memory-side
                    // requests each; the path is this entry's only writer within the launch, so a 16-B load-add-store gives the
                    // same IEEE additions
                    const float4 cur = a.planes.color[plane_idx];
                    a.planes.color[plane_idx] = make_float4(cur.x + thr.x * 0.7f, cur.y + thr.y * 0.7f, cur.z + thr.z * 0.85f, cur.w);
                }
                else
                {
                    float* c = reinterpret_cast<float*>(a.planes.color + plane_idx);
                    atomicAdd(c + 0, thr.x * 0.7f);
                    atomicAdd(c + 1, thr.y * 0.7f);
                    atomicAdd(c + 2, thr.z * 0.85f);
                }
            }
        }
        else if (valid)
        {
            ++n_shaded;
            // scene.h:5-50 InterpolateAttributes on the pre-gathered triangle record
            const float4* tab = shade_tab + kShadeRec * (size_t)gid;
            const float4  s0 = tab[0], s1 = tab[1], s2 = tab[2], s3 = tab[3], s4 = tab[4], s5 = tab[5];
            const float   u = hit.x, v = hit.y, w = (1.0f - u) - v;
            auto          mix = [&](float c0, float c1, float c2) { return fmaf(c2, v, fmaf(c1, u, c0 * w)); };
            const v3      nm = mk3(mix(s3.x, s4.x, s5.x), mix(s3.y, s4.y, s5.y), mix(s3.z, s4.z, s5.z));
            const v3      n  = C::TAME ? normalize3_tame(nm) : normalize3(nm);  // tame records: |nm|^2 in [0.24, 2.01] (bvh.hip k_tri_setup)
            p = mk3(mix(s0.x, s1.x, s2.x), mix(s0.y, s1.y, s2.y), mix(s0.z, s1.z, s2.z));
            // scene.h:52-61 GetMaterial
            v3       kd   = mk3(a.scene.kd_untextured, a.scene.kd_untextured, a.scene.kd_untextured);
            uint32_t inst = 0;
            if (a.scene.texture_count != 0 || (C::FIRST && slot == a.aov_slot))  // wave-uniform: untextured scenes skip the dependent load
            {
                const float4 idf   = tab[6];  // (instance, primitive, mesh_texture[instance]) in the record itself: no second fetch
                inst               = f2u(idf.x);
                const uint32_t tex = f2u(idf.z);
                if (tex != kInvalidId && tex < a.scene.texture_count)
                {
                    const float tu = mix(s0.w, s2.w, s4.w), tv = mix(s1.w, s3.w, s5.w);
                    const v3    c  = sample_texture(a.scene.textures[tex], tu, 1.0f - tv);
                    kd             = mk3(pow22_c(c.x), pow22_c(c.y), pow22_c(c.z));
                }
            }
            const bool black = kd.x < 1e-5f && kd.y < 1e-5f && kd.z < 1e-5f;  // rt_direct_lighting.hlsl:68, rt_indirect.hlsl:108
            if (C::FIRST)
            {
                // albedo_in_w (untextured scene, accumulate-only render): the albedo is one of four constants, so its plane is
                // neither written nor read; direct.w carries which -- 0: (0,0,0) padding, 1: (1,1,1) sky, 2: the untextured kd, 3: black
                // CODE: color.w carries it and `direct` is not written here -- all it would say is "nothing yet".  The word is safe
                // there: the load-add-stores of the later bounces carry cur.w through and the sky term's atomics touch x, y, z only.
                if (C::CODE)
                    a.planes.color[plane_idx] = make_float4(0.f, 0.f, 0.f, black ? kCodeBlack : kCodeKd);  // (the shadow entry below repeats it)
                else
                {
                    a.planes.color[plane_idx]  = make_float4(0.f, 0.f, 0.f, 1.f);
                    a.planes.direct[plane_idx] = make_float4(0.f, 0.f, 0.f, a.albedo_in_w ? (black ? kCodeBlack : kCodeKd) : 1.f);
                }
                if (!C::CODE && !a.albedo_in_w) a.planes.albedo[plane_idx] = black ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(kd.x, kd.y, kd.z, 1.f);
                if (slot == a.aov_slot)
                {
                    float4 nd = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (!black)
                    {
                        oct_encode(n, nd.x, nd.y);
                        nd.z = (float)inst;
                        nd.w = length3(mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]) - p);
                    }
                    a.planes.aov_normal_depth[pl] = nd;
                }
            }
            bool reused = false;
            if (C::FB && !C::FIRST && !black)
            {
                // rt_indirect.hlsl:116-145 GBUFFER_FEEDBACK: a vertex the previous frame saw (inside its image, depth within 5 %)
                // takes that frame's shaded, TAA'd colour and ends the path.  A NaN uv counts as disocclusion (stated choice:
                // HLSL's any(uv < 0) || any(uv > 1) would let it through to an undefined texel address).
                const uint32_t W = a.screen.width, H = a.screen.height;
                const f2       puv = image_plane_uv(a.fb.prev_cam, p);
                if (puv.x >= 0.0f && puv.y >= 0.0f && puv.x <= 1.0f && puv.y <= 1.0f)
                {
                    const f2    pxy        = uv_to_xy(puv, W, H);
                    const float prev_depth = ldi(Img{a.fb.prev_normal_depth, W, H}, (int)pxy.x, (int)pxy.y).w;
                    const float cur_depth =
                        length3(p - mk3(a.fb.prev_cam.position[0], a.fb.prev_cam.position[1], a.fb.prev_cam.position[2]));
                    if (!(fabsf(prev_depth - cur_depth) / cur_depth > 0.05f))
                    {
                        reused        = true;
                        const v3 hc   = sample_bilinear(Img{a.fb.color_history, W, H}, puv);
                        // the path is this entry's only writer within the launch (it either escapes or is shaded), and bounce 0 defined the
                        // entry one launch ago: a 16-B load-add-store makes the same IEEE additions as three float atomics.  Unlike the sky
                        // term above, where the atomics win by 1 %, here most vertices of a frame take this branch -- the previous frame saw
                        // them -- and 6 M atomics per launch cost more than the load's latency: real-time frame 0.648 -> 0.638 ms.
                        const float4 cur = a.planes.color[plane_idx];
                        const v3     th  = thr3(thr);  // (no feedback kernel is GRAY)
                        a.planes.color[plane_idx] = make_float4(cur.x + th.x * hc.x, cur.y + th.y * hc.y, cur.z + th.z * hc.z, cur.w);
                    }
                }
            }
            if (!black && !reused)
            {
                // lighting.h:35-61: unshadowed direct term; the visibility ray is queued for the any-hit kernel
                const float ndl = fmaxf(0.0f, dot3(n, pre.L));
                v3          c   = mk3(((pre.I.x * kd.x) * kInvPi) * ndl, ((pre.I.y * kd.y) * kInvPi) * ndl, ((pre.I.z * kd.z) * kInvPi) * ndl);
                if (c.x != 0.0f || c.y != 0.0f || c.z != 0.0f)
                {
                    emit_shadow = true;
                    if constexpr (C::GRAY)
                        contrib = C::FIRST ? c : c * thr;
                    else
                        contrib = C::FIRST ? c : thr * c;  // rt_direct_lighting.hlsl:77 / rt_indirect.hlsl:136
                }
                // rt_indirect.hlsl:149-170
                // the reference traces one more ray after the last bounce whose payload is never read (:91,:173): at that bounce
                // (launch-uniform) no extension ray is emitted.  TAME: the sampled direction, its pdf and the throughput feed nothing
                // else there and are not computed
                const bool more = a.bounce < a.num_bounces;
                if (!C::TAME || more)
                {
                    if constexpr (C::TAB)
                        dir = hemisphere_dir_tame(n, [&] { return HemiTerms{pre.r1, pre.r2, pre.r1n}; });
                    else
                        dir = C::TAME ? map_to_hemisphere_tame(pre.r1, pre.r2, n) : map_to_hemisphere(pre.r1, pre.r2, n);
                    const float ndd = dot3(n, dir);
                    // TAME: n and dir are unit vectors (or dir is NaN: numerator 0), so the numerator is 0 or in (0, 1.01].  From 2^-80 on
                    // the quotient has the bits of the plain one; below, it is some finite value < 2^-78, which `pdf < 1e-5f` rejects like
                    // the plain quotient.  Past that test the numerator of f is >= 0.99e-5 and its denominator >= 1e-5.
                    const float pdf = C::TAME ? div_unscaled(fmaxf(0.0f, ndd), kPi) : fmaxf(0.0f, ndd) / kPi;  // shading.h:19-22
                    if (!(pdf < 1e-5f))
                    {
                        const float fn = kInvPi * fmaxf(ndd, 0.0f);
                        const float f  = C::TAME ? div_unscaled(fn, pdf) : fn / pdf;
                        thr            = thr * f;
                        if constexpr (C::GRAY)
                        {
                            if (!C::FIRST) thr = thr * kd.x;  // kd = (k, k, k): the condition of the form
                        }
                        else if (!C::FIRST)
                            thr = thr * kd;
                        emit_ext = more && (!C::FIRST || pre.indirect_on);
                    }
                }
            }
        }

        if (C::PROBE)
        {
            if (probe.rows != nullptr)  // wave-uniform
            {
                // lanes without a shadow ray test an empty interval's worth of nothing: their result is discarded
                const Ray    sr  = make_ray(p, pre.L, kRayEps, kRayFar);
                const uint32_t ps = valid ? slot : 0u;
                const float4   pa = probe.rows[2u * ps], pb = probe.rows[2u * ps + 1u];
                const bool   occluded = pair_occludes_pre(sr, probe.pairs, probe.k, pa, pb);
                if (emit_shadow && occluded) emit_shadow = false, ++*n_probed;
            }
        }
        // a.shadow.count == a.out.count + 1: both counters of a class share one 64-bit word (one atomic per wave for both queues)
        uint32_t ei, si;
        STAMP(st, 2, true);  // shading inputs arrived + shading ALU
        wave_append2(emit_ext, emit_shadow, a.out.count + klass * kCounterStride, ei, si, a.out.class_capacity, a.shaded_counter);
        STAMP(st, 3, true);  // append atomic returned
        ei += klass * a.out.class_capacity;
        si += klass * a.shadow.class_capacity;
        if (C::PROBE && probe.ring_org != nullptr)  // wave-uniform
        {
            // the entry goes to this wave's own ring (the counter above still counted it: CapStats::shadow_entries)
            const unsigned long long ms = __ballot(emit_shadow);
            if (emit_shadow)
            {
                const uint32_t lane_ = threadIdx.x & 63u;
                const uint32_t pos   = (ring_head + *ring_n + (uint32_t)__popcll(ms & ((1ull << lane_) - 1ull))) & (kWaveRing - 1u);
                probe.ring_org[pos]  = make_float4(p.x, p.y, p.z, u2f(pid));
                probe.ring_con[pos]  = make_float4(contrib.x, contrib.y, contrib.z, 0.0f);
            }
            *ring_n += (uint32_t)__popcll(ms);
            // the entries are read by OTHER lanes of this wave (trace_ring): wavefront-scope release here, acquire there.  No code on
            // gfx950 (same-wave LDS and vector-memory operations retire in issue order), but it is what forbids the compiler to move
            // the stores below the loads -- ordering that until round 3 rested on a scheduling barrier alone.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
        else if (emit_shadow)
        {
            // reference model: the shadow ray's direction is its frame's light and tmin / tmax are constants (lighting.h:39-47), so
            // the entry is 32 B -- (origin, path id) and the contribution; the any-hit kernel looks the direction up by frame slot
            // CODE: the spare word is the path's code for the any-hit kernel, which rewrites color.w without loading it.  It must be
            // the word stored into color.w above, `black ? kCodeBlack : kCodeKd`: emit_shadow is only ever set under !black, so that
            // is kCodeKd here.  A code that depends on more than `black` has to be carried to this store as a value.
            a.shadow.org_tmin[si]    = make_float4(p.x, p.y, p.z, u2f(pid));
            a.shadow.contrib_pid[si] = make_float4(contrib.x, contrib.y, contrib.z, C::CODE ? kCodeKd : 0.0f);
        }
        if constexpr (C::GRAY)
        {
            if (emit_ext)
            {
                a.out.org_tmin[ei] = make_float4(p.x, p.y, p.z, thr);
                a.out.dir_tmax[ei] = make_float4(dir.x, dir.y, dir.z, u2f(pid));
            }
        }
        else if (emit_ext)
        {
            a.out.org_tmin[ei] = make_float4(p.x, p.y, p.z, C::CARRY ? pre.r1n : kRayEps);
            a.out.dir_tmax[ei] = make_float4(dir.x, dir.y, dir.z, C::CARRY ? pre.r2n : kRayFar);
            a.out.thr_pid[ei]  = make_float4(thr.x, thr.y, thr.z, u2f(pid));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// EXT shading model (no reference counterpart, specification in DESIGN.md "EXT shading model"):
// Lambert + GGX microfacet BSDF, emissive triangles sampled by area with one shadow ray per vertex (next-event estimation),
// emission seen directly only from the camera, black environment.  Same queues and kernels as the reference model.
// ------------------------------------------------------------------------------------------------
struct ExtBsdf
{
    v3    f;
    float pdf_spec, pdf_diff;
};

__device__ __forceinline__ float lum3(v3 c) { return fmaf(c.z, 0.114f, fmaf(c.y, 0.587f, c.x * 0.299f)); }

// What the BSDF needs of the vertex and the outgoing direction alone: both evaluations of a vertex (towards the light sample and
// along the sampled direction) share them, so they are computed once -- the same expressions on the same operands as before.
struct ExtView
{
    float cos_o, lam_o;  // lam_o = cos_o + sqrt(a2 + (1 - a2) cos_o^2): the outgoing direction's factor of the masking term
};
__device__ __forceinline__ ExtView ext_view(float a2, v3 nf, v3 wo)
{
    ExtView w;
    w.cos_o = dot3(nf, wo);
    w.lam_o = w.cos_o + sqrtf(fmaf(1.0f - a2, w.cos_o * w.cos_o, a2));
    return w;
}
__device__ __forceinline__ ExtBsdf ext_bsdf(v3 kd, v3 ks, float a2, v3 nf, v3 wo, v3 wi, const ExtView& vw)
{
    const float cos_i = dot3(nf, wi);
    const v3    h     = normalize3(wo + wi);
    const float cos_h = dot3(nf, h), woh = dot3(wo, h);
    const float dd    = fmaf(cos_h * cos_h, a2 - 1.0f, 1.0f);
    // D G / (4 cos_o cos_i) in its cancelled ("visibility") form, one division: see oracle/cap_oracle.cpp ext_bsdf (the same operations)
    const float pdd   = kPi * dd * dd;
    const float lam_i = cos_i + sqrtf(fmaf(1.0f - a2, cos_i * cos_i, a2));
#if defined(CAP_EXT_DIAG) && CAP_EXT_DIAG == 3  // diagnostic build: no microfacet term (D, G and their divisions fall away)
    const float spec  = 0.0f * (vw.cos_o + woh);
#else
    const float spec  = a2 / (pdd * (vw.lam_o * lam_i));
#endif
    ExtBsdf     r;
    r.f        = mk3(kd.x * kInvPi + ks.x * spec, kd.y * kInvPi + ks.y * spec, kd.z * kInvPi + ks.z * spec);
    r.pdf_spec = (a2 * cos_h) / (pdd * (4.0f * woh));
    r.pdf_diff = cos_i * kInvPi;
    return r;
}

// Tables of the EXT model in LDS (fused small-scene kernels, scenes of at most kExhaustiveMax triangles): the per-mesh materials,
// the light table and, per emissive triangle, its three vertices, unit normal and emission -- what shade_vertex_ext otherwise
// fetches through four dependent global loads and recomputes per vertex (the normal: a cross product and a normalisation that
// depend on the light triangle alone).  Same operations on the same operands, done once per workgroup.
struct ExtTables
{
    const MaterialDev* materials  = nullptr;  // [mesh]
    const float*       light_cdf  = nullptr;
    const float4*      light_rec  = nullptr;  // 4 per light: (q0, ke.x) (q1, ke.y) (q2, ke.z) (nl, -)
};
constexpr uint32_t kExtLightsMax = 32;  // lights the LDS table holds (more: the global path)

// INLINE (ShadeArgs::inline_nee, fused small-scene kernels only): bvh is traced for the shadow ray here; acc = what the path has
// gathered so far
template <bool FIRST, bool INLINE = false>
__device__ __forceinline__ void shade_vertex_ext(const ShadeArgs& a, const float4* shade_tab, const ShadePre& pre, uint32_t klass,
                                                 uint32_t pid, float4 hit, v3 thr,
                                                 v3 d, uint32_t& n_shaded, const BvhDev* bvh = nullptr, v3 acc = mk3(0.f, 0.f, 0.f),
                                                 const ExtTables tabs = ExtTables())
{
    const uint32_t Ppad = a.screen.pixels_padded;
    const uint32_t slot = pid >> kPidShift, pl = pid & kPidMask;
    const size_t   plane_idx = (size_t)slot * Ppad + pl;
    bool           valid = pre.valid;
    if (valid && (slot >= a.n_slots || pl >= Ppad))
    {
        atomicAdd((unsigned long long*)a.shaded_counter + 1, 1ull);
        a.shaded_counter[3] = ((uint64_t)a.bounce << 32) | pid;
        valid = false;
    }
    const uint32_t gid = f2u(hit.z);
    bool  emit_shadow = false, emit_ext = false;
    v3    p = mk3(0, 0, 0), dir = mk3(0, 0, 0), contrib = mk3(0, 0, 0), sdir = mk3(0, 0, 1), first_ke = mk3(0, 0, 0);
    float stmax = 0.0f;

    if (FIRST && !valid)
    {
        a.planes.color[plane_idx]  = make_float4(0, 0, 0, 0);
        a.planes.direct[plane_idx] = make_float4(0, 0, 0, 0);
        if (!a.albedo_in_w) a.planes.albedo[plane_idx] = make_float4(0, 0, 0, 0);
    }
    if (valid && gid == kInvalidId)
    {
        if (FIRST)
        {
            // black environment: the camera ray that leaves the scene carries nothing
            a.planes.color[plane_idx]  = make_float4(0.f, 0.f, 0.f, 1.f);
            a.planes.direct[plane_idx] = make_float4(0.f, 0.f, 0.f, 1.f);
            if (!a.albedo_in_w) a.planes.albedo[plane_idx] = make_float4(1.f, 1.f, 1.f, 1.f);  // else: direct.w == 1 says so
            if (slot == a.aov_slot) a.planes.aov_normal_depth[pl] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    else if (valid)
    {
        ++n_shaded;
        const float4* st = shade_tab + kShadeRec * (size_t)gid;
        const float4  s0 = st[0], s1 = st[1], s2 = st[2], s3 = st[3], s4 = st[4], s5 = st[5];
        const float   u = hit.x, v = hit.y, w = (1.0f - u) - v;
        auto          mix = [&](float c0, float c1, float c2) { return fmaf(c2, v, fmaf(c1, u, c0 * w)); };
        const v3      n = normalize3(mk3(mix(s3.x, s4.x, s5.x), mix(s3.y, s4.y, s5.y), mix(s3.z, s4.z, s5.z)));
        p = mk3(mix(s0.x, s1.x, s2.x), mix(s0.y, s1.y, s2.y), mix(s0.z, s1.z, s2.z));
        const uint32_t    inst = f2u(st[6].x);
        const MaterialDev m    = tabs.materials ? tabs.materials[inst] : a.scene.materials[inst];
        const v3    kd = mk3(m.kd[0], m.kd[1], m.kd[2]), ks = mk3(m.ks[0], m.ks[1], m.ks[2]), ke = mk3(m.ke[0], m.ke[1], m.ke[2]);
        const float alpha = fmaxf(m.roughness * m.roughness, 1e-3f), a2 = alpha * alpha;
        const v3    wo = mk3(-d.x, -d.y, -d.z);
        const v3    nf = dot3(n, wo) < 0.0f ? mk3(-n.x, -n.y, -n.z) : n;
        const ExtView vw = ext_view(a2, nf, wo);
        if (FIRST)
        {
            first_ke = ke;
            if (!INLINE)  // (INLINE: both written below, once the shadow ray is known / the path ends)
            {
                a.planes.color[plane_idx]  = make_float4(0.f, 0.f, 0.f, 1.f);
                a.planes.direct[plane_idx] = make_float4(ke.x, ke.y, ke.z, 1.f);
            }
            if (!a.albedo_in_w) a.planes.albedo[plane_idx] = make_float4(1.f, 1.f, 1.f, 1.f);  // this model folds kd into the throughput
            if (slot == a.aov_slot)
            {
                float4 nd;
                oct_encode(n, nd.x, nd.y);
                nd.z = (float)inst;
                nd.w = length3(mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]) - p);
                a.planes.aov_normal_depth[pl] = nd;
            }
        }
        // ---- next-event estimation: one point on the emissive triangles, uniform by area ----
#if defined(CAP_EXT_DIAG) && CAP_EXT_DIAG == 2  // diagnostic build: no next-event estimation at all
        if (false)
#else
        if (a.scene.light_count != 0)
#endif
        {
            const float target = pre.r4 * a.scene.light_area;
            const float* cdf   = tabs.light_cdf ? tabs.light_cdf : a.scene.light_cdf;
            uint32_t    lo = 0, hi = a.scene.light_count - 1;
            while (lo < hi)  // first entry whose prefix sum exceeds target, else the last
            {
                const uint32_t mid = (lo + hi) >> 1;
                if (cdf[mid] > target) hi = mid; else lo = mid + 1;
            }
            v3 q0, q1, q2, nl, lke;
            if (tabs.light_rec)  // wave-uniform
            {
                const float4 r0 = tabs.light_rec[4 * lo], r1 = tabs.light_rec[4 * lo + 1], r2 = tabs.light_rec[4 * lo + 2], r3 = tabs.light_rec[4 * lo + 3];
                q0 = mk3(r0.x, r0.y, r0.z), q1 = mk3(r1.x, r1.y, r1.z), q2 = mk3(r2.x, r2.y, r2.z), nl = mk3(r3.x, r3.y, r3.z);
                lke = mk3(r0.w, r1.w, r2.w);
            }
            else
            {
                const uint32_t lg = a.scene.light_tris[lo];
                const float4*  lt = shade_tab + kShadeRec * (size_t)lg;
                const float4   l0 = lt[0], l1 = lt[1], l2 = lt[2];
                q0 = mk3(l0.x, l0.y, l0.z), q1 = mk3(l1.x, l1.y, l1.z), q2 = mk3(l2.x, l2.y, l2.z);
                nl = normalize3(cross3(q1 - q0, q2 - q0));
                const MaterialDev lm = a.scene.materials[f2u(lt[6].x)];
                lke = mk3(lm.ke[0], lm.ke[1], lm.ke[2]);
            }
            const float    su = sqrtf(pre.r5), b0 = 1.0f - su, b1 = su * (1.0f - pre.r6), b2 = su * pre.r6;
            const v3 lp = mk3(fmaf(q2.x, b2, fmaf(q1.x, b1, q0.x * b0)), fmaf(q2.y, b2, fmaf(q1.y, b1, q0.y * b0)),
                              fmaf(q2.z, b2, fmaf(q1.z, b1, q0.z * b0)));
            const v3    Lv = lp - p;
            const float d2 = dot3(Lv, Lv), dist = sqrtf(d2);
            const v3    wi = Lv * (1.0f / dist);
            const float cos_s = dot3(nf, wi), cos_l = fabsf(dot3(nl, wi));
            if (cos_s > 0.0f && cos_l > 0.0f && d2 > 0.0f)
            {
                const ExtBsdf     bs  = ext_bsdf(kd, ks, a2, nf, wo, wi, vw);
                const float       wgt = ((cos_s * cos_l) * a.scene.light_area) / d2;
                const v3 c = mk3((thr.x * bs.f.x) * (lke.x * wgt), (thr.y * bs.f.y) * (lke.y * wgt), (thr.z * bs.f.z) * (lke.z * wgt));
                if (c.x != 0.0f || c.y != 0.0f || c.z != 0.0f)
                {
                    emit_shadow = true, contrib = c, sdir = wi, stmax = dist * 0.999f;
                }
            }
        }
        // ---- BSDF sampling: GGX half vector or cosine hemisphere, chosen by luminance ----
        const float ls = lum3(ks), sum = lum3(kd) + ls;
        if (sum > 0.0f)
        {
            const float ps = ls / sum;
            // The two lobes sample a polar angle -- GGX: cos^2 = (1 - r2) / (1 + (a2 - 1) r2) for the half vector, Lambert:
            // cos = sqrt(1 - r2) for the direction (MapToHemisphere, sampling.h:113-132, e = 1) -- around the SAME frame with
            // the SAME azimuth; a wave whose lanes chose different lobes (any wave: the choice is a random number per lane) used
            // to run the frame, the sincos and the normalisation twice.  One copy now, the polar angle selected per lane: the
            // same operations on the same operands for either lobe, so the same bits.
            const bool  lobe_spec = pre.r3 < ps;
            const float c2  = (1.0f - pre.r2) / fmaf(a2 - 1.0f, pre.r2, 1.0f);
            const float ctd = sqrtf(1.0f - pre.r2);
            const float ct  = lobe_spec ? sqrtf(c2) : ctd;
            const float stt = lobe_spec ? sqrtf(fmaxf(0.0f, 1.0f - c2)) : sqrtf(1.0f - ctd * ctd);
            float       sp, cp;
            sincos_c((2.0f * kPi) * pre.r1, sp, cp);
            v3       uu = ortho_vector(nf);
            const v3 vv = cross3(uu, nf);
            uu          = cross3(nf, vv);
            const float ca = stt * cp, cb = stt * sp;
            const v3    hh = normalize3(mk3(fmaf(nf.x, ct, fmaf(vv.x, cb, uu.x * ca)), fmaf(nf.y, ct, fmaf(vv.y, cb, uu.y * ca)),
                                            fmaf(nf.z, ct, fmaf(vv.z, cb, uu.z * ca))));
            const float k2 = 2.0f * dot3(wo, hh);
            const v3    wi = lobe_spec ? mk3(fmaf(hh.x, k2, -wo.x), fmaf(hh.y, k2, -wo.y), fmaf(hh.z, k2, -wo.z)) : hh;
            const float cos_i = dot3(nf, wi);
            if (cos_i > 0.0f)
            {
                const ExtBsdf bs  = ext_bsdf(kd, ks, a2, nf, wo, wi, vw);
                const float   pdf = ps * bs.pdf_spec + (1.0f - ps) * bs.pdf_diff;
                if (pdf > 1e-8f)
                {
                    const float wgt = cos_i / pdf;
                    thr      = mk3(thr.x * (bs.f.x * wgt), thr.y * (bs.f.y * wgt), thr.z * (bs.f.z * wgt));
                    dir      = wi;
                    emit_ext = a.bounce < a.num_bounces;
                }
            }
        }
    }
    uint32_t ei, si;
    wave_append2(emit_ext, emit_shadow, a.out.count + klass * kCounterStride, ei, si, a.out.class_capacity, a.shaded_counter);  // (INLINE: the shadow counter still counts the rays)
    ei += klass * a.out.class_capacity;
    si += klass * a.shadow.class_capacity;
    if (INLINE)
    {
        // the any-hit kernel's test and its addition, here: lanes without a shadow ray trace an empty interval
        const Ray  sr      = make_ray(p, sdir, kRayEps, emit_shadow ? stmax : kRayEps);
        bool       visible = false;
#if defined(CAP_EXT_DIAG) && CAP_EXT_DIAG == 1  // diagnostic build (wrong images, right timing): what the inline any-test costs
        visible = emit_shadow;
#else
#if defined(CAP_NEE_CHECK)  // diagnostic build: both lists, every disagreement counted (CapStats::guard_shade stays 0 when the rule holds)
        if (__ballot(emit_shadow) != 0ull)
        {
            const bool full = exhaustive_any<false>(*bvh, sr), part = exhaustive_any<false, true>(*bvh, sr);
            if (emit_shadow && full != part) atomicAdd((unsigned long long*)a.shaded_counter + 1, 1ull);
            visible = emit_shadow && !part;
        }
#else
        if (__ballot(emit_shadow) != 0ull) visible = emit_shadow && !exhaustive_any<false, true>(*bvh, sr);  // (a wave without a shadow ray: no test)
#endif
#endif
        const bool on_surface = valid && gid != kInvalidId;
        if (FIRST)
        {
            if (on_surface)
                a.planes.direct[plane_idx] = visible ? make_float4(first_ke.x + contrib.x, first_ke.y + contrib.y, first_ke.z + contrib.z, 1.f)
                                                     : make_float4(first_ke.x, first_ke.y, first_ke.z, 1.f);
        }
        else if (visible)
            acc = mk3(acc.x + contrib.x, acc.y + contrib.y, acc.z + contrib.z);
        // the path ends here unless it continues: its colour-plane entry is written exactly once (a camera ray that left the scene
        // wrote it above)
        if (valid && !emit_ext && (!FIRST || on_surface)) a.planes.color[plane_idx] = make_float4(acc.x, acc.y, acc.z, 1.f);
        if (emit_ext) a.out.acc[ei] = make_float4(acc.x, acc.y, acc.z, 0.f);
    }
    else if (emit_shadow)
    {
        a.shadow.org_tmin[si]    = make_float4(p.x, p.y, p.z, kRayEps);
        a.shadow.dir_tmax[si]    = make_float4(sdir.x, sdir.y, sdir.z, stmax);
        a.shadow.contrib_pid[si] = make_float4(contrib.x, contrib.y, contrib.z, u2f(pid));
    }
    if (emit_ext)
    {
        a.out.org_tmin[ei] = make_float4(p.x, p.y, p.z, kRayEps);
        a.out.dir_tmax[ei] = make_float4(dir.x, dir.y, dir.z, kRayFar);
        a.out.thr_pid[ei]  = make_float4(thr.x, thr.y, thr.z, u2f(pid));
    }
}

// Statistics of a launch: shaded vertices and (small-scene path) the shadow rays the producer's probe answered -- ONE 64-bit atomic
// per wave into words 2 (probed) and 3 (shaded) of the counter line of the wave's queue class, whose words 0 and 1 are the
// bounce's extension / shadow queue lengths (context.hip reads all four from the batch's counter copy).
// Until round 3 every wave of the grid added to ONE word at the end of every launch (and a second one for the probe count): a
// device-scope atomic on one address retires ~88 per microsecond (MI355X_MICROARCH.md "dequeue"), so the 6144 waves of a launch
// with little work -- which all finish together -- queued for 70 us behind each other: the whole "fixed cost" of the persistent
// launches that round 2's batch-size sweep measured (tools/tiny_trace.sh: 77 us per fused launch whatever its work, 6 us for
// the any-hit kernel, which has no such flush), and 17 % of a rank's step at eight shards.
__device__ __forceinline__ void flush_stats(uint32_t* class_line, uint32_t n_shaded, uint32_t n_probed = 0)
{
    for (int off = 32; off > 0; off >>= 1) n_shaded += __shfl_down(n_shaded, off), n_probed += __shfl_down(n_probed, off);
    if ((threadIdx.x & 63u) == 0 && (n_shaded | n_probed))
        atomicAdd(reinterpret_cast<unsigned long long*>(class_line + 2), ((unsigned long long)n_shaded << 32) | (unsigned long long)n_probed);
}
}  // namespace cap
