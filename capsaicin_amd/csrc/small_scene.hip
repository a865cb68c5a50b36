// small_scene.hip — the fused stage of the small-scene path (scenes traced exhaustively, cap_exhaustive.h): k_trace_shade, its
// launcher, the per-phase clocks of the diagnostic build and the device self-test of the unscaled shading forms.
#include "cap_shade.h"

#include <algorithm>
#include <cassert>
#include <type_traits>

namespace cap
{
// Fused stage of the small-scene path: closest-hit (exhaustive, wave-uniform) + shading of the vertex it finds, in one pass over
// the ray queue.  The hit record never travels through HBM and the shading stage's memory latency hides under the ALU-bound
// triangle loop of the other waves.  FIRST generates the camera ray instead of reading a queue entry (rt_primary_visibility).
#ifndef CAP_TS_FIRST
#define CAP_TS_FIRST 5  // workgroups per CU the bounce-0 kernel is register-allocated for
#endif
#ifndef CAP_TS_EXT
#define CAP_TS_EXT 6  // ... and the EXT model's bounce >= 1 kernel
#endif
#ifndef CAP_TS_NEXT
#define CAP_TS_NEXT 6  // ... and the bounce >= 1 kernel (8 fits in 64 VGPRs without spills but measured 8 % slower)
#endif
#ifdef CAP_STAMPS
__device__ unsigned long long g_wave_times[2 * 16384];  // (start, end) s_memrealtime of every wave of the LAST fused launch
#endif
// What one instantiation of k_trace_shade is: everything the kernel derives from its five template arguments, derived once.
// shade_prefetch() and shade_vertex() read the same type (cap_shade.h, C).
// LDS: scenes of at most kExhaustiveMax triangles keep their shading records (96 B each) and intersection records in LDS
// (<= 10 KB per workgroup), so the gathers by hit triangle after the loop are ds_reads instead of a global round trip.
// TAME: the scene's shading records are tame (SceneDev::shade_tame, established where they are written), which is what lets the
// vertex's normalize3 -- and with it everything downstream of a unit normal -- take the unscaled forms.  Chosen at launch like LDS;
// only the reference model's kernels with the scene in LDS have the instantiation.
// CODE: ShadeArgs::code_in_color, bounce 0's form without the direct plane.  Only the TAME kernel has it (trace_shade_has_code_form).
// TAB: the terms of a vertex's direction sample come from the batch's table (ShadeArgs::sample_terms, k_sample_terms below) and no
// queue entry carries a sample.  Only the lean kernels have the form (trace_shade_has_table_form).
// HEAD: the batch's first bounce >= 1 launch with bounce 0 inside it (ShadeArgs::in re-used for the camera table, see k_camera_vertices
// below): the queue is bounce 0's identity queue, a chunk starts with the per-slot remainder of bounce 0 on its table entry and keeps the
// ray that makes in registers.  Only the TAB bounce >= 1 kernel has the form (k_trace_shade_head).
// GRAY: the extension queue's 32-byte entries (RayQueue, cap_device.h) and the throughput as one float, for a scene without textures.  A
// FIRST kernel writes them, the bounce >= 1 kernel reads and writes them, the HEAD kernel writes them.  Only the TAB kernels have the form
// (k_trace_shade_tab_gray, k_trace_shade_head_gray), beside their 48-byte forms: trace_shade_has_gray_form.
// SKYP: the sky term of an escaping path goes to ShadeArgs::planes.sky as one plain store instead of three float atomics on the colour
// plane, and the resolve adds it (shade_vertex's escape branch has the argument).  The head zeroes the plane next to its store of the
// code.  Only the GRAY bounce >= 1 kernel and the GRAY head have the form (k_trace_shade_tab_gray_sky, k_trace_shade_head_gray_sky).
template <bool FIRST_, bool EXT_, bool FB_, bool LDS_, bool TAME_, bool CODE_ = false, bool TAB_ = false, bool HEAD_ = false, bool GRAY_ = false,
          bool SKYP_ = false>
struct TraceShadeCfg
{
    // (TAB_ = kChunkLean in k_trace_shade_tab: a build without the lean plumbing compiles the plain kernel under that name, never launched)
    static_assert(!TAME_ || (!EXT_ && !FB_ && LDS_), "TAME: reference model, scene in LDS");
    static_assert(!CODE_ || (FIRST_ && TAME_), "CODE: bounce 0 of the reference model, scene in LDS, tame records");
    static_assert(!TAB_ || (TAME_ && kChunkLean), "TAB: the lean kernels (reference model, scene in LDS, tame records)");
    static_assert(!HEAD_ || (TAB_ && !FIRST_), "HEAD: the lean bounce >= 1 kernel with the sample table");
    static_assert(!GRAY_ || TAB_, "GRAY: the lean kernels with the sample table");
    static_assert(!SKYP_ || (GRAY_ && !FIRST_), "SKYP: the 32-byte bounce >= 1 kernel and its head form");
    static constexpr bool FIRST = FIRST_, EXT = EXT_, FB = FB_, LDS = LDS_, TAME = TAME_, CODE = CODE_, TAB = TAB_, HEAD = HEAD_, GRAY = GRAY_;
    static constexpr bool SKYP = SKYP_;
    using Thr = typename std::conditional<GRAY_, float, v3>::type;  // a path's throughput
    static constexpr bool CARRY = !EXT && !TAB, SKY_RMW = false;
    static constexpr bool PROBE = !EXT && !FB && LDS;  // the producer-side shadow probe (ShadeArgs::inline_probe) and the per-wave ring
    // the lean per-chunk plumbing (see kChunkLean): the reference model's kernels with the scene in LDS and tame records.  (The
    // instantiations without TAME pay for it with 8 and 4 B of scratch, the EXT and feedback kernels were not tried: they keep round 8's.)
    static constexpr bool LEAN = PROBE && TAME && kChunkLean;
    static constexpr bool ORG  = FIRST && LDS;  // camera rays of a small scene: per-pair origin terms and screen bounds (stage_camera_pairs)
    static constexpr bool XT   = EXT && LDS;    // EXT model: materials, light table and per-light records (stage_ext_tables)
    static constexpr int  kBlocksPerCu = FB ? 4 : (EXT ? (FIRST ? 5 : CAP_TS_EXT) : (FIRST ? CAP_TS_FIRST : CAP_TS_NEXT));  // launch bounds
};

// ---- the kernel's prologue: what a workgroup stages in LDS once, block by block.  Each function fills the arrays it is given; the
// barrier between them and the chunk loop is stage_frames' (stage_probe_rows has two of its own).
// LDS: the scene's shading and intersection records
__device__ __forceinline__ void stage_scene_records(const BvhDev& bvh, const ShadeArgs& a, float4* lds_shade, float4* lds_rec)
{
    const uint32_t n = bvh.tri_count <= kExhaustiveMax ? bvh.tri_count : kExhaustiveMax;
    for (uint32_t k = threadIdx.x; k < kShadeRec * n; k += kBlock) lds_shade[k] = a.scene.shade_tris[k];
    for (uint32_t k = threadIdx.x; k < 4 * n; k += kBlock) lds_rec[k] = bvh.tris_by_id[k];
}
// XT: the tables of ExtTables, when they fit
__device__ __forceinline__ void stage_ext_tables(const ShadeArgs& a, float* lds_mat, float* lds_lcdf, float4* lds_lrec)
{
    const float* ms = reinterpret_cast<const float*>(a.scene.materials);
    for (uint32_t k = threadIdx.x; k < 12u * a.scene.material_count; k += kBlock) lds_mat[k] = ms[k];
    for (uint32_t k = threadIdx.x; k < a.scene.light_count; k += kBlock)
    {
        lds_lcdf[k] = a.scene.light_cdf[k];
        const float4* lt = a.scene.shade_tris + kShadeRec * (size_t)a.scene.light_tris[k];
        const float4  l0 = lt[0], l1 = lt[1], l2 = lt[2];
        const v3      q0 = mk3(l0.x, l0.y, l0.z), q1 = mk3(l1.x, l1.y, l1.z), q2 = mk3(l2.x, l2.y, l2.z);
        const v3      nl = normalize3(cross3(q1 - q0, q2 - q0));  // as shade_vertex_ext computes it per vertex without the table
        const MaterialDev lm = a.scene.materials[f2u(lt[6].x)];
        lds_lrec[4 * k]     = make_float4(q0.x, q0.y, q0.z, lm.ke[0]);
        lds_lrec[4 * k + 1] = make_float4(q1.x, q1.y, q1.z, lm.ke[1]);
        lds_lrec[4 * k + 2] = make_float4(q2.x, q2.y, q2.z, lm.ke[2]);
        lds_lrec[4 * k + 3] = make_float4(nl.x, nl.y, nl.z, 0.f);
    }
}
// ORG: per fan pair, the origin terms of pair_scaled<ORG> (lds_org) and its pixel bounds (x0, y0, x1, y1) as the launch's camera
// sees it, grown by two pixels (the sub-pixel jitter of the frames and the rounding of the projection); a pair with a vertex at or
// behind the camera plane covers the screen.  A tile of camera rays only tests the pairs whose bounds overlap it: a ray can only hit
// a quad through a sample point inside the quad's projection, so the pairs left out are missed by all 64 rays -- same hits, same bits.
__device__ __forceinline__ void stage_camera_pairs(const BvhDev& bvh, const ShadeArgs& a, float4* lds_org, float4* lds_bounds)
{
    const v3     o  = mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]);
    const float* fp = reinterpret_cast<const float*>(bvh.fan_pairs);
    for (uint32_t k = threadIdx.x; k < bvh.fan_pair_count && 2 * k + 1 < kExhaustiveMax; k += kBlock)
    {
        const float* rec  = fp + 20 * (size_t)k;  // (v0, e1, e2, e3, nA, nB, id, 0)
        const v3     tvec = o - mk3(rec[0], rec[1], rec[2]);
        lds_org[2 * k]     = make_float4(tvec.x, tvec.y, tvec.z, dot3(tvec, mk3(rec[12], rec[13], rec[14])));
        lds_org[2 * k + 1] = make_float4(dot3(tvec, mk3(rec[15], rec[16], rec[17])), 0.f, 0.f, 0.f);
        // screen bounds: pixel = ((f * (d.right) / (d.forward)) / sensor + 0.5) * extent  (inverse of primary_dir, camera.h:39-63)
        const v3 R = mk3(a.cam.right[0], a.cam.right[1], a.cam.right[2]), U = mk3(a.cam.up[0], a.cam.up[1], a.cam.up[2]),
                 F = mk3(a.cam.forward[0], a.cam.forward[1], a.cam.forward[2]);
        float x0 = 3.0e38f, y0 = 3.0e38f, x1 = -3.0e38f, y1 = -3.0e38f;
        bool  behind = false;
        for (int e = 0; e < 4; ++e)
        {
            const v3    d = e == 0 ? tvec * -1.0f : (mk3(rec[3 * e], rec[3 * e + 1], rec[3 * e + 2]) - tvec);  // vertex - camera
            const float z = dot3(d, F);
            behind |= !(z > 1e-4f);
            const float px = ((a.cam.focal_length * dot3(d, R) / z) / a.cam.sensor_x + 0.5f) * (float)a.screen.width;
            const float py = ((a.cam.focal_length * dot3(d, U) / z) / a.cam.sensor_y + 0.5f) * (float)a.screen.height;
            x0 = fminf(x0, px), x1 = fmaxf(x1, px), y0 = fminf(y0, py), y1 = fmaxf(y1, py);
        }
        const bool usable = a.cull_camera_pairs != 0u && !behind && x0 == x0 && y0 == y0 && x1 == x1 && y1 == y1;
        lds_bounds[k] = usable ? make_float4(x0 - kCameraCullPad, y0 - kCameraCullPad, x1 + kCameraCullPad, y1 + kCameraCullPad) : make_float4(-3.0e38f, -3.0e38f, 3.0e38f, 3.0e38f);
    }
}
// PROBE: the pair whose four vertices reach farthest along the batch's first light direction (k_trace_any_small's first probe) into
// probe_k, and its PairPre rows per frame slot into lds_probe
__device__ __forceinline__ void stage_probe_rows(const BvhDev& bvh, const ShadeArgs& a, float* lds_pscore, uint32_t& probe_k, float4* lds_probe)
{
    const uint32_t np = bvh.fan_pair_count;  // 1 .. kExhaustiveMax / 2, checked by the host
    const float*   fp = reinterpret_cast<const float*>(bvh.fan_pairs);
    if (threadIdx.x < np)
    {
        const float* rec = fp + 20 * (size_t)threadIdx.x;
        const v3     L   = mk3(a.frames[0].light_dir[0], a.frames[0].light_dir[1], a.frames[0].light_dir[2]);
        const v3     v0  = mk3(rec[0], rec[1], rec[2]);
        float        sc  = dot3(v0, L);
        for (int e = 0; e < 3; ++e) sc += dot3(v0 + mk3(rec[3 + 3 * e], rec[4 + 3 * e], rec[5 + 3 * e]), L);
        lds_pscore[threadIdx.x] = sc;
    }
    __syncthreads();
    if (threadIdx.x < np)
    {
        const float sc   = lds_pscore[threadIdx.x];
        uint32_t    rank = 0;
        for (uint32_t j = 0; j < np; ++j)
        {
            const float o = lds_pscore[j];
            rank += (o > sc || (o == sc && j < threadIdx.x)) ? 1u : 0u;
        }
        if (rank == 0) probe_k = threadIdx.x;
    }
    __syncthreads();
    const float* rec = fp + 20 * (size_t)probe_k;
    for (uint32_t sl = threadIdx.x; sl < a.n_slots && sl < kMaxFrameSlots; sl += kBlock)
    {
        const v3 d = mk3(a.frames[sl].light_dir[0], a.frames[sl].light_dir[1], a.frames[sl].light_dir[2]);
        lds_probe[2 * sl]     = tri_pre(d, mk3(rec[12], rec[13], rec[14]), kRayEps, kRayFar);
        lds_probe[2 * sl + 1] = tri_pre(d, mk3(rec[15], rec[16], rec[17]), kRayEps, kRayFar);
    }
}

// All seven kernels are small_scene_body.h and nothing else: k_trace_shade the thirteen forms without the sample table, under the names
// and with the instructions they have always had, k_trace_shade_tab the three with it, k_trace_shade_head (below) bounce 1 with bounce 0
// at the head of its chunks, k_trace_shade_tab_gray and k_trace_shade_head_gray those four with 32-byte queue entries,
// k_trace_shade_tab_gray_sky and k_trace_shade_head_gray_sky the two of those that run at bounce >= 1 with the sky plane.
template <bool FIRST, bool EXT, bool FB = false, bool LDS = false, bool TAME = false, bool CODE = false>
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<FIRST, EXT, FB, LDS, TAME, CODE>::kBlocksPerCu)) void k_trace_shade(BvhDev bvh, ShadeArgs a)
{
    using C            = TraceShadeCfg<FIRST, EXT, FB, LDS, TAME, CODE>;
    constexpr bool TAB = false;
#include "small_scene_body.h"
}
// TAB: reference model, scene in LDS, tame records, the lean plumbing; bounce 0 with and without CODE, and bounce >= 1
template <bool FIRST, bool CODE>
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<FIRST, false, false, true, true, CODE, kChunkLean>::kBlocksPerCu)) void k_trace_shade_tab(BvhDev bvh, ShadeArgs a)
{
    using C            = TraceShadeCfg<FIRST, false, false, true, true, CODE, kChunkLean>;
    constexpr bool EXT = false, FB = false, LDS = true, TAB = kChunkLean;
#include "small_scene_body.h"
}

// HEAD: bounce 1 of a batch with bounce 0 as the head of every chunk (TraceShadeCfg)
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<false, false, false, true, true, false, kChunkLean, kChunkLean>::kBlocksPerCu)) void k_trace_shade_head(BvhDev bvh, ShadeArgs a)
{
    using C              = TraceShadeCfg<false, false, false, true, true, false, kChunkLean, kChunkLean>;
    constexpr bool FIRST = false, EXT = false, FB = false, LDS = true, TAB = kChunkLean;
#include "small_scene_body.h"
}

// GRAY: the three table kernels and the head with 32-byte entries, beside their 48-byte forms -- which keep their names and their
// instructions, so that the switch CAP_NO_GRAY_ENTRIES stands for the commit before these in a measurement
template <bool FIRST, bool CODE>
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<FIRST, false, false, true, true, CODE, kChunkLean, false, kChunkLean>::kBlocksPerCu)) void k_trace_shade_tab_gray(BvhDev bvh, ShadeArgs a)
{
    using C            = TraceShadeCfg<FIRST, false, false, true, true, CODE, kChunkLean, false, kChunkLean>;
    constexpr bool EXT = false, FB = false, LDS = true, TAB = kChunkLean;
#include "small_scene_body.h"
}
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<false, false, false, true, true, false, kChunkLean, kChunkLean, kChunkLean>::kBlocksPerCu)) void k_trace_shade_head_gray(BvhDev bvh, ShadeArgs a)
{
    using C              = TraceShadeCfg<false, false, false, true, true, false, kChunkLean, kChunkLean, kChunkLean>;
    constexpr bool FIRST = false, EXT = false, FB = false, LDS = true, TAB = kChunkLean;
#include "small_scene_body.h"
}

// SKYP: the 32-byte bounce >= 1 kernel and the 32-byte head with the sky plane, beside the two above -- which keep their names and their
// instructions, so that the switch CAP_NO_SKY_PLANE stands for the commit before these in a measurement
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<false, false, false, true, true, false, kChunkLean, false, kChunkLean, kChunkLean>::kBlocksPerCu)) void k_trace_shade_tab_gray_sky(BvhDev bvh, ShadeArgs a)
{
    using C              = TraceShadeCfg<false, false, false, true, true, false, kChunkLean, false, kChunkLean, kChunkLean>;
    constexpr bool FIRST = false, EXT = false, FB = false, LDS = true, TAB = kChunkLean;
#include "small_scene_body.h"
}
__global__ __launch_bounds__(kBlock, (TraceShadeCfg<false, false, false, true, true, false, kChunkLean, kChunkLean, kChunkLean, kChunkLean>::kBlocksPerCu)) void k_trace_shade_head_gray_sky(BvhDev bvh, ShadeArgs a)
{
    using C              = TraceShadeCfg<false, false, false, true, true, false, kChunkLean, kChunkLean, kChunkLean, kChunkLean>;
    constexpr bool FIRST = false, EXT = false, FB = false, LDS = true, TAB = kChunkLean;
#include "small_scene_body.h"
}

#ifdef CAP_STAMPS
extern "C" int cap_debug_stamps(unsigned long long* out, int reset)
{
    if (reset == 2) return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), 2 * 16384 * sizeof(unsigned long long));
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), 8 * sizeof(unsigned long long));
    if (e == hipSuccess && reset)
    {
        unsigned long long z[16] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
    }
    return (int)e;
}
#endif

// cap_debug_get(CAP_DEBUG_SELFTEST_SHADE_UNARY / _DIV2): the unscaled forms of the small-scene shading against the plain sqrtf and `/`
// compiled in the same kernel, bit for bit, over every float of the range each is used on (out[0]: mismatches, out[1]: comparisons made).
//   which 0: sqrt_pos and sqrt_unscaled over every normal x >= 2^-96 (both), sqrt_unscaled at +0, -0 and +inf;
//            1 / sqrt(x) as normalize3_tame computes it over every x in [kNormLo, kNormHi];
//            x / kPi over x = 0 and every x in [2^-80, 2]; over every 0 < x < 2^-80, denormals included, the unscaled quotient must be
//            finite and below 1e-5 (what `pdf < 1e-5f` needs of it);
//            f = (kInvPi x) / (x / kPi) over every x in [0, 2] whose pdf passes !(pdf < 1e-5f).
//   which 1: ortho_vector's sqrt and two quotients over 2^31 pseudo-random (a, b), signs, zeros and -0 included, of which those inside the
//            guard (ortho_in_range, the kernel's own) are compared: the host asks for >= 2^30.
__device__ __forceinline__ uint32_t selftest_hash32(uint32_t x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
__global__ __launch_bounds__(kBlock) void k_shade_forms_selftest(unsigned long long* out, uint32_t which)
{
    const uint32_t     tid = blockIdx.x * kBlock + threadIdx.x, total = gridDim.x * kBlock;
    unsigned long long bad = 0, n = 0;
    auto               differ = [](float x, float y) { return f2u(x) != f2u(y) ? 1u : 0u; };
    if (which == 0)
    {
        for (uint64_t b = ((127ull - 96ull) << 23) + tid; b <= 0x7f7fffffull; b += total)
        {
            const float x = u2f((uint32_t)b), s = sqrtf(x);
            bad += differ(sqrt_pos(x), s) + differ(sqrt_unscaled(x), s), n += 2;
        }
        if (tid < 3)
        {
            const float x = tid == 0 ? 0.0f : (tid == 1 ? -0.0f : __builtin_inff());
            bad += differ(sqrt_unscaled(x), sqrtf(x)), ++n;
        }
        for (uint64_t b = (uint64_t)f2u(kNormLo) + tid; b <= f2u(kNormHi); b += total)
        {
            const float x = u2f((uint32_t)b);
            bad += differ(div_unscaled(1.0f, sqrt_pos(x)), 1.0f / sqrtf(x)), ++n;
        }
        for (uint64_t b = tid; b <= f2u(2.0f); b += total)
        {
            const float x = u2f((uint32_t)b), pdf = x / kPi, fast = div_unscaled(x, kPi);
            if (b == 0 || b >= ((127ull - 80ull) << 23))
                bad += differ(fast, pdf);
            else
                bad += (fast < 1e-5f && fast > -1e-5f) ? 0u : 1u;  // (false for NaN and inf)
            ++n;
            if (!(pdf < 1e-5f)) bad += differ(div_unscaled(kInvPi * fmaxf(x, 0.0f), pdf), (kInvPi * fmaxf(x, 0.0f)) / pdf), ++n;
        }
    }
    else
    {
        for (uint64_t i = tid; i < (1ull << 31); i += total)
        {
            const uint32_t h0 = selftest_hash32((uint32_t)i), h1 = selftest_hash32((uint32_t)i ^ 0x9e3779b9u), h2 = selftest_hash32(h0 + h1);
            // exponent fields: the larger operand 2^-45 .. 2^44, the other 0 .. 95 binades below it (both ends beyond the guard)
            const uint32_t e1 = 82u + h2 % 90u, d = (h2 >> 8) % 96u, e0 = e1 > d ? e1 - d : 1u;
            float          p = u2f((e1 << 23) | (h0 & 0x007fffffu) | ((h2 << 3) & 0x80000000u));
            float          q = u2f((e0 << 23) | (h1 & 0x007fffffu) | ((h2 << 2) & 0x80000000u));
            if ((h2 >> 24 & 7u) == 0u) q = (h2 & 0x08000000u) ? 0.0f : -0.0f;
            const bool  sw = (h2 >> 27 & 1u) != 0u;
            const float a = sw ? q : p, b = sw ? p : q, g = fmaf(a, a, b * b);
            if (!ortho_in_range(a, b, g)) continue;
            const float k = sqrtf(g), kf = sqrt_pos(g);
            float       qa, qb;
            div2_unscaled(a, b, kf, qa, qb);
            bad += differ(kf, k) + differ(qa, a / k) + differ(qb, b / k), ++n;
        }
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicAdd(&out[1], n);
}

void launch_shade_forms_selftest(hipStream_t stream, unsigned long long* out_device, uint32_t which)
{
    hipLaunchKernelGGL(k_shade_forms_selftest, dim3(4096), dim3(kBlock), 0, stream, out_device, which);
}

// ---- the table of direction-sample terms (ShadeArgs::sample_terms, the TAB kernels).  A vertex's sample (r1, r2) is the blue-noise
// texel of (pixel mod 64, count = frame_count * 25 + bounce) and what shading makes of it first -- hemisphere_terms: sincos, two square
// roots -- depends on nothing else: 4 096 distinct results per (bounce, frame slot) where a batch shades up to a few hundred vertices per
// entry.  One thread per (sampling bounce b < num_bounces, slot s, yy, xx); entry [b][s][(yy << 6) | xx] = (ca, cb, cos_theta, 0).  The texel,
// the shift and the terms by the functions the kernels without the table run on the same operands: the same bits.
__global__ __launch_bounds__(kBlock) void k_sample_terms(const float2* bluenoise, const FrameConst* frames, uint32_t n_slots, uint32_t num_bounces, float4* table)
{
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, row = tid >> 12, at = tid & 4095u;  // the grid is rows * 4096 / kBlock blocks exactly
    if (row >= n_slots * num_bounces) return;
    const uint32_t b = row / n_slots, sl = row - b * n_slots;
    const uint32_t count = frames[sl].frame_count * 25u + b;
    float          r1, r2;
    bluenoise_at(bluenoise, bluenoise_base(at & 63u, at >> 6), bluenoise_offset(count), bluenoise_shift(count), r1, r2);
    const HemiTerms h = hemisphere_terms(r1, r2);
    table[tid]        = make_float4(h.ca, h.cb, h.cos_theta, 0.0f);
}

void launch_sample_terms(hipStream_t stream, const float2* bluenoise, const FrameConst* frames, uint32_t n_slots, uint32_t num_bounces, float4* table)
{
    const uint32_t rows = n_slots * num_bounces;  // <= 64 * 255
    if (!rows) return;
    hipLaunchKernelGGL(k_sample_terms, dim3(rows * (4096u / kBlock)), dim3(kBlock), 0, stream, bluenoise, frames, n_slots, num_bounces, table);
}

// cap_debug_get(CAP_DEBUG_SELFTEST_SAMPLE_TABLE): every entry of a table against the sample as the kernels without the table draw it -- by
// pixel and count (bluenoise4x4) -- and hemisphere_terms of it, bit for bit, the unused word included.  out[0]: mismatches, out[1]: entries.
__global__ __launch_bounds__(kBlock) void k_sample_terms_selftest(const float2* bluenoise, const FrameConst* frames, uint32_t n_slots, uint32_t num_bounces,
                                                                  const float4* table, unsigned long long* out)
{
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, row = tid >> 12, at = tid & 4095u;
    if (row >= n_slots * num_bounces) return;
    const uint32_t b = row / n_slots, sl = row - b * n_slots;
    float          r1, r2;
    bluenoise4x4(bluenoise, at & 63u, at >> 6, frames[sl].frame_count * 25u + b, r1, r2);
    const HemiTerms h = hemisphere_terms(r1, r2);
    const float4    q = table[tid];
    const bool      bad = f2u(q.x) != f2u(h.ca) || f2u(q.y) != f2u(h.cb) || f2u(q.z) != f2u(h.cos_theta) || f2u(q.w) != 0u;
    const unsigned long long mb = __ballot(bad), mn = __ballot(true);
    if ((threadIdx.x & 63u) == 0u)
    {
        if (mb) atomicAdd(&out[0], (unsigned long long)__popcll(mb));
        atomicAdd(&out[1], (unsigned long long)__popcll(mn));
    }
}

void launch_sample_terms_selftest(hipStream_t stream, const float2* bluenoise, const FrameConst* frames, uint32_t n_slots, uint32_t num_bounces,
                                  const float4* table, unsigned long long* out_device)
{
    const uint32_t rows = n_slots * num_bounces;
    if (!rows) return;
    hipLaunchKernelGGL(k_sample_terms_selftest, dim3(rows * (4096u / kBlock)), dim3(kBlock), 0, stream, bluenoise, frames, n_slots, num_bounces, table, out_device);
}

// ---- the table of camera vertices (the HEAD kernel).  The frame slots of a batch share few sub-pixel jitters (eight: halton23 of
// frame_count mod 8), and bounce 0's camera ray, its closest hit and the vertex it interpolates depend on the slot through the jitter
// alone.  The host groups the slots by the bits of (jitter_x, jitter_y) -- frames[s].pad1 = the group of slot s, frames[g].pad2 = the first
// slot of group g -- and this kernel traces one camera ray per (group, padded pixel), one wave per 8 x 8 tile on a persistent grid:
// tab_p[g * Ppad + pl] = (p, code), tab_n[g * Ppad + pl] = (n, 0), the code being the word bounce 0 puts into color.w (kCodePadding,
// kCodeSky, kCodeKd, kCodeBlack; p = n = 0 without a vertex).  camera_vertex() is bounce 0's own sequence: the ray of
// small_scene_body.h's FIRST branch, its tile's pair mask, exhaustive_closest<ORG>, and shade_vertex's record gather, p,
// normalize3_tame(nm) and black test (untextured scene: the host's condition).  Same operations on the same operands: the same bits.
__device__ __forceinline__ void camera_vertex(const BvhDev& bvh, const ShadeArgs& a, const FrameConst& fc, uint32_t i, const float4* lds_shade,
                                              const float4* lds_rec, const float4* lds_org, const float4* lds_bounds, float4& cp, float4& cn)
{
    const uint32_t lane = threadIdx.x & 63u;
    Ray            r    = make_ray(mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 1.f), 0.0f, 0.0f);  // empty interval: hits nothing
    uint32_t       x, y;
    const bool     valid = local_pixel_to_xy(a.screen, i, x, y);
    if (valid) r = make_ray(mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]), primary_dir(a.cam, a.screen, fc, x, y), 0.0f, kPrimaryFar);
    uint32_t tx = 0, ty = 0;
    (void)local_pixel_to_xy(a.screen, i & ~63u, tx, ty);  // first pixel of the 8x8 tile
    const float4   b    = lds_bounds[lane < kExhaustiveMax / 2 ? lane : 0u];
    const bool     over = lane < bvh.fan_pair_count && b.x < (float)(tx + 8u) && b.z >= (float)tx && b.y < (float)(ty + 8u) && b.w >= (float)ty;
    const uint32_t pair_mask = (uint32_t)__ballot(over);
    float          t, u, v;
    uint32_t       gid;
    exhaustive_closest<true, false>(bvh, lds_rec, r, t, u, v, gid, lds_org, pair_mask);
    cp = make_float4(0.f, 0.f, 0.f, kCodePadding), cn = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid && gid == kInvalidId)
        cp.w = kCodeSky;
    else if (valid)
    {
        const float4* tab = lds_shade + kShadeRec * (size_t)gid;
        const float4  s0 = tab[0], s1 = tab[1], s2 = tab[2], s3 = tab[3], s4 = tab[4], s5 = tab[5];
        const float   w = (1.0f - u) - v;
        auto          mix = [&](float c0, float c1, float c2) { return fmaf(c2, v, fmaf(c1, u, c0 * w)); };
        const v3      nm = mk3(mix(s3.x, s4.x, s5.x), mix(s3.y, s4.y, s5.y), mix(s3.z, s4.z, s5.z));
        const v3      n  = normalize3_tame(nm);
        const v3      p  = mk3(mix(s0.x, s1.x, s2.x), mix(s0.y, s1.y, s2.y), mix(s0.z, s1.z, s2.z));
        const float   kd = a.scene.kd_untextured;
        cp = make_float4(p.x, p.y, p.z, kd < 1e-5f ? kCodeBlack : kCodeKd);
        cn = make_float4(n.x, n.y, n.z, 0.0f);
    }
}
// SELFTEST false: the table.  true (cap_debug_get(CAP_DEBUG_SELFTEST_CAMERA_TABLE)): one lane per (SLOT, padded pixel) evaluates bounce 0's
// sequence with the slot's own frame constants and compares all eight words with the entry of the slot's group; out[0]: mismatches,
// out[1]: entries compared.
template <bool SELFTEST>
__global__ __launch_bounds__(kBlock) void k_camera_vertices(BvhDev bvh, ShadeArgs a, uint32_t rows, float4* tab_p, float4* tab_n, unsigned long long* out)
{
    __shared__ float4 lds_shade[kShadeRec * kExhaustiveMax];
    __shared__ float4 lds_rec[4 * kExhaustiveMax];
    __shared__ float4 lds_org[kExhaustiveMax];
    __shared__ float4 lds_bounds[kExhaustiveMax / 2];
    stage_scene_records(bvh, a, lds_shade, lds_rec);
    stage_camera_pairs(bvh, a, lds_org, lds_bounds);
    __syncthreads();
    const uint32_t Ppad = a.screen.pixels_padded, cps = Ppad >> 6, chunks = cps * rows, lane = threadIdx.x & 63u;
    unsigned long long bad = 0, n = 0;
    for (uint32_t chunk = wave_global_id(); chunk < chunks; chunk += gridDim.x * (kBlock / 64))
    {
        const uint32_t   row = chunk / cps, i = (chunk - row * cps) * 64 + lane;  // row: the group, or the slot (SELFTEST)
        const FrameConst fc  = a.frames[SELFTEST ? row : f2u(a.frames[row].pad2)];
        float4           cp, cn;
        camera_vertex(bvh, a, fc, i, lds_shade, lds_rec, lds_org, lds_bounds, cp, cn);
        const size_t at = (size_t)(SELFTEST ? f2u(fc.pad1) : row) * Ppad + i;
        if (!SELFTEST)
            tab_p[at] = cp, tab_n[at] = cn;
        else
        {
            const float4 qp = tab_p[at], qn = tab_n[at];
            const bool   differ = f2u(qp.x) != f2u(cp.x) || f2u(qp.y) != f2u(cp.y) || f2u(qp.z) != f2u(cp.z) || f2u(qp.w) != f2u(cp.w) ||
                                f2u(qn.x) != f2u(cn.x) || f2u(qn.y) != f2u(cn.y) || f2u(qn.z) != f2u(cn.z) || f2u(qn.w) != f2u(cn.w);
            bad += (unsigned long long)__popcll(__ballot(differ)), n += 64ull;
        }
    }
    if (SELFTEST && lane == 0u)
    {
        if (bad) atomicAdd(&out[0], bad);
        if (n) atomicAdd(&out[1], n);
    }
}

void launch_camera_vertices(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, uint32_t rows, float4* tab_p, float4* tab_n,
                            unsigned long long* selftest_out)
{
    assert(bvh.tri_count <= kExhaustiveMax && args.scene.shade_tame != 0 && args.scene.texture_count == 0);  // the host's condition for the form
    const uint32_t chunks = (args.screen.pixels_padded >> 6) * rows;
    if (!chunks) return;
    const uint32_t gx = std::max(1u, std::min(cfg.grid_blocks, (chunks + kBlock / 64 - 1) / (kBlock / 64)));
    if (selftest_out)
        hipLaunchKernelGGL(k_camera_vertices<true>, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, args, rows, tab_p, tab_n, selftest_out);
    else
        hipLaunchKernelGGL(k_camera_vertices<false>, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, args, rows, tab_p, tab_n, selftest_out);
}

// cap_debug_get(CAP_DEBUG_SELFTEST_GRAY): what the GRAY form rests on, looked up in a 48-byte queue a render left behind -- every entry
// below its class's count (clamped to the capacity, as the consumers clamp it) has three bitwise equal throughput words.  out[0]: entries
// that do not, out[1]: entries looked at.
__global__ __launch_bounds__(kBlock) void k_gray_selftest(RayQueue q, unsigned long long* out)
{
    const uint32_t total = kQueueClasses * q.class_capacity;  // <= the queue's allocation (ctx_render.hip lane_sizes)
    unsigned long long bad = 0, n = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock)
    {
        const uint32_t klass = i / q.class_capacity, local = i - klass * q.class_capacity;
        const uint32_t count = q.count[klass * kCounterStride];
        bool           in = local < (count < q.class_capacity ? count : q.class_capacity), differ = false;
        if (in)
        {
            const float4 tp = q.thr_pid[i];
            differ          = f2u(tp.x) != f2u(tp.y) || f2u(tp.x) != f2u(tp.z);
        }
        bad += (unsigned long long)__popcll(__ballot(differ)), n += (unsigned long long)__popcll(__ballot(in));
    }
    if ((threadIdx.x & 63u) == 0u)
    {
        if (bad) atomicAdd(&out[0], bad);
        if (n) atomicAdd(&out[1], n);
    }
}

void launch_gray_selftest(hipStream_t stream, const RayQueue& q, unsigned long long* out_device)
{
    if (!q.class_capacity) return;
    const uint32_t total = kQueueClasses * q.class_capacity;
    hipLaunchKernelGGL(k_gray_selftest, dim3(std::min(4096u, (total + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, q, out_device);
}

// The twenty-three instantiations that exist, each under the tuple it was instantiated with.  Bounce 0 has no feedback form, the two
// models and feedback exclude each other, TAME is the reference model with the scene in LDS, CODE its bounce 0, TAB its three lean
// kernels with the sample table, HEAD the fourth, GRAY those four with 32-byte queue entries and SKYP the two of those that run at
// bounce >= 1 with the sky plane (TraceShadeCfg).
enum : uint32_t { TS_FIRST = 1, TS_EXT = 2, TS_FB = 4, TS_LDS = 8, TS_TAME = 16, TS_CODE = 32, TS_TAB = 64, TS_HEAD = 128, TS_GRAY = 256, TS_SKYP = 512 };
struct TraceShadeKernel
{
    uint32_t is;
    void (*kernel)(BvhDev, ShadeArgs);
};
template <uint32_t IS>
constexpr TraceShadeKernel trace_shade_kernel()
{
    if constexpr ((IS & TS_SKYP) != 0)
    {
        static_assert((IS & ~TS_HEAD) == (TS_LDS | TS_TAME | TS_TAB | TS_GRAY | TS_SKYP), "SKYP: the 32-byte bounce >= 1 kernel and its head form");
        return {IS, (IS & TS_HEAD) != 0 ? k_trace_shade_head_gray_sky : k_trace_shade_tab_gray_sky};
    }
    else if constexpr ((IS & TS_HEAD) != 0)
    {
        static_assert((IS & ~TS_GRAY) == (TS_LDS | TS_TAME | TS_TAB | TS_HEAD), "HEAD: the lean bounce >= 1 kernel");
        return {IS, (IS & TS_GRAY) != 0 ? k_trace_shade_head_gray : k_trace_shade_head};
    }
    else if constexpr ((IS & TS_GRAY) != 0)
    {
        static_assert((IS & ~(TS_FIRST | TS_CODE)) == (TS_LDS | TS_TAME | TS_TAB | TS_GRAY), "GRAY: the lean kernels with the sample table");
        static_assert((IS & TS_FIRST) != 0 || (IS & TS_CODE) == 0, "CODE: bounce 0");
        return {IS, k_trace_shade_tab_gray<(IS & TS_FIRST) != 0, (IS & TS_CODE) != 0>};
    }
    else if constexpr ((IS & TS_TAB) != 0)
    {
        static_assert((IS & ~(TS_FIRST | TS_CODE)) == (TS_LDS | TS_TAME | TS_TAB), "TAB: the lean kernels");
        return {IS, k_trace_shade_tab<(IS & TS_FIRST) != 0, (IS & TS_CODE) != 0>};
    }
    else
        return {IS, k_trace_shade<(IS & TS_FIRST) != 0, (IS & TS_EXT) != 0, (IS & TS_FB) != 0, (IS & TS_LDS) != 0, (IS & TS_TAME) != 0, (IS & TS_CODE) != 0>};
}
// (a build without the lean plumbing, -DCAP_CHUNK_PLAIN, has no table form: trace_shade_has_table_form() says so and the last ten are never looked up)
constexpr uint32_t         kTraceShadeKernelCount = 23;
constexpr TraceShadeKernel kTraceShadeKernels[kTraceShadeKernelCount] = {
    trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME | TS_CODE>(),
    trace_shade_kernel<TS_FIRST | TS_EXT | TS_LDS>(), trace_shade_kernel<TS_FIRST | TS_EXT>(),
    trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME>(), trace_shade_kernel<TS_FIRST | TS_LDS>(), trace_shade_kernel<TS_FIRST>(),
    trace_shade_kernel<TS_EXT | TS_LDS>(), trace_shade_kernel<TS_EXT>(),
    trace_shade_kernel<TS_FB | TS_LDS>(), trace_shade_kernel<TS_FB>(),
    trace_shade_kernel<TS_LDS | TS_TAME>(), trace_shade_kernel<TS_LDS>(), trace_shade_kernel<0>(),
    trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME | TS_CODE | TS_TAB>(), trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME | TS_TAB>(), trace_shade_kernel<TS_LDS | TS_TAME | TS_TAB>(),
    trace_shade_kernel<TS_LDS | TS_TAME | TS_TAB | TS_HEAD>(),
    trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME | TS_CODE | TS_TAB | TS_GRAY>(), trace_shade_kernel<TS_FIRST | TS_LDS | TS_TAME | TS_TAB | TS_GRAY>(),
    trace_shade_kernel<TS_LDS | TS_TAME | TS_TAB | TS_GRAY>(), trace_shade_kernel<TS_LDS | TS_TAME | TS_TAB | TS_HEAD | TS_GRAY>(),
    trace_shade_kernel<TS_LDS | TS_TAME | TS_TAB | TS_GRAY | TS_SKYP>(), trace_shade_kernel<TS_LDS | TS_TAME | TS_TAB | TS_HEAD | TS_GRAY | TS_SKYP>(),
};

// the unscaled forms: reference model, scene in LDS, tame shading records (-DCAP_SHADE_IEEE keeps the plain sqrtf and `/`
// everywhere for A/B runs: capsaicin_amd/variants/shadeieee.flags)
static bool tame_kernels(const BvhDev& bvh, const SceneDev& scene)
{
#if defined(CAP_SHADE_IEEE)
    return false;
#else
    return bvh.tri_count <= kExhaustiveMax && scene.shade_tame != 0;
#endif
}
bool trace_shade_has_code_form(const BvhDev& bvh, const SceneDev& scene) { return tame_kernels(bvh, scene); }
bool trace_shade_has_table_form(const BvhDev& bvh, const SceneDev& scene) { return kChunkLean && tame_kernels(bvh, scene); }
// the table kernels with 32-byte entries: kd = (k, k, k) at every vertex, which is what keeps a throughput's three components equal
bool trace_shade_has_gray_form(const BvhDev& bvh, const SceneDev& scene) { return trace_shade_has_table_form(bvh, scene) && scene.texture_count == 0; }

uint32_t launch_trace_shade(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, bool ext, bool feedback, bool camera_head, bool gray, bool sky_plane)
{
    const bool first = args.bounce == 0;
    const bool fb    = feedback && !ext && !first;  // (bounce 0 defines the planes' entries: nothing to reuse yet)
    const bool lds   = bvh.tri_count <= kExhaustiveMax;
    const bool tame  = !ext && !fb && tame_kernels(bvh, args.scene);
    const bool code  = first && args.code_in_color != 0u;
    assert(!code || tame);  // the host's condition for code_in_color: reference model and trace_shade_has_code_form()
    // the sample table: every launch of a batch or none (a queue entry of the other form carries no sample), so the host decides once
    // per batch, under its own condition -- reference model, no feedback, trace_shade_has_table_form()
    const bool tab = args.sample_terms != nullptr;
    assert(!tab || (tame && kChunkLean));
    // bounce 0 as the head of bounce 1's chunks (TraceShadeCfg HEAD): the host's condition implies the lean table form, the probe and the ring
    assert(!camera_head || (args.bounce == 1 && tab && args.inline_probe && args.wave_ring && args.in.org_tmin && args.in.dir_tmax && args.in.thr_pid));
    // 32-byte entries: like the table, every launch of a batch or none (the host's condition: the table form and trace_shade_has_gray_form())
    assert(!gray || (tab && args.scene.texture_count == 0));
    // the sky plane: every launch of a batch or none -- the head zeroes what the later launches store into and the resolve adds (the
    // host's condition: 32-byte entries, the head form and the code in the colour plane, whose albedo_in_w frees the plane's word)
    assert(!sky_plane || (gray && !first && args.albedo_in_w && args.code_in_color && args.planes.sky));
    const uint32_t is = (first ? TS_FIRST : 0u) | (ext ? TS_EXT : 0u) | (fb ? TS_FB : 0u) | (lds ? TS_LDS : 0u) | (tame ? TS_TAME : 0u) | (code ? TS_CODE : 0u) | (tab ? TS_TAB : 0u) |
                        (camera_head ? TS_HEAD : 0u) | (gray ? TS_GRAY : 0u) | (sky_plane ? TS_SKYP : 0u);
    // the queue's persistent grid; bounce 0's queue is the identity queue of the batch, one entry per padded pixel and frame slot
    const uint32_t gx = queue_grid(cfg, (first || camera_head) ? args.screen.pixels_padded * args.n_slots : args.max_count);
    const TraceShadeKernel* k = kTraceShadeKernels;
    while (k->is != is && k + 1 < kTraceShadeKernels + kTraceShadeKernelCount) ++k;
    assert(k->is == is);  // the table holds every tuple the lines above can derive
    hipLaunchKernelGGL(k->kernel, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, args);
    // the kernel's own conditions: the marked loop where it calls exhaustive_closest_marked, the carry chain where that takes it
#if defined(CAP_CLOSEST_V1)
    return 0u;
#else
    if (!lds || first) return 0u;
    return (kMarkCarry && bvh.tri_ids_dense) ? (bvh.tri_count > 32u ? 3u : 2u) : 1u;
#endif
}
}  // namespace cap
