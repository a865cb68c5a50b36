// kernels.hip — gfx950 (CDNA4) kernels of the tree path of the wavefront path tracer: the binary-tree walks and their queue kernels,
// the camera rays' packet walk, and the stand-alone shade stages (k_shade, k_primary_shade) with the binary-tree ray query.
// The exhaustive small-scene intersectors are in cap_exhaustive.h, the shading bodies in cap_shade.h, the fused small-scene kernel
// in small_scene.hip and the image-plane kernels in planes.hip.
//
// Reference semantics (paths relative to /root/reference/src/core/shaders): rt_primary_visibility.hlsl,
// rt_direct_lighting.hlsl, rt_indirect.hlsl, camera.h, sampling.h, lighting.h, shading.h, scene.h.
// The DXR TraceRay / acceleration structure (driver code in the reference) is replaced by the explicit
// traversal below.  No MFMA: nothing here is a dense contraction.
#include "cap_exhaustive.h"
#include "cap_kernels.h"
#include "cap_reproject.h"
#include "cap_shade.h"
#include "cap_trace.h"
#include "cap_unscaled.h"
#include "cap_wide_trace.h"

#include <cassert>

namespace cap
{
// Closest hit: minimum t, equal t resolved towards the lower global triangle id (visit-order independent).
// stack: this lane's column of the per-wave LDS stack; entry k lives at stack[k * kBlock].
template <int STACK>
__device__ __forceinline__ void traverse_closest(const BvhDev& bvh, const Ray& r, uint32_t* stack, float& best_t, float& best_u,
                                                 float& best_v, uint32_t& best_gid)
{
    best_t = r.tmax, best_u = 0.0f, best_v = 0.0f, best_gid = kInvalidId;
    if (bvh.tri_count == 0) return;
    int node = bvh.root;
    int sp   = 0;
    while (true)
    {
        if (node >= 0)
        {
            const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                         q3 = bvh.nodes[4 * node + 3];
            float      tn0, tn1;
            const bool h0 = slab(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, best_t, tn0);
            const bool h1 = slab(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, best_t, tn1);
            const int  c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
            if (h0 && h1)
            {
                const bool swap = tn1 < tn0;
                if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)(swap ? c0 : c1);
                node = swap ? c1 : c0;
                continue;
            }
            if (h0 || h1)
            {
                node = h0 ? c0 : c1;
                continue;
            }
        }
        else
        {
            // leaf = up to kLeafMax consecutive sorted triangles: ~(first | (count - 1) << kLeafCountShift)
            const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
            for (uint32_t leaf = first; leaf <= last; ++leaf)
            {
                const float4 t0 = bvh.tris[4 * leaf + 0], t1 = bvh.tris[4 * leaf + 1], t2 = bvh.tris[4 * leaf + 2];
                float        t, u, v;
                if (tri_test(r, t0, t1, t2, t, u, v))
                {
                    const uint32_t gid = f2u(bvh.tris[4 * leaf + 3].x);
                    if (t < best_t || (t == best_t && gid < best_gid)) best_t = t, best_u = u, best_v = v, best_gid = gid;
                }
            }
        }
        if (sp == 0) break;
        node = (int)stack[(--sp) * kBlock];
    }
}

// Any hit (RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH, lighting.h:49): true when some triangle has tmin < t < tmax.
template <int STACK>
__device__ __forceinline__ bool traverse_any(const BvhDev& bvh, const Ray& r, uint32_t* stack)
{
    if (bvh.tri_count == 0) return false;
    if (bvh.wide8_ok) return traverse_any8<STACK>(bvh, r, stack);  // wave-uniform
    int node = bvh.root;
    int sp   = 0;
    while (true)
    {
        if (node >= 0)
        {
            const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                         q3 = bvh.nodes[4 * node + 3];
            float      tn0, tn1;
            const bool h0 = slab(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r.tmax, tn0);
            const bool h1 = slab(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r.tmax, tn1);
            const int  c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
            if (h0 && h1)
            {
                if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)c1;
                node = c0;
                continue;
            }
            if (h0 || h1)
            {
                node = h0 ? c0 : c1;
                continue;
            }
        }
        else
        {
            const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
            for (uint32_t leaf = first; leaf <= last; ++leaf)
            {
                const float4 t0 = bvh.tris[4 * leaf + 0], t1 = bvh.tris[4 * leaf + 1], t2 = bvh.tris[4 * leaf + 2];
                if (tri_occludes(r, t0, t1, t2)) return true;
            }
        }
        if (sp == 0) break;
        node = (int)stack[(--sp) * kBlock];
    }
    return false;
}

// STACK == 0 selects the exhaustive small-scene path.
template <int STACK>
__device__ __forceinline__ void trace_closest_any_size(const BvhDev& bvh, const Ray& r, uint32_t* stack, float& t, float& u, float& v,
                                                       uint32_t& gid)
{
    if constexpr (STACK == 0)
        exhaustive_closest(bvh, bvh.tris_by_id, r, t, u, v, gid);
    else
        traverse_closest<STACK>(bvh, r, stack, t, u, v, gid);
}
template <int STACK>
__device__ __forceinline__ bool trace_any_any_size(const BvhDev& bvh, const Ray& r, uint32_t* stack, const float4* pre_row = nullptr)
{
    if constexpr (STACK == 0)
        return pre_row ? exhaustive_any<true>(bvh, r, pre_row) : exhaustive_any<false>(bvh, r);  // wave-uniform choice
    else
        return traverse_any<STACK>(bvh, r, stack);
}

// Workgroups per CU the stack kernels are register-allocated for: what their LDS stacks allow.  A workgroup's stack is
// entries x 256 lanes x 4 B; of 32-KB stacks four fit into the CU's 160 KB beside the runtime's own share, of 24-KB ones six.
// (0 = no hint: the small-scene kernels keep the compiler's default allocation; a hint of 8 squeezed k_trace_any<0> from 44 to
// 35 VGPRs and cost 9 %.)
constexpr int stack_residency(int stack_entries) { return stack_entries == 0 ? 0 : (stack_entries <= 24 ? 6 : (stack_entries <= 32 ? 4 : 2)); }

// One workgroup per four 64-pixel groups of a frame slot (blockIdx.y): camera rays are coherent but their cost varies strongly
// over the image, and a persistent grid with static slots left long tails here (4.1 -> 5.4 ms on the 262 k-triangle scene).
// The grid is therefore far larger than the wide traversal's spill area: binary traversal (wide8_ok cleared by the launcher).
template <int STACK>
__global__ __launch_bounds__(kBlock, stack_residency(STACK)) void k_trace_primary(BvhDev bvh, CameraDev cam, ScreenDev screen, const FrameConst* frames,
                                                          float4* hits)
{
    __shared__ uint32_t lds_stack[(STACK ? STACK : 1) * (STACK ? kBlock : 1)];
    uint32_t*           stack  = lds_stack + threadIdx.x;
    const uint32_t      slot   = blockIdx.y;
    const FrameConst    fc     = frames[slot];
    const uint32_t      chunks = screen.pixels_padded >> 6;
    for (uint32_t chunk = wave_global_id(); chunk < chunks; chunk += wave_total())
    {
        const uint32_t pl = chunk * 64 + (threadIdx.x & 63u);
        uint32_t       x, y;
        float          t = kPrimaryFar, u = 0.0f, v = 0.0f;
        uint32_t       gid = kInvalidId;
        if (local_pixel_to_xy(screen, pl, x, y))
        {
            const Ray r = make_ray(mk3(cam.position[0], cam.position[1], cam.position[2]), primary_dir(cam, screen, fc, x, y), 0.0f,
                                   kPrimaryFar);
            trace_closest_any_size<STACK>(bvh, r, stack, t, u, v, gid);
        }
        hits[(size_t)slot * screen.pixels_padded + pl] = make_float4(u, v, u2f(gid), t);
    }
}

// Packet traversal for camera rays.  The 64 rays of a chunk are the 8x8 pixels of one screen tile: they share an origin and
// nearly a direction, so the wave walks ONE node sequence with ONE stack (wave-uniform, in LDS) and fetches nodes and triangle
// records through the scalar cache; a child is entered when any lane's ray hits its box (each lane prunes with its own
// closest hit so far), nearer child first by majority.  Per-lane traversal is bound by the texture-address unit here -- seven
// 16-B loads per lane and step, 64 lanes, all to the same address: ~112 TA cycles per step and wave -- while this form issues no
// vector loads at all (262 k-triangle scene: 3.7 -> 2.4 ms; what then bounds it is instruction issue -- ~3 900 vector and ~1 800
// scalar instructions per packet, docs/experiments.md (85) -- not, as assumed until round 6, the chain of scalar fetches).  The same walk on the wide view of the tree, four boxes per step ordered by the packet's
// first live lane, was slower: 3.2 ms, the scalar sorting costs more than the halved fetch chain saves).
// The hit rule is visit-order independent (minimum t, ties to the lower id), so the result is bit-identical.
// wstack: this wave's kPacketStack entries (the tree depth is checked on the host against the same 64).
constexpr uint32_t kPacketStack = 64;
// One box of a packet step, written for what the step is bound by -- vector ISSUE (round 6: 3 880 vector instructions per packet at
// ~3 cycles each fill the SIMD's time; docs/experiments.md (85)).  Near and far plane as slab() picks them: the plane distance is
// monotonic in the plane (rounding is monotonic), increasing for inv > 0 and decreasing for inv < 0, so min / max of a slab's two
// distances IS the distance picked by the sign of inv -- a full-rate v_bitop3 select with the ray's sign word instead of a half-rate
// min / max.  Where slab()'s min / max drop a NaN (0 * inf) the select keeps it, and the max / min behind it drop it: only wider.
__device__ __forceinline__ float packet_sel(uint32_t m, float a, float b) { return u2f(__builtin_amdgcn_bitop3_b32(m, f2u(a), f2u(b), 0xca)); }
// v_max3 / v_min3 / v_max / v_min as the hardware has them.  Through fmaxf / fminf the compiler first canonicalises every operand it
// cannot prove quiet (four of the selected words per box, 4 cycles each): a signalling NaN would pass through v_max instead of being
// dropped.  None can occur here -- every operand is the result of an arithmetic instruction (NaNs from 0 * inf are quiet), a select
// between two such results, or a constant -- so the hardware forms drop NaNs exactly as fmaxf / fminf do.
__device__ __forceinline__ float packet_max3(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float packet_min3(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float packet_max(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float packet_min(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// Entry distance and (widened) exit distance of one box: the box is hit when tn <= tf.
// Plane distances as ONE fused operation each, t = fma(plane, inv, -(o * inv)), instead of slab()'s subtraction and product (12 of a
// step's vector instructions).  In space the crossing moves by at most u |o| (the rounding of o * inv) + u |plane - o| (the fma's),
// u = 2^-24, against slab()'s 2 u |plane - o|: both sit two orders of magnitude inside the boxes' padding of 1e-5 max(1, |coordinate|)
// for a camera within ~80 scene sizes of the scene (intersection contract), and the hit rule never looks at boxes.
// With inv = +-inf (a zero direction component) the fma can give inf - inf = NaN where slab() gave +-inf; the max / min drop it:
// the axis is ignored, which is wider.
// OCT 0 .. 7: the packet's 64 rays agree in the signs of their direction (all but the tiles a zero of a component runs through) and
// OCT holds them (bit 0: 1 / d.x negative, bit 1: y, bit 2: z): which plane is the near one is then known when the code is compiled,
// and the walk exists once per octant -- no select at all, vector or scalar (a scalar select per plane, 12 more scalar instructions
// per step, would only move the work to the unit that is second-busiest; (85)).  OCT 8: mixed signs, per-lane selects.
struct PacketSigns
{
    uint32_t mx, my, mz;  // per lane: all ones where 1 / d is negative
};
template <int OCT>
__device__ __forceinline__ void packet_slab(const Ray& r, v3 noi, const PacketSigns& g, float lox, float loy, float loz, float hix, float hiy,
                                            float hiz, float tfar, float& tn, float& tf)
{
    if constexpr (OCT < 8)
    {
        const float nx = (OCT & 1) ? hix : lox, ny = (OCT & 2) ? hiy : loy, nz = (OCT & 4) ? hiz : loz;
        const float fx = (OCT & 1) ? lox : hix, fy = (OCT & 2) ? loy : hiy, fz = (OCT & 4) ? loz : hiz;
        tn = packet_max(packet_max3(fmaf(nx, r.inv.x, noi.x), fmaf(ny, r.inv.y, noi.y), fmaf(nz, r.inv.z, noi.z)), r.tmin);
        tf = packet_min(packet_min3(fmaf(fx, r.inv.x, noi.x), fmaf(fy, r.inv.y, noi.y), fmaf(fz, r.inv.z, noi.z)), tfar) * 1.0000004f;
    }
    else
    {
        const float ax = fmaf(lox, r.inv.x, noi.x), bx = fmaf(hix, r.inv.x, noi.x);
        const float ay = fmaf(loy, r.inv.y, noi.y), by = fmaf(hiy, r.inv.y, noi.y);
        const float az = fmaf(loz, r.inv.z, noi.z), bz = fmaf(hiz, r.inv.z, noi.z);
        tn = packet_max(packet_max3(packet_sel(g.mx, bx, ax), packet_sel(g.my, by, ay), packet_sel(g.mz, bz, az)), r.tmin);
        tf = packet_min(packet_min3(packet_sel(g.mx, ax, bx), packet_sel(g.my, ay, by), packet_sel(g.mz, az, bz)), tfar) * 1.0000004f;
    }
}

template <int OCT>
__device__ __forceinline__ void packet_walk(const BvhDev& bvh, const Ray& r, v3 noi, const PacketSigns& g, unsigned long long alive_mask,
                                            uint32_t* wstack, float& best_t, float& best_u, float& best_v, uint32_t& best_gid)
{
    int      node = bvh.root;
    uint32_t sp   = 0;
    while (true)
    {
        node = __builtin_amdgcn_readfirstlane(node);
        bool pop = true;
        if (node >= 0)
        {
            float4 q0, q1, q2, q3;
            load_const_tri(bvh.nodes, (uint32_t)node, q0, q1, q2, q3);
            // (no `alive &&` around the tests: a lane without a pixel computes on its dummy ray; the branches cost scalar issue slots
            // and kept the two boxes from being scheduled together)
            float tn0, tn1, tf0, tf1;
            packet_slab<OCT>(r, noi, g, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, best_t, tn0, tf0);
            packet_slab<OCT>(r, noi, g, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, best_t, tn1, tf1);
            const int c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
            // Lanes that hit both vote for the nearer child, the others for the one they hit; the majority's child is entered first.
            // One rule for all three cases: only child 1 hit -> every voter says 1, only child 0 -> nobody does.
            // (the compares' lane masks, AND-ed with the mask of lanes that have a pixel: the ballot of a computed bool costs two
            // half-rate vector instructions, the ballot of a compare none)
            const unsigned long long m0 = __builtin_amdgcn_ballot_w64(tn0 <= tf0) & alive_mask, m1 = __builtin_amdgcn_ballot_w64(tn1 <= tf1) & alive_mask;
            const unsigned long long first1 = m1 & (~m0 | __builtin_amdgcn_ballot_w64(tn1 < tn0));
            const bool               swap   = 2 * __popcll(first1) > __popcll(m0 | m1);
            if ((m0 | m1) != 0ull)
            {
                // (no depth guard: the host refuses trees deeper than kPacketStack for this walk; the index is masked for safety)
                if (m0 != 0ull && m1 != 0ull) wstack[(sp++) & (kPacketStack - 1u)] = (uint32_t)(swap ? c0 : c1);
                node = swap ? c1 : c0;
                pop  = false;
            }
        }
        else
        {
            const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
            for (uint32_t leaf = first; leaf <= last; ++leaf)
            {
                float4 t0, t1, t2, t3;
                load_const_tri(bvh.tris, leaf, t0, t1, t2, t3);
                float t, u, v;
                // (a lane without a pixel walks its dummy ray: its result is dropped below.  Skipping the reciprocal and the interval test
                // when no lane of the wave is inside the triangle measured nothing: (85))
                if (tri_test(r, t0, t1, t2, t, u, v))
                {
                    const uint32_t gid = f2u(t3.x);
                    if (t < best_t || (t == best_t && gid < best_gid)) best_t = t, best_u = u, best_v = v, best_gid = gid;
                }
            }
        }
        if (pop)
        {
            if (sp == 0) break;
            node = (int)wstack[--sp];
        }
    }
}

__device__ __forceinline__ void traverse_closest_packet(const BvhDev& bvh, const Ray& r_in, bool alive, uint32_t* wstack, float& best_t,
                                                        float& best_u, float& best_v, uint32_t& best_gid)
{
    // 1 / d for the BOX tests from v_rcp_f32 (1 ulp; d = +-0 gives +-inf like the division): three IEEE divisions per ray less.  Like
    // the wide view's make_wide_ray: the boxes' padding covers it and the hit rule never looks at boxes (tri_test does not use inv).
    Ray r = r_in;
    r.inv = mk3(__builtin_amdgcn_rcpf(r.d.x), __builtin_amdgcn_rcpf(r.d.y), __builtin_amdgcn_rcpf(r.d.z));
    // (The camera position is wave-uniform and lives in scalar registers, like the triangle records: three moves per triangle test.
    // Pinning it into vector registers saves them and costs more in spills at this kernel's 64 registers: + 1 %.)
    const v3 noi = mk3(-(r.o.x * r.inv.x), -(r.o.y * r.inv.y), -(r.o.z * r.inv.z));
    PacketSigns g;
    g.mx = (uint32_t)((int)f2u(r.inv.x) >> 31), g.my = (uint32_t)((int)f2u(r.inv.y) >> 31), g.mz = (uint32_t)((int)f2u(r.inv.z) >> 31);
    const unsigned long long alive_mask = __builtin_amdgcn_ballot_w64(alive);
    const unsigned long long bx = __builtin_amdgcn_ballot_w64(g.mx != 0u), by = __builtin_amdgcn_ballot_w64(g.my != 0u),
                             bz = __builtin_amdgcn_ballot_w64(g.mz != 0u);
    // every lane of the wave is active here (the chunk loop is wave-uniform), so "all 64 agree" is a ballot of 0 or of all ones
    const bool     uniform = alive_mask == ~0ull && (bx == 0ull || bx == ~0ull) && (by == 0ull || by == ~0ull) && (bz == 0ull || bz == ~0ull);
    const uint32_t oct     = uniform ? ((bx != 0ull ? 1u : 0u) | (by != 0ull ? 2u : 0u) | (bz != 0ull ? 4u : 0u)) : 8u;
    best_t = r.tmax, best_u = 0.0f, best_v = 0.0f, best_gid = kInvalidId;
    switch (oct)
    {
#define CAP_PACKET_CASE(K) case K: packet_walk<K>(bvh, r, noi, g, alive_mask, wstack, best_t, best_u, best_v, best_gid); break;
        CAP_PACKET_CASE(0) CAP_PACKET_CASE(1) CAP_PACKET_CASE(2) CAP_PACKET_CASE(3) CAP_PACKET_CASE(4) CAP_PACKET_CASE(5) CAP_PACKET_CASE(6) CAP_PACKET_CASE(7)
#undef CAP_PACKET_CASE
        default: packet_walk<8>(bvh, r, noi, g, alive_mask, wstack, best_t, best_u, best_v, best_gid); break;
    }
    if (!alive) best_t = r.tmax, best_u = 0.0f, best_v = 0.0f, best_gid = kInvalidId;
}

template <int DUMMY>
__global__ __launch_bounds__(kBlock, 8) void k_trace_primary_packet(BvhDev bvh, CameraDev cam, ScreenDev screen, const FrameConst* frames,
                                                                    uint32_t n_slots, float4* hits, uint32_t* work)
{
    __shared__ uint32_t lds_wstack[(kBlock / 64) * kPacketStack];
    uint32_t*           wstack   = lds_wstack + (threadIdx.x >> 6) * kPacketStack;
    const uint32_t      cps      = screen.pixels_padded >> 6;
    const uint32_t      chunks   = cps * n_slots;
    const uint32_t      my_class = wave_global_id() % kQueueClasses;
    uint32_t            grab     = grab_issue(work, my_class);
    while (true)
    {
        const uint32_t chunk = grab_value(grab) * kQueueClasses + my_class;
        if (chunk >= chunks) break;
        grab = grab_issue(work, my_class);
        const uint32_t slot = chunk / cps;  // wave-uniform
        const uint32_t pl   = (chunk - slot * cps) * 64 + (threadIdx.x & 63u);
        uint32_t       x = 0, y = 0;
        const bool     alive = local_pixel_to_xy(screen, pl, x, y);
        const Ray      r     = make_ray(mk3(cam.position[0], cam.position[1], cam.position[2]),
                                        alive ? primary_dir(cam, screen, frames[slot], x, y) : mk3(0.f, 0.f, 1.f), 0.0f, kPrimaryFar);
        float          t, u, v;
        uint32_t       gid;
        traverse_closest_packet(bvh, r, alive, wstack, t, u, v, gid);
        hits[(size_t)slot * screen.pixels_padded + pl] = make_float4(alive ? u : 0.0f, alive ? v : 0.0f, u2f(gid), alive ? t : kPrimaryFar);
    }
}

// Camera rays as an "identity queue" for the wide closest-hit kernel (dense scenes, see launch_raygen_identity): entry i is the ray
// of (frame slot, local pixel) = (i / Ppad, i % Ppad), so the hit record lands where the bounce-0 shade stage looks for it.
// Padding lanes of partial tiles get an empty interval.  The 64 sub-queue counters are written here too: class k owns entries
// [k * capacity, min((k + 1) * capacity, total)).
__global__ __launch_bounds__(kBlock) void k_raygen_identity(CameraDev cam, ScreenDev screen, const FrameConst* frames, uint32_t n_slots, float4* org,
                                                            float4* dir, uint32_t* count, uint32_t capacity)
{
    const uint32_t Ppad = screen.pixels_padded, total = n_slots * Ppad;
    if (blockIdx.x == 0 && threadIdx.x < kQueueClasses)
    {
        const uint64_t begin = (uint64_t)threadIdx.x * capacity;
        count[threadIdx.x * kCounterStride] = begin < total ? (uint32_t)(total - begin < capacity ? total - begin : capacity) : 0u;
    }
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock)
    {
        const uint32_t slot = i / Ppad, pl = i - slot * Ppad;
        uint32_t       x = 0, y = 0;
        const bool     alive = local_pixel_to_xy(screen, pl, x, y);
        const v3       d     = alive ? primary_dir(cam, screen, frames[slot], x, y) : mk3(0.f, 0.f, 1.f);
        org[i] = make_float4(cam.position[0], cam.position[1], cam.position[2], 0.0f);
        dir[i] = make_float4(d.x, d.y, d.z, alive ? kPrimaryFar : 0.0f);
    }
}

void launch_raygen_identity(const LaunchCfg& cfg, const CameraDev& cam, const ScreenDev& screen, const FrameConst* frames, uint32_t n_slots,
                            const RayQueue& q)
{
    const uint32_t total = n_slots * screen.pixels_padded;
    uint32_t       g     = (total + kBlock - 1) / kBlock;
    const uint32_t cap   = (cfg.cu_count ? cfg.cu_count : 256u) * 8u;
    if (g > cap) g = cap;
    if (g == 0) g = 1;
    hipLaunchKernelGGL(k_raygen_identity, dim3(g), dim3(kBlock), 0, cfg.stream, cam, screen, frames, n_slots, q.org_tmin, q.dir_tmax, q.count,
                       q.class_capacity);
}

template <int STACK>
__global__ __launch_bounds__(kBlock, stack_residency(STACK)) void k_trace_closest(BvhDev bvh, RayQueue q, float4* hits)
{
    __shared__ uint32_t lds_stack[(STACK ? STACK : 1) * (STACK ? kBlock : 1)];
    uint32_t*           stack  = lds_stack + threadIdx.x;
    const uint32_t      slots  = (q.class_capacity >> 6) * kQueueClasses;
    for (uint32_t cs = wave_global_id(); cs < slots; cs += wave_total())
    {
        uint32_t i, klass;
        if (queue_chunk(q.count, q.class_capacity, cs, threadIdx.x & 63u, i, klass))
        {
            const float4 a = q.org_tmin[i], b = q.dir_tmax[i];
            const Ray    r = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
            float        t, u, v;
            uint32_t     gid;
            trace_closest_any_size<STACK>(bvh, r, stack, t, u, v, gid);
            hits[i] = make_float4(u, v, u2f(gid), t);
        }
    }
}

// An unoccluded ray adds its contribution to its path's plane entry by load-add-store: the path is the entry's only writer
// within a launch and launches are ordered on the stream, so the sums are the same IEEE additions in the same order whichever
// way they are carried out.  RMW says WHEN the entry is loaded.  true: up front with the ray (next-event rays of the EXT model,
// ~90 % unoccluded: the load's latency hides behind the test; three float atomics per ray instead made the L2 atomic rate the
// kernel's bound, 31 -> 10.8 ms per step).  false: after the test, by the few lanes that need it (the reference's directional
// light inside the box: ~5 % unoccluded; an up-front load costs 7.05 -> 7.98 ms, float atomics 6.6 ms, this 5.8 ms).
// Entry formats.  RMW (EXT model, next-event rays): (origin, tmin) (direction, tmax) (contribution, path id), 48 B.
// !RMW (reference model): (origin, path id) (contribution, -), 32 B; direction = the light of the path's frame (LDS copy of the
// batch's frame constants), tmin / tmax = kRayEps / kRayFar (lighting.h:39-47).
// k_trace_any's table of PairPre entries lives in dynamic LDS (pre_table_bytes(), passed at launch; 0 = no table): rows of
// 2 * pairs + 1 float4 per frame slot -- the extra one shifts the banks, so that lanes reading the same pair of different frame
// slots do not collide.  8 KB for the headline's 16-frame batches, 34 KB for a 64-frame batch of a sharded run.
constexpr uint32_t kPreTableMaxBytes = 40u << 10;
static inline uint32_t pre_table_bytes(uint32_t n_slots, uint32_t pairs)
{
    const uint64_t b = (uint64_t)n_slots * (2u * pairs + 1u) * sizeof(float4);
    return (pairs && n_slots <= kMaxFrameSlots && b <= kPreTableMaxBytes) ? (uint32_t)b : 0u;
}
// CODE (launch_trace_any's code_plane, bounce 0 under ShadeArgs::code_in_color): nothing has written target[idx] in this batch.  The
// parent form added the contribution c to the (0, 0, 0) bounce 0 had stored there; 0 + c has the bits of c because no component of c
// is -0 -- every factor of it is >= +0 (light intensity, kd, 1 / pi, ndl = fmaxf(0, .)) -- so c is stored as it is, without the load.
// The path's word in the colour plane goes from its code (the entry's spare word) to code + 4: "direct holds a value" (k_resolve_coded).
// This launch runs before bounce 1's on the same stream, and the path is the only writer of both entries in it.
__device__ __forceinline__ void store_first_direct(float4* target, float4* code_plane, size_t idx, float4 c)
{
    target[idx] = make_float4(c.x, c.y, c.z, 0.0f);
    reinterpret_cast<float*>(code_plane + idx)[3] = c.w + kCodeLit;  // c.w: the entry's spare word, the code shade_vertex put into color.w
}
template <int STACK, bool RMW, bool CODE = false>
__global__ __launch_bounds__(kBlock, stack_residency(STACK)) void k_trace_any(BvhDev bvh, ShadowQueue q, float4* target, uint32_t pixels_padded, uint32_t n_slots,
                                                      uint64_t* guard, uint32_t* work, const FrameConst* frames, uint32_t pre_bytes,
                                                      float4* code_plane)
{
    static_assert(!CODE || (STACK == 0 && !RMW), "CODE: the small-scene path's reference-model shadow rays");
    extern __shared__ float4 lds_pre[];
    __shared__ uint32_t lds_stack[(STACK ? STACK : 1) * (STACK ? kBlock : 1)];
    __shared__ float4   lds_light[RMW ? 1 : kMaxFrameSlots];
    // reference model on the small-scene path: the direction-dependent part of the pair tests per (frame slot, pair), see PairPre
    constexpr bool      DDN = STACK == 0 && !RMW;
    uint32_t*           stack    = lds_stack + threadIdx.x;
    const uint32_t      pre_row  = 2u * bvh.fan_pair_count + 1u;  // float4 per frame slot
    const bool          use_ddn  = DDN && pre_bytes != 0u;
    if (!RMW)
    {
        for (uint32_t k = threadIdx.x; k < n_slots && k < kMaxFrameSlots; k += kBlock)
            lds_light[k] = make_float4(frames[k].light_dir[0], frames[k].light_dir[1], frames[k].light_dir[2], 0.f);
        if (use_ddn)
        {
            const uint32_t np = bvh.fan_pair_count;
            const float*   fp = reinterpret_cast<const float*>(bvh.fan_pairs);
            for (uint32_t e = threadIdx.x; e < n_slots * np; e += kBlock)
            {
                const uint32_t slot = e / np, k = e - slot * np;
                const v3       d    = mk3(frames[slot].light_dir[0], frames[slot].light_dir[1], frames[slot].light_dir[2]);
                const float*   rec  = fp + 20 * (size_t)k;  // (v0, e1, e2, e3, nA, nB, id, 0)
                lds_pre[slot * pre_row + 2 * k]     = tri_pre(d, mk3(rec[12], rec[13], rec[14]), kRayEps, kRayFar);
                lds_pre[slot * pre_row + 2 * k + 1] = tri_pre(d, mk3(rec[15], rec[16], rec[17]), kRayEps, kRayFar);
            }
        }
        __syncthreads();
    }
    // Reference model on the wide tree: every shadow ray of the launch points at its frame's light, and the frames of a batch differ by
    // a jitter -- one direction octant for the whole launch unless a component of the light direction is (almost) zero.  Told here from
    // the LDS copy of the lights (sign bits, as make_wide_ray reads them off 1 / d); the traversal then runs in the copy compiled for
    // that octant (traverse_any8<.., OCT>: near / far planes and the visiting permutation are constants; docs/experiments.md (86)).
    uint32_t oct = 8u;  // mixed, or not this instantiation: per-lane signs
    if constexpr (!RMW && STACK == (int)kWideLdsEntries)
    {
        const float4   L  = lds_light[(threadIdx.x & 63u) < n_slots ? (threadIdx.x & 63u) : 0u];
        const uint32_t o  = (f2u(L.x) >> 31) | ((f2u(L.y) >> 31) << 1) | ((f2u(L.z) >> 31) << 2);
        const uint32_t o0 = __builtin_amdgcn_readfirstlane(o);
        if (__builtin_amdgcn_ballot_w64(o != o0) == 0ull && bvh.wide8_ok && bvh.tri_count != 0u) oct = o0;  // (all 64 lanes are active here)
    }
    // Memory round trips a chunk starts with, in order: (1) the grab issued one chunk ago (its wait also covers the previous
    // chunk's plane updates: vmcnt retires in order), (2) the queue entry.  The class's length is read once per wave (constant
    // during the launch), and the next grab is issued AFTER the entry loads, so that the wait for the entry is a counted
    // vmcnt(1) that leaves the grab in flight instead of a third round trip.
    const uint32_t my_class = wave_global_id() % kQueueClasses;
    const uint32_t lane     = threadIdx.x & 63u;
    uint32_t       n_class  = q.count[my_class * kCounterStride];
    n_class                 = n_class < q.class_capacity ? n_class : q.class_capacity;
    uint32_t       grab     = grab_issue(work, my_class);
    while (true)
    {
        const uint32_t local0 = grab_value(grab) * 64u;
        if (local0 >= n_class) break;  // past the end of this class's sub-queue
        const bool     active = local0 + lane < n_class;
        const uint32_t i      = my_class * q.class_capacity + local0 + lane;
        float4         a      = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) a = q.org_tmin[i];
        grab = grab_issue(work, my_class);
        if (active)
        {
            float4       c = make_float4(0.f, 0.f, 0.f, 0.f), cur = c;
            uint32_t     pid = 0;
            size_t       idx = 0;
            bool         good = true;
            auto         locate = [&]() {
                good = (pid >> kPidShift) < n_slots && (pid & kPidMask) < pixels_padded;
                idx  = (size_t)(pid >> kPidShift) * pixels_padded + (pid & kPidMask);
                if (!good)
                {
                    // never true for a well-formed queue; reported through CapStats::guard_* instead of faulting
                    atomicAdd((unsigned long long*)guard + 2, 1ull);
                    guard[3] = ((uint64_t)i << 32) | pid;
                }
            };
            Ray r;
            if (RMW)
            {
                const float4 b = q.dir_tmax[i];
                r   = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
                c   = q.contrib_pid[i];
                pid = f2u(c.w);
                locate();
                if (good) cur = target[idx];
            }
            else
            {
                pid = f2u(a.w);
                locate();
                const float4 L = lds_light[good ? (pid >> kPidShift) : 0u];
                r = make_ray(mk3(a.x, a.y, a.z), mk3(L.x, L.y, L.z), kRayEps, good ? kRayFar : 0.0f);  // malformed entry: empty interval
            }
            const float4* row = use_ddn ? lds_pre + (good ? (pid >> kPidShift) : 0u) * pre_row : nullptr;
            if (STACK == 0) __builtin_amdgcn_s_setprio(0);
            bool occluded;
            if constexpr (!RMW && STACK == (int)kWideLdsEntries)
            {
                switch (oct)  // wave-uniform
                {
#define CAP_ANY_OCT(K) case K: occluded = traverse_any8<STACK, K>(bvh, r, stack); break;
                    // (the four octants the reference's light visits: it turns about the vertical axis, y stays positive -- lighting.h:20-33;
                    // tests/test_sponza_class_gpu.py test_light_octants_parity renders a frame of each)
                    CAP_ANY_OCT(0) CAP_ANY_OCT(1) CAP_ANY_OCT(4) CAP_ANY_OCT(5)
#undef CAP_ANY_OCT
                    default: occluded = trace_any_any_size<STACK>(bvh, r, stack, row); break;
                }
            }
            else
                occluded = trace_any_any_size<STACK>(bvh, r, stack, row);
            if (STACK == 0) __builtin_amdgcn_s_setprio(3);
            if (!occluded)
            {
                // lighting.h:57-60: unoccluded -> the contribution evaluated at shading time is added
                if (good)
                {
                    if (RMW)
                        target[idx] = make_float4(cur.x + c.x, cur.y + c.y, cur.z + c.z, cur.w);
                    else if constexpr (CODE)
                        store_first_direct(target, code_plane, idx, q.contrib_pid[i]);
                    else
                    {
                        c           = q.contrib_pid[i];
                        cur         = target[idx];
                        target[idx] = make_float4(cur.x + c.x, cur.y + c.y, cur.z + c.z, cur.w);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Shadow rays of the reference model on small scenes, with occluder-first ordering and wave-level compaction.
//
// An any-hit query is over at the first occluder, but the exhaustive loop is wave-uniform: it could only stop early when all 64
// rays of the wave are occluded.  Inside a box most shadow rays ARE occluded, and by very few of the triangles -- whatever lies
// farthest along the light direction (the ceiling of the Cornell box for the reference's light from above: 84 % of the shadow
// rays of the headline workload; the other 16 % leave through the open front).  So the loop is split:
//   probe   every ray is tested against the first `probe` fan pairs of an order sorted by how far along the light direction a
//           pair's centre lies (per launch, for the light of the batch's first frame);
//   rest    the rays that survived are parked in a per-wave LDS buffer; whenever 64 of them have gathered, the wave tests those 64
//           against the remaining pairs and the unpaired triangles, and adds the contributions of the unoccluded ones.
// An occlusion query's answer does not depend on the order of the tests, and each path has at most one shadow entry per launch,
// so the planes receive the same additions as in k_trace_any: bit-identical images and counters.
// ------------------------------------------------------------------------------------------------
#ifndef CAP_ANY_GRAB
#define CAP_ANY_GRAB 4  // chunk slots per grab of the probe kernel
#endif
#ifndef CAP_ANY_PROBE
#define CAP_ANY_PROBE 1
#endif
constexpr uint32_t kSurvivorCap = 128;  // per wave: <= 63 parked + <= 64 new
template <bool CODE>  // see k_trace_any
__global__ __launch_bounds__(kBlock) void k_trace_any_small(BvhDev bvh, ShadowQueue q, float4* target, uint32_t pixels_padded, uint32_t n_slots,
                                                           uint64_t* guard, uint32_t* work, const FrameConst* frames, uint32_t probe,
                                                           float4* code_plane)
{
    extern __shared__ float4 lds_pre[];  // PairPre rows per frame slot, see k_trace_any
    __shared__ float4   lds_light[kMaxFrameSlots];
    __shared__ float    lds_score[kExhaustiveMax / 2];
    __shared__ uint32_t lds_order[kExhaustiveMax / 2];
    __shared__ float4   lds_surv[(kBlock / 64) * kSurvivorCap];    // (origin, path id) of parked rays
    __shared__ uint32_t lds_surv_i[(kBlock / 64) * kSurvivorCap];  // their queue entries
    const uint32_t np      = bvh.fan_pair_count;  // <= kExhaustiveMax / 2
    const uint32_t pre_row = 2u * np + 1u;
    const float*   fp      = reinterpret_cast<const float*>(bvh.fan_pairs);
    for (uint32_t k = threadIdx.x; k < n_slots && k < kMaxFrameSlots; k += kBlock)
        lds_light[k] = make_float4(frames[k].light_dir[0], frames[k].light_dir[1], frames[k].light_dir[2], 0.f);
    for (uint32_t e = threadIdx.x; e < n_slots * np; e += kBlock)
    {
        const uint32_t slot = e / np, k = e - slot * np;
        const v3       d    = mk3(frames[slot].light_dir[0], frames[slot].light_dir[1], frames[slot].light_dir[2]);
        const float*   rec  = fp + 20 * (size_t)k;  // (v0, e1, e2, e3, nA, nB, id, 0)
        lds_pre[slot * pre_row + 2 * k]     = tri_pre(d, mk3(rec[12], rec[13], rec[14]), kRayEps, kRayFar);
        lds_pre[slot * pre_row + 2 * k + 1] = tri_pre(d, mk3(rec[15], rec[16], rec[17]), kRayEps, kRayFar);
    }
    if (threadIdx.x < np)
    {
        const float* rec = fp + 20 * (size_t)threadIdx.x;
        const v3     L   = mk3(frames[0].light_dir[0], frames[0].light_dir[1], frames[0].light_dir[2]);
        const v3     v0  = mk3(rec[0], rec[1], rec[2]);
        float        sc  = dot3(v0, L);  // sum over the quad's four vertices = 4 x its centre's reach
        for (int e = 0; e < 3; ++e) sc += dot3(v0 + mk3(rec[3 + 3 * e], rec[4 + 3 * e], rec[5 + 3 * e]), L);
        lds_score[threadIdx.x] = sc;
    }
    __syncthreads();
    if (threadIdx.x < np)
    {
        // rank sort: position = pairs whose centre lies farther along the light (ties by index)
        const float sc   = lds_score[threadIdx.x];
        uint32_t    rank = 0;
        for (uint32_t j = 0; j < np; ++j)
        {
            const float o = lds_score[j];
            rank += (o > sc || (o == sc && j < threadIdx.x)) ? 1u : 0u;
        }
        lds_order[rank] = threadIdx.x;
    }
    __syncthreads();
    const uint32_t  n_probe = probe < np ? probe : np;
    const uint32_t  lane    = threadIdx.x & 63u;
    float4* const   surv    = lds_surv + (threadIdx.x >> 6) * kSurvivorCap;
    uint32_t* const surv_i  = lds_surv_i + (threadIdx.x >> 6) * kSurvivorCap;
    uint32_t        surv_n  = 0;  // wave-uniform

    // the rest of the tests for the parked rays [first, first + count), count <= 64
    auto finish = [&](uint32_t first, uint32_t count) {
        if (lane < count)
        {
            const float4   a    = surv[first + lane];
            const uint32_t i    = surv_i[first + lane];
            const uint32_t pid  = f2u(a.w);
            const bool     good = (pid >> kPidShift) < n_slots && (pid & kPidMask) < pixels_padded;  // counted once, in the probe
            const uint32_t slot = good ? (pid >> kPidShift) : 0u;
            const float4   L    = lds_light[slot];
            const Ray      r    = make_ray(mk3(a.x, a.y, a.z), mk3(L.x, L.y, L.z), kRayEps, good ? kRayFar : 0.0f);
            const float4*  row  = lds_pre + slot * pre_row;
            bool           hit  = false;
            for (uint32_t j = n_probe; j < np; ++j)
            {
                const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_order[j]);  // wave-uniform: scalar-cache record
                hit |= pair_occludes_pre(r, bvh.fan_pairs, k, row[2 * k], row[2 * k + 1]);
            }
            const uint32_t ns = bvh.fan_single_count;
            for (uint32_t j = 0; j < ns; ++j)
            {
                float4 t0, t1, t2, t3;
                load_const_tri(bvh.fan_singles, j, t0, t1, t2, t3);
                hit |= tri_occludes(r, t0, t1, t2);
            }
            if (!hit && good)
            {
                // lighting.h:57-60: unoccluded -> the contribution evaluated at shading time is added
                const size_t idx = (size_t)(pid >> kPidShift) * pixels_padded + (pid & kPidMask);
                if constexpr (CODE)
                    store_first_direct(target, code_plane, idx, q.contrib_pid[i]);
                else
                {
                    const float4 c = q.contrib_pid[i], cur = target[idx];
                    target[idx]    = make_float4(cur.x + c.x, cur.y + c.y, cur.z + c.z, cur.w);
                }
            }
        }
    };

    const uint32_t my_class = wave_global_id() % kQueueClasses;
    uint32_t       n_class  = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.count[my_class * kCounterStride]);
    n_class                 = n_class < q.class_capacity ? n_class : q.class_capacity;
    // The probe is short (a few hundred cycles per chunk), far shorter than a returned device atomic or a queue-entry load take:
    // a grab therefore fetches kGrabChunks consecutive chunk slots of the class, the grab for the next group is issued when a
    // group is started, and within the stream of chunks the entry of the NEXT chunk is loaded before this chunk is worked on.
    constexpr uint32_t kGrabChunks = CAP_ANY_GRAB;
    auto grab_group = [&]() {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(work + my_class * kCounterStride, kGrabChunks);
        return v;
    };
    uint32_t grab     = grab_group();
    uint32_t local0   = grab_value(grab) * 64u;  // first ray of the chunk being worked on
    grab              = grab_group();
    uint32_t in_group = 0;
    float4   a_next   = make_float4(0.f, 0.f, 0.f, 0.f);
    if (local0 + lane < n_class) a_next = q.org_tmin[my_class * q.class_capacity + local0 + lane];
    while (true)
    {
        if (local0 >= n_class) break;  // past the end of this class's sub-queue (groups are handed out in order)
        const bool     active = local0 + lane < n_class;
        const uint32_t i      = my_class * q.class_capacity + local0 + lane;
        const float4   a      = a_next;
        // the next chunk: the next one of this group, or the first one of the next group
        if (++in_group == kGrabChunks)
        {
            in_group = 0;
            local0   = grab_value(grab) * 64u;
            grab     = grab_group();
        }
        else
            local0 += 64u;
        if (local0 + lane < n_class) a_next = q.org_tmin[my_class * q.class_capacity + local0 + lane];
        bool hit = false;
        if (active)
        {
            const uint32_t pid  = f2u(a.w);
            const bool     good = (pid >> kPidShift) < n_slots && (pid & kPidMask) < pixels_padded;
            if (!good)
            {
                // never true for a well-formed queue; reported through CapStats::guard_* instead of faulting
                atomicAdd((unsigned long long*)guard + 2, 1ull);
                guard[3] = ((uint64_t)i << 32) | pid;
            }
            const uint32_t slot = good ? (pid >> kPidShift) : 0u;
            const float4   L    = lds_light[slot];
            const Ray      r    = make_ray(mk3(a.x, a.y, a.z), mk3(L.x, L.y, L.z), kRayEps, good ? kRayFar : 0.0f);
            const float4*  row  = lds_pre + slot * pre_row;
            for (uint32_t j = 0; j < n_probe; ++j)
            {
                const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_order[j]);
                hit |= pair_occludes_pre(r, bvh.fan_pairs, k, row[2 * k], row[2 * k + 1]);
            }
        }
        // park the survivors
        const bool               alive = active && !hit;
        const unsigned long long m     = __ballot(alive);
        if (alive)
        {
            const uint32_t at = surv_n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            surv[at]   = a;
            surv_i[at] = i;
        }
        surv_n += (uint32_t)__popcll(m);
        wave_handoff();
        if (surv_n >= 64u)
        {
            surv_n -= 64u;
            finish(surv_n, 64u);
            wave_handoff();
        }
    }
    if (surv_n) finish(0u, surv_n);
}

// ------------------------------------------------------------------------------------------------
// LBVH traversal with lane refill.  Incoherent rays leave a wave in the stack loop for the MAXIMUM of 64 traversal lengths
// (measured on the 262 k-triangle scene: 11 of 64 lanes active on average).  Here a lane that finishes its ray takes the next
// ray of the wave's own chunk sequence, so the wave keeps its lanes busy until that sequence is exhausted.  The feed is
// wave-uniform bookkeeping (no atomics); every ray is still traced by exactly one lane and writes its own queue index.
// ------------------------------------------------------------------------------------------------
struct WaveFeed
{
    uint32_t cs, slots, stride;  // next chunk slot of this wave, slot count, slot stride (waves in the grid)
    uint32_t base, n, pos;       // current chunk: first queue index, rays in it, rays already handed out
    bool     exhausted;
};

__device__ __forceinline__ void feed_init(WaveFeed& f, uint32_t class_capacity)
{
    f.cs = wave_global_id(), f.slots = (class_capacity >> 6) * kQueueClasses, f.stride = wave_total();
    f.base = f.n = f.pos = 0;
    f.exhausted = false;
}

// Move to this wave's next non-empty chunk.  All values are wave-uniform.
__device__ __forceinline__ void feed_advance(WaveFeed& f, const uint32_t* count, uint32_t class_capacity)
{
    while (f.pos >= f.n && !f.exhausted)
    {
        if (f.cs >= f.slots)
        {
            f.exhausted = true;
            break;
        }
        const uint32_t klass = f.cs % kQueueClasses, j = f.cs / kQueueClasses;
        const uint32_t cnt   = __builtin_amdgcn_readfirstlane(count[klass * kCounterStride]);
        const uint32_t start = j * 64u;
        f.n    = cnt > start ? min(64u, cnt - start) : 0u;
        f.base = klass * class_capacity + start;
        f.pos  = 0;
        f.cs += f.stride;
    }
}

// Hands rays to idle lanes; returns this lane's new queue index or ~0u.
__device__ __forceinline__ uint32_t feed_take(WaveFeed& f, bool idle, const uint32_t* count, uint32_t class_capacity)
{
    uint32_t           mine = kInvalidId;
    unsigned long long mask = __ballot(idle);
    while (mask != 0ull)
    {
        feed_advance(f, count, class_capacity);
        if (f.exhausted) break;
        const uint32_t lane  = threadIdx.x & 63u;
        const uint32_t rank  = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const uint32_t avail = f.n - f.pos, want = (uint32_t)__popcll(mask);
        const uint32_t take  = avail < want ? avail : want;
        if (idle && mine == kInvalidId && rank < take) mine = f.base + f.pos + rank;
        f.pos += take;
        mask = __ballot(idle && mine == kInvalidId);
    }
    return mine;
}

#ifndef CAP_REFILL_IDLE
#define CAP_REFILL_IDLE 28
#endif
#ifndef CAP_LEAF_BATCH
#define CAP_LEAF_BATCH 24
#endif
constexpr uint32_t kRefillIdle = CAP_REFILL_IDLE;  // refill once this many lanes are idle (amortises the ray-load latency over several lanes)
constexpr int      kLeafBatch  = CAP_LEAF_BATCH;  // keep running the box code while at least this many lanes are on internal nodes

template <int STACK>
__global__ __launch_bounds__(kBlock, stack_residency(STACK)) void k_trace_closest_refill(BvhDev bvh, RayQueue q, float4* hits)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t*           stack = lds_stack + threadIdx.x;
    WaveFeed            feed;
    feed_init(feed, q.class_capacity);
    if (bvh.tri_count == 0)
    {
        // no geometry: every queued ray misses
        for (uint32_t cs = wave_global_id(); cs < feed.slots; cs += wave_total())
        {
            uint32_t i, klass;
            if (queue_chunk(q.count, q.class_capacity, cs, threadIdx.x & 63u, i, klass)) hits[i] = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
        }
        return;
    }
    bool     alive = false;
    Ray      r     = make_ray(mk3(0, 0, 0), mk3(0, 0, 1), 0.f, 0.f);
    float    best_t = 0.f, best_u = 0.f, best_v = 0.f;
    uint32_t best_gid = kInvalidId, out = 0;
    int      node = 0, sp = 0;
    while (true)
    {
        const uint32_t n_alive = (uint32_t)__popcll(__ballot(alive));
        if (!feed.exhausted && 64u - n_alive >= kRefillIdle)
        {
            const uint32_t i = feed_take(feed, !alive, q.count, q.class_capacity);
            if (i != kInvalidId)
            {
                const float4 a = q.org_tmin[i], b = q.dir_tmax[i];
                r      = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
                best_t = r.tmax, best_u = 0.f, best_v = 0.f, best_gid = kInvalidId;
                out = i, node = bvh.root, sp = 0, alive = true;
            }
        }
        if (__ballot(alive) == 0ull) break;  // feed exhausted and every lane retired
        // while-while: as long as enough lanes sit on an internal node only the box code runs; lanes that reached a leaf wait
        // until leaves are due (few lanes left on internal nodes), then only the triangle code runs.  Every iteration pays for
        // one of the two bodies instead of both.
        const unsigned long long m_inner = __ballot(alive && node >= 0);
        const unsigned long long m_leaf  = __ballot(alive && node < 0);
        const bool               inner_phase = __popcll(m_inner) >= kLeafBatch || m_leaf == 0ull;
        bool pop = false;
        if (inner_phase)
        {
            if (alive && node >= 0)
            {
                const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                             q3 = bvh.nodes[4 * node + 3];
                float      tn0, tn1;
                const bool h0 = slab(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, best_t, tn0);
                const bool h1 = slab(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, best_t, tn1);
                const int  c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
                pop           = true;
                if (h0 && h1)
                {
                    const bool swap = tn1 < tn0;
                    if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)(swap ? c0 : c1);
                    node = swap ? c1 : c0;
                    pop  = false;
                }
                else if (h0 || h1)
                {
                    node = h0 ? c0 : c1;
                    pop  = false;
                }
            }
        }
        else if (alive && node < 0)
        {
            const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
            for (uint32_t leaf = first; leaf <= last; ++leaf)
            {
                const float4 t0 = bvh.tris[4 * leaf + 0], t1 = bvh.tris[4 * leaf + 1], t2 = bvh.tris[4 * leaf + 2];
                float        t, u, v;
                if (tri_test(r, t0, t1, t2, t, u, v))
                {
                    const uint32_t gid = f2u(bvh.tris[4 * leaf + 3].x);
                    if (t < best_t || (t == best_t && gid < best_gid)) best_t = t, best_u = u, best_v = v, best_gid = gid;
                }
            }
            pop = true;
        }
        if (pop)
        {
            if (sp == 0)
            {
                hits[out] = make_float4(best_u, best_v, u2f(best_gid), best_t);
                alive     = false;
            }
            else
                node = (int)stack[(--sp) * kBlock];
        }
    }
}

// the wide traversal paths need every thread of the (1-D) grid to own a slice of the spill area
static BvhDev for_grid(const BvhDev& bvh, uint32_t grid_blocks)
{
    BvhDev b = bvh;
    if ((uint64_t)grid_blocks * kBlock > b.spill_threads) b.wide8_ok = 0;
    return b;
}

void launch_trace_primary(const LaunchCfg& cfg, const BvhDev& bvh, const CameraDev& cam, const ScreenDev& screen,
                          const FrameConst* frames, uint32_t n_slots, float4* hits, uint32_t* work)
{
    const uint32_t chunks = screen.pixels_padded >> 6;
    const bool no_packet = cfg.sw_on(SW_NO_PACKET);  // A/B switch
    if (cfg.stack_entries != 0 && work && bvh.tri_count >= 2 && !no_packet)
    {
        // issue-bound and light on registers: as many waves as fit
        uint32_t gx = (chunks * n_slots + 3) / 4;
        const uint32_t cap = cfg.cu_count ? resident_grid<k_trace_primary_packet<0>>(cfg, ~0u) : cfg.grid_blocks;
        if (gx > cap) gx = cap;
        if (gx == 0) gx = 1;
        hipLaunchKernelGGL(k_trace_primary_packet<0>, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, cam, screen, frames, n_slots, hits, work);
        return;
    }
    uint32_t       gx     = (chunks + 3) / 4;
    if (gx > cfg.grid_blocks) gx = cfg.grid_blocks;
    if (gx == 0) gx = 1;
    const dim3 grid(gx, n_slots);
    BvhDev     b = bvh;
    b.wide8_ok   = 0;  // 2-D grid: no per-thread spill slice
    if (cfg.stack_entries == 0)
        hipLaunchKernelGGL(k_trace_primary<0>, grid, dim3(kBlock), 0, cfg.stream, b, cam, screen, frames, hits);
    else if (cfg.stack_entries <= 32)
        hipLaunchKernelGGL(k_trace_primary<32>, grid, dim3(kBlock), 0, cfg.stream, b, cam, screen, frames, hits);
    else
        hipLaunchKernelGGL(k_trace_primary<64>, grid, dim3(kBlock), 0, cfg.stream, b, cam, screen, frames, hits);
}

void launch_trace_closest(const LaunchCfg& cfg, const BvhDev& bvh, const RayQueue& q, uint32_t max_count, float4* hits)
{
    dim3 grid(queue_grid(cfg, max_count));
    if (cfg.stack_entries == 0)
        hipLaunchKernelGGL(k_trace_closest<0>, grid, dim3(kBlock), 0, cfg.stream, bvh, q, hits);
    else if (cfg.stack_entries <= 32)
    {
        grid.x = resident_grid<k_trace_closest_refill<32>>(cfg, grid.x);
        hipLaunchKernelGGL(k_trace_closest_refill<32>, grid, dim3(kBlock), 0, cfg.stream, bvh, q, hits);
    }
    else
    {
        grid.x = resident_grid<k_trace_closest_refill<64>>(cfg, grid.x);
        hipLaunchKernelGGL(k_trace_closest_refill<64>, grid, dim3(kBlock), 0, cfg.stream, bvh, q, hits);
    }
}

void launch_trace_any(const LaunchCfg& cfg, const BvhDev& bvh, const ShadowQueue& q, uint32_t max_count, float4* target,
                      uint32_t pixels_padded, uint32_t n_slots, uint64_t* guard, uint32_t* work, bool mostly_unoccluded,
                      const FrameConst* frames, float4* code_plane)
{
    assert(!code_plane || (cfg.stack_entries == 0 && !mostly_unoccluded));  // the two kernels below that have the form
    dim3         grid(queue_grid(cfg, max_count));
    const BvhDev bw = for_grid(bvh, grid.x);
    // shadow rays share one direction per frame and retire early: the plain per-chunk kernel beats the refill variant here
    // (8.3 vs 10.5 ms on the 262 k-triangle scene when it was tried)
    const uint32_t pre = (cfg.stack_entries == 0 && !mostly_unoccluded) ? pre_table_bytes(n_slots, bvh.fan_pair_count) : 0u;
    const bool     no_probe = cfg.sw_on(SW_NO_ANY_PROBE);  // A/B switch
    const uint32_t probe    = (uint32_t)cfg.sw_get(SW_ANY_PROBE, CAP_ANY_PROBE);
    if (pre != 0u && work && !no_probe && !cfg.any_no_probe && bvh.fan_pair_count <= kExhaustiveMax / 2)
    {
        // (3 .. 8 workgroups per CU measure the same: what is left is the planes' scattered read-modify-write traffic)
        const uint32_t per_cu = (uint32_t)cfg.sw_get(SW_ANY_BLOCKS, 6);
        uint32_t g = (max_count + kBlock - 1) / kBlock;
        const uint32_t cap = cfg.cu_count ? cfg.cu_count * per_cu : cfg.grid_blocks;
        g = g > cap ? cap : (g ? g : 1u);
        grid = dim3(g);
        const auto kernel = code_plane ? k_trace_any_small<true> : k_trace_any_small<false>;
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), pre, cfg.stream, bw, q, target, pixels_padded, n_slots, guard, work, frames, probe, code_plane);
        return;
    }
#define CAP_LAUNCH_ANY(S, R, ...) \
    hipLaunchKernelGGL((k_trace_any<S, R, ##__VA_ARGS__>), grid, dim3(kBlock), pre, cfg.stream, bw, q, target, pixels_padded, n_slots, guard, work, frames, pre, code_plane)
    if (cfg.stack_entries == 0)
    {
        if (mostly_unoccluded)
            CAP_LAUNCH_ANY(0, true);
        else if (code_plane)
            CAP_LAUNCH_ANY(0, false, true);
        else
            CAP_LAUNCH_ANY(0, false);
    }
    else if (bw.wide8_ok)
    {
        // wide traversal only (its stack continues in the spill slice): the smaller LDS part lets more workgroups be resident.
        // The binary code in this instantiation is never reached -- it has no spill and would drop entries past the LDS part.
        if (mostly_unoccluded) CAP_LAUNCH_ANY((int)kWideLdsEntries, true); else CAP_LAUNCH_ANY((int)kWideLdsEntries, false);
    }
    else if (cfg.stack_entries <= 32)
    {
        if (mostly_unoccluded) CAP_LAUNCH_ANY(32, true); else CAP_LAUNCH_ANY(32, false);
    }
    else
    {
        if (mostly_unoccluded) CAP_LAUNCH_ANY(64, true); else CAP_LAUNCH_ANY(64, false);
    }
#undef CAP_LAUNCH_ANY
}

// What the tree path's two shade stages are to shade_prefetch() and shade_vertex() (cap_shade.h, C)
template <bool FIRST_, bool EXT_, bool FB_ = false>
struct ShadeStageCfg
{
    static constexpr bool FIRST = FIRST_, EXT = EXT_, FB = FB_;
    static constexpr bool CARRY = false, SKY_RMW = true, PROBE = false, TAME = false, LEAN = false, CODE = false, TAB = false, GRAY = false, SKYP = false;
    using Thr = v3;
};

// Stand-alone shade stage (used with the LBVH stack traversal): consumes the hit records of the preceding trace kernel.
template <bool FIRST, bool EXT, bool FB = false>
__global__ __launch_bounds__(kBlock) void k_shade(ShadeArgs a)
{
    using C = ShadeStageCfg<FIRST, EXT, FB>;
    const uint32_t Ppad = a.screen.pixels_padded;
    // FIRST: identity queue, item i of frame slot blockIdx.y is local pixel i.  Otherwise: chunk slots of the input queue.
    const uint32_t chunks   = FIRST ? (Ppad >> 6) : (a.in.class_capacity >> 6) * kQueueClasses;
    uint32_t       n_shaded = 0;
    __shared__ FrameConst lds_frames[kMaxFrameSlots];
    stage_frames(a, lds_frames);
    Stamps st;
    st.start();
    for (uint32_t chunk = wave_global_id(); chunk < chunks; chunk += wave_total())
    {
        uint32_t i, klass;
        bool     active;
        if (FIRST)
        {
            i      = chunk * 64 + (threadIdx.x & 63u);
            active = true;
            klass  = chunk_class(blockIdx.y * (Ppad >> 6) + chunk);  // the path's class for its whole life
        }
        else
            active = queue_chunk(a.in.count, a.in.class_capacity, chunk, threadIdx.x & 63u, i, klass);
        uint32_t pid = 0;
        float4   hit = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
        v3       thr = mk3(1.0f, 1.0f, 1.0f);
        if (active)
        {
            if (FIRST)
            {
                pid = (blockIdx.y << kPidShift) | i;
                hit = a.hits[(size_t)blockIdx.y * Ppad + i];
            }
            else
            {
                const float4 tp = a.in.thr_pid[i];
                thr = mk3(tp.x, tp.y, tp.z), pid = f2u(tp.w);
                hit = a.hits[i];
            }
        }
        const ShadePre pre = shade_prefetch<C>(a, lds_frames, active, pid);
        if constexpr (EXT)
        {
            // the EXT BSDF depends on the incoming direction: the camera ray (bounce 0) or the queue entry's direction
            v3 d = mk3(0.f, 0.f, 1.f);
            if (active)
            {
                if (FIRST)
                {
                    uint32_t x, y;
                    if (local_pixel_to_xy(a.screen, i, x, y)) d = primary_dir(a.cam, a.screen, a.frames[blockIdx.y], x, y);
                }
                else
                {
                    const float4 dq = a.in.dir_tmax[i];
                    d               = mk3(dq.x, dq.y, dq.z);
                }
            }
            shade_vertex_ext<FIRST>(a, a.scene.shade_tris, pre, klass, pid, hit, thr, d, n_shaded);
        }
        else
            shade_vertex<C>(a, a.scene.shade_tris, pre, klass, pid, hit, thr, n_shaded, st);
    }
    flush_stats(a.out.count + (size_t)(wave_global_id() % kQueueClasses) * kCounterStride, n_shaded);
}

// Tree path, bounce 0: the camera rays' packet walk (k_trace_primary_packet) and the shading of the vertices it finds in one
// kernel, like the small-scene path's k_trace_shade<FIRST>: the hit records (32 B per path written and read back) stay in
// registers, and the shade stage's streaming writes -- three planes and two queue entries per path, the HBM-bound part --
// overlap the packet walk's arithmetic of the other waves.  Only the AOV slot's hits are stored (launch_geo_aov reads them).
#ifndef CAP_PS_BLOCKS
#define CAP_PS_BLOCKS 8  // workgroups per CU (residency sweep 4 ... 8: 3.7, 3.25, 3.05, 2.86, 2.81 ms: the packet walk wants waves more than registers)
#endif
template <bool EXT>
__global__ __launch_bounds__(kBlock, CAP_PS_BLOCKS) void k_primary_shade(BvhDev bvh, ShadeArgs a, float4* hits_out)
{
    using C = ShadeStageCfg<true, EXT>;
    __shared__ uint32_t   lds_wstack[(kBlock / 64) * kPacketStack];
    __shared__ FrameConst lds_frames[kMaxFrameSlots];
    stage_frames(a, lds_frames);  // ends with the workgroup barrier
    uint32_t*      wstack   = lds_wstack + (threadIdx.x >> 6) * kPacketStack;
    const uint32_t Ppad     = a.screen.pixels_padded;
    const uint32_t cps      = Ppad >> 6;
    const uint32_t chunks   = cps * a.n_slots;
    const uint32_t my_class = wave_global_id() % kQueueClasses;
    uint32_t       n_shaded = 0;
    uint32_t       grab     = grab_issue(a.work, my_class);
    Stamps         st;
    st.start();
    while (true)
    {
        const uint32_t chunk = class_chunk(grab_value(grab), my_class);  // chunk_class(chunk) == my_class: the paths' class, as k_shade<FIRST> assigns it
        if (chunk >= chunks) break;
        grab = grab_issue(a.work, my_class);
        const uint32_t slot = chunk / cps;  // wave-uniform
        const uint32_t pl   = (chunk - slot * cps) * 64 + (threadIdx.x & 63u);
        uint32_t       x = 0, y = 0;
        const bool     alive = local_pixel_to_xy(a.screen, pl, x, y);
        const Ray      r     = make_ray(mk3(a.cam.position[0], a.cam.position[1], a.cam.position[2]),
                                        alive ? primary_dir(a.cam, a.screen, lds_frames[slot], x, y) : mk3(0.f, 0.f, 1.f), 0.0f, kPrimaryFar);
        float          t, u, v;
        uint32_t       gid;
        traverse_closest_packet(bvh, r, alive, wstack, t, u, v, gid);
        const float4 hit = make_float4(alive ? u : 0.0f, alive ? v : 0.0f, u2f(gid), alive ? t : kPrimaryFar);
        if (slot == a.aov_slot) hits_out[(size_t)slot * Ppad + pl] = hit;
        const uint32_t pid = (slot << kPidShift) | pl;
        const ShadePre pre = shade_prefetch<C>(a, lds_frames, true, pid);
        if constexpr (EXT)
            shade_vertex_ext<true>(a, a.scene.shade_tris, pre, my_class, pid, hit, mk3(1.0f, 1.0f, 1.0f), r.d, n_shaded);
        else
            shade_vertex<C>(a, a.scene.shade_tris, pre, my_class, pid, hit, mk3(1.0f, 1.0f, 1.0f), n_shaded, st);
    }
    flush_stats(a.out.count + (size_t)my_class * kCounterStride, n_shaded);
}

bool launch_primary_shade(const LaunchCfg& cfg, const BvhDev& bvh, const ShadeArgs& args, float4* hits, bool ext)
{
    const bool off = cfg.sw_on(SW_NO_PRIMARY_FUSE) || cfg.sw_on(SW_NO_PACKET);  // A/B switches
    if (off || cfg.stack_entries == 0 || !args.work || bvh.tri_count < 2 || !cfg.cu_count) return false;
    const uint32_t chunks = (args.screen.pixels_padded >> 6) * args.n_slots;
    uint32_t       gx     = (chunks + 3) / 4;
    const uint32_t cap    = ext ? resident_grid<k_primary_shade<true>>(cfg, ~0u) : resident_grid<k_primary_shade<false>>(cfg, ~0u);
    if (gx > cap) gx = cap;
    if (gx == 0) gx = 1;
    if (ext)
        hipLaunchKernelGGL(k_primary_shade<true>, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, args, hits);
    else
        hipLaunchKernelGGL(k_primary_shade<false>, dim3(gx), dim3(kBlock), 0, cfg.stream, bvh, args, hits);
    return true;
}

// bounce >= 1.  Static chunk assignment: the grid must be resident at once (resident_grid())
template <bool EXT, bool FB>
static void launch_shade_next(const LaunchCfg& cfg, const ShadeArgs& args)
{
    const uint32_t g = resident_grid<k_shade<false, EXT, FB>>(cfg, queue_grid(cfg, args.max_count));
    hipLaunchKernelGGL((k_shade<false, EXT, FB>), dim3(g), dim3(kBlock), 0, cfg.stream, args);
}

void launch_shade(const LaunchCfg& cfg, const ShadeArgs& args, bool ext, bool feedback)
{
    if (args.bounce == 0)
    {
        const uint32_t chunks = args.screen.pixels_padded >> 6;
        uint32_t       gx     = (chunks + 3) / 4;
        if (gx > cfg.grid_blocks) gx = cfg.grid_blocks;
        if (gx == 0) gx = 1;
        if (ext)
            hipLaunchKernelGGL((k_shade<true, true>), dim3(gx, args.n_slots), dim3(kBlock), 0, cfg.stream, args);
        else
            hipLaunchKernelGGL((k_shade<true, false>), dim3(gx, args.n_slots), dim3(kBlock), 0, cfg.stream, args);
    }
    else if (ext)
        launch_shade_next<true, false>(cfg, args);
    else if (feedback)
        launch_shade_next<false, true>(cfg, args);
    else
        launch_shade_next<false, false>(cfg, args);
}

// Ray queries of caller-supplied rays (cap_trace_rays / cap_trace_occlusion) on the binary tree, one lane per ray: every ray where the
// compressed 8-wide view is not used (CAP_NO_WIDE8, a tree deeper than the wide kernels' stacks), and the rays the wide query kernels
// passed on (query.hip: origins beyond the wide box test's error budget).  traverse_closest / traverse_any as k_trace_primary runs them
// (wide8_ok cleared: the grid need not fit the spill area), so the records are the same bits as the wide kernels' and the render's.
template <int STACK, bool ANY>
__global__ __launch_bounds__(kBlock, stack_residency(STACK)) void k_query_binary(BvhDev bvh, QueryArgs q, uint32_t deferred)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    const uint32_t      count = deferred ? q.work[kCounterStride] : q.n;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < count; j += gridDim.x * kBlock)
    {
        const uint32_t i = deferred ? q.defer[j] : j;
        const float4   a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];
        const bool     ok = query_ray_ok(a, b);
        const Ray      r  = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
        if (ANY)
            static_cast<uint32_t*>(q.out)[i] = (ok && traverse_any<STACK>(bvh, r, stack)) ? 1u : 0u;
        else
        {
            float    t = b.w, u = 0.0f, v = 0.0f;
            uint32_t gid = kInvalidId;
            if (ok) traverse_closest<STACK>(bvh, r, stack, t, u, v, gid);
            static_cast<float4*>(q.out)[i] = make_float4(t, u, v, u2f(gid));
        }
    }
}

void launch_query_binary(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, bool any, bool deferred)
{
    BvhDev   b    = bvh;
    b.wide8_ok    = 0;
    uint32_t want = (q.n + kBlock - 1) / kBlock;
    // (deferred: the count is on the device and is normally small -- one workgroup per CU at most)
    if (deferred && cfg.cu_count && want > cfg.cu_count) want = cfg.cu_count;
    if (want == 0) want = 1;
#define CAP_LAUNCH_QUERY(S, A) \
    hipLaunchKernelGGL((k_query_binary<S, A>), dim3(resident_grid<k_query_binary<S, A>>(cfg, want)), dim3(kBlock), 0, cfg.stream, b, q, deferred ? 1u : 0u)
    if (cfg.stack_entries <= 32)
    {
        if (any) CAP_LAUNCH_QUERY(32, true); else CAP_LAUNCH_QUERY(32, false);
    }
    else
    {
        if (any) CAP_LAUNCH_QUERY(64, true); else CAP_LAUNCH_QUERY(64, false);
    }
#undef CAP_LAUNCH_QUERY
}
}  // namespace cap
