// sweep.hip — sphere sweep queries (cap_sweep_spheres) on the binary tree, gfx950: for every sweep (o, r, d, tmax) the triangle minimal in
// (t, triangle) among those the sphere of radius r centred at c(t) = o + t d touches for some t in [0, tmax], by the per-triangle function
// of include/capsaicin_hip.h ("sphere sweep queries"): (A) the closest-point cascade at o, (B) the smallest entry time of the ray (o, d)
// into the seven pieces of the triangle's r-offset surface, polished by up to two Newton steps on the distance where rounding left the
// centre outside, (C) the cascade again at c = o + t d, which alone accepts the candidate.
//
// One lane per sweep, a grid-stride loop over the chunk, k_closest_points' shape: a node fetch yields both child boxes, each is tested
// with a slab test of the ray against the box grown by the sweep's prune radius R over [0, best]; the nearer entry is visited first and
// the other child pushed with its entry time, 8-byte LDS entries strided by kBlock.  A popped entry is tested again against the bound as
// it stands then.  The lane keeps (best t, best id) only and computes the winner's record again at the end from tris_by_id.
//
// Pruning (DESIGN.md "Sphere sweep queries" has the argument): R = fl(r + 128 eps (|o|_inf + M + r)), M the largest coordinate
// magnitude of the scene bounds, is fixed per sweep: it holds the acceptance tolerance, the closest-point argument's own bound, the
// distance between the computed centre c and the exact line point, and the roundings of the box's two subtractions.  What is left of
// the slab test's roundings is relative and is taken by the factor (1 + 8 eps) on the far side, plus the smallest normal number for a
// product that underflows.  No test is strict: a box whose entry time equals `best` is opened, its lower id may win.
#include "cap_closest.h"
#include "cap_kernels.h"
#include "cap_near.h"
#include "cap_query_walk.h"

namespace cap
{
namespace
{
__device__ __forceinline__ bool sweep_ok(const float4 q0, const float4 q1)
{
    const float inf = __builtin_inff();
    return fabsf(q0.x) < inf && fabsf(q0.y) < inf && fabsf(q0.z) < inf && fabsf(q1.x) < inf && fabsf(q1.y) < inf && fabsf(q1.z) < inf && q0.w >= 0.f &&
           q1.w >= 0.f;  // (a NaN fails its comparison)
}

// (sweep_padded, SweepRay and sweep_slab, the walk's time comparisons and its box test, are in cap_near.h: the debug entry runs them too)
template <int STACK>
__device__ __forceinline__ bool sweep_node_step(const BvhDev& bvh, const SweepRay& s, float best, uint2* stack, int& node, int& sp)
{
    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
    float        t0, t1;
    const bool   k0 = sweep_slab(s, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, best, t0);
    const bool   k1 = sweep_slab(s, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, best, t1);
    const int    c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
    if (k0 && k1)
    {
        const bool swap = t1 < t0;
        if (sp < STACK) stack[(sp++) * kBlock] = make_uint2(f2u(swap ? t0 : t1), (uint32_t)(swap ? c0 : c1));
        node = swap ? c1 : c0;
        return true;
    }
    if (k0 || k1)
    {
        node = k0 ? c0 : c1;
        return true;
    }
    return false;
}

// The next stack entry whose entry time still passes `best` as it stands now; false: the stack is empty
__device__ __forceinline__ bool sweep_pop(uint2* stack, int& sp, float best, int& node)
{
    const float far = sweep_padded(best);
    while (sp > 0)
    {
        const uint2 e = stack[(--sp) * kBlock];
        if (u2f(e.x) <= far)
        {
            node = (int)e.y;
            return true;
        }
    }
    return false;
}

// ---- part (B) of the contract: the candidate time of one triangle ----
// The smaller root of  a t^2 + 2 b t + c = 0, if it is real and lies in (0, tmax]; +inf otherwise (a NaN fails the comparisons)
__device__ __forceinline__ float sweep_root(float a, float b, float c, float tmax)
{
    const float disc = b * b - a * c;
    const float t    = (-b - sqrtf(disc)) / a;
    return (a > 0.f && t > 0.f && t <= tmax) ? t : __builtin_inff();
}
// the sphere of radius r (r2 = r r) around the vertex at m = o - vertex
__device__ __forceinline__ float sweep_vertex(float mx, float my, float mz, float dx, float dy, float dz, float dd, float r2, float tmax)
{
    const float md = dot_c(mx, my, mz, dx, dy, dz), mm = dot_c(mx, my, mz, mx, my, mz);
    return sweep_root(dd, md, mm - r2, tmax);
}
// the cylinder of radius r around the edge from the vertex at m = o - vertex along e, accepted with the axis parameter in [0, 1]
__device__ __forceinline__ float sweep_edge(float mx, float my, float mz, float ex, float ey, float ez, float dx, float dy, float dz, float dd, float r2,
                                            float tmax)
{
    const float ee = dot_c(ex, ey, ez, ex, ey, ez), me = dot_c(mx, my, mz, ex, ey, ez), de = dot_c(dx, dy, dz, ex, ey, ez);
    const float md = dot_c(mx, my, mz, dx, dy, dz), mm = dot_c(mx, my, mz, mx, my, mz);
    const float t  = sweep_root(ee * dd - de * de, ee * md - de * me, ee * (mm - r2) - me * me, tmax);
    const float s  = me + t * de;
    return (s >= 0.f && s <= ee) ? t : __builtin_inff();
}

__device__ __forceinline__ float sweep_candidate(const float4 t0, const float4 t1, const float4 t2, const float4 q0, const float4 q1, float r2, float dd)
{
    const float inf = __builtin_inff();
    const float e1x = t0.w, e1y = t1.x, e1z = t1.y, e2x = t1.z, e2y = t1.w, e2z = t2.x;
    const float ox = q0.x, oy = q0.y, oz = q0.z, r = q0.w, dx = q1.x, dy = q1.y, dz = q1.z, tmax = q1.w;
    const float m0x = ox - t0.x, m0y = oy - t0.y, m0z = oz - t0.z;
    // the offset plane on o's side
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float nn = dot_c(nx, ny, nz, nx, ny, nz), h = dot_c(nx, ny, nz, m0x, m0y, m0z), nd = dot_c(nx, ny, nz, dx, dy, dz);
    const float num = fabsf(h) - r * sqrtf(nn), den = h >= 0.f ? -nd : nd;
    float       tc = inf;
    {
        const float t  = num / den;
        const float wx = (ox + t * dx) - t0.x, wy = (oy + t * dy) - t0.y, wz = (oz + t * dz) - t0.z;
        const float a  = dot_c(wy * e2z - wz * e2y, wz * e2x - wx * e2z, wx * e2y - wy * e2x, nx, ny, nz);
        const float b  = dot_c(e1y * wz - e1z * wy, e1z * wx - e1x * wz, e1x * wy - e1y * wx, nx, ny, nz);
        if (den > 0.f && t > 0.f && t <= tmax && a >= 0.f && b >= 0.f && a + b <= nn) tc = t;
    }
    // the three edge cylinders: v0 v1, v0 v2, v1 v2
    const float m1x = ox - (t0.x + e1x), m1y = oy - (t0.y + e1y), m1z = oz - (t0.z + e1z);
    const float m2x = ox - (t0.x + e2x), m2y = oy - (t0.y + e2y), m2z = oz - (t0.z + e2z);
    tc = fminf(tc, sweep_edge(m0x, m0y, m0z, e1x, e1y, e1z, dx, dy, dz, dd, r2, tmax));
    tc = fminf(tc, sweep_edge(m0x, m0y, m0z, e2x, e2y, e2z, dx, dy, dz, dd, r2, tmax));
    tc = fminf(tc, sweep_edge(m1x, m1y, m1z, e2x - e1x, e2y - e1y, e2z - e1z, dx, dy, dz, dd, r2, tmax));
    // the three vertex spheres
    tc = fminf(tc, sweep_vertex(m0x, m0y, m0z, dx, dy, dz, dd, r2, tmax));
    tc = fminf(tc, sweep_vertex(m1x, m1y, m1z, dx, dy, dz, dd, r2, tmax));
    tc = fminf(tc, sweep_vertex(m2x, m2y, m2z, dx, dy, dz, dd, r2, tmax));
    return tc;
}

// Parts (A), (B) with its polish and (C) for one triangle record (t0, t1, t2) -- the stored one, or the world record of an instanced
// triangle: the triangle's contact time, or a NaN where it has none or cannot beat `best` (wins_tie: it would win a tie at `best`).
// The caller's comparison  t < best || (t == best && wins_tie)  then fails by itself.  It is the leaf body of k_sweep_spheres below,
// operation for operation; that kernel keeps its own copy of the text, because calling this function from it cost it a register (70
// VGPRs for 69, tools/kernel_regs.sh), and its code is held to what it was.
__device__ __forceinline__ float sweep_contact(const float4 t0, const float4 t1, const float4 t2, const float4 q0, const float4 q1, float r2, float r2k,
                                               float dd, float best, bool wins_tie)
{
    const float none = __builtin_nanf("");
    // (A) a start overlap is a contact at t = 0
    if (closest_dist2(t0, t1, t2, q0.x, q0.y, q0.z) <= r2) return 0.f;
    // (B) the candidate, compared with best before (C) is paid for; best == 0 admits no t > 0
    if (!(best > 0.f)) return none;
    float t = sweep_candidate(t0, t1, t2, q0, q1, r2, dd);
    if (!(t < best || (t == best && wins_tie))) return none;
    // (C) the centre at the candidate time touches the triangle by the closest-point function itself; (B)'s polish:
    // a centre that rounding left outside is moved inwards by a Newton step on the distance plus the nudge, twice at the most
#pragma unroll 1
    for (int k = 0; k < 3; ++k)
    {
        const float        cx = q0.x + t * q1.x, cy = q0.y + t * q1.y, cz = q0.z + t * q1.z;
        const ClosestPoint c  = closest_record(t0, t1, t2, cx, cy, cz);
        if (c.d2 <= r2k) return t;
        if (k == 2) break;
        const float dist = sqrtf(c.d2);
        const float rate = -dot_c(cx - c.x, cy - c.y, cz - c.z, q1.x, q1.y, q1.z);
        const float size = fmaxf(fmaxf(fmaxf(fabsf(cx), fabsf(cy)), fabsf(cz)), fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fabsf(c.z))) + q0.w;
        const float tn   = t + (((dist - q0.w) + kSweepNudge * size) * dist) / rate;
        if (!(rate > 0.f && tn <= q1.w)) break;
        t = tn;
    }
    return none;
}

__device__ __forceinline__ void sweep_write_miss(float4* slot, float t)
{
    slot[0] = make_float4(0.f, 0.f, 0.f, t);
    slot[1] = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
}

// Workgroups per CU: the stack is 8 B x STACK x kBlock of the CU's 160 KB of LDS, as k_closest_points'.  Every instantiation uses 69
// VGPRs and no scratch (tools/kernel_regs.sh; the table is in DESIGN.md), within the 96 that five workgroups of the 16-entry class leave.
constexpr int sweep_blocks(int STACK) { return STACK <= 16 ? 5 : STACK <= 24 ? 3 : STACK <= 32 ? 2 : 1; }

// FILTER: the mesh-mask table (RayFilter::tri_mask by global id), read before the record is fetched.
template <int STACK, bool FILTER>
__global__ __launch_bounds__(kBlock, sweep_blocks(STACK)) void k_sweep_spheres(BvhDev bvh, SweepArgs a, RayFilter f)
{
    __shared__ uint2 lds_stack[STACK * kBlock];
    uint2* const     stack = lds_stack + threadIdx.x;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock)
    {
        const float4 q0 = a.sweeps[2 * (size_t)i], q1 = a.sweeps[2 * (size_t)i + 1];
        if (!sweep_ok(q0, q1))
        {
            sweep_write_miss(a.out + 2 * (size_t)i, 0.f);
            continue;
        }
        const float r2 = q0.w * q0.w, r2k = r2 * kSweepAccept;
        const float dd = dot_c(q1.x, q1.y, q1.z, q1.x, q1.y, q1.z);
        // (dd == 0: part (A) only, nothing beyond t = 0 can be an answer)
        float       best     = dd == 0.f ? 0.f : q1.w;
        uint32_t    best_gid = kInvalidId;
        const float omax     = fmaxf(fabsf(q0.x), fmaxf(fabsf(q0.y), fabsf(q0.z)));
        SweepRay    s{q0.x, q0.y, q0.z, 1.0f / q1.x, 1.0f / q1.y, 1.0f / q1.z, q0.w + kSweepSlackScale * ((omax + a.mag) + q0.w)};
        int         node = bvh.root, sp = 0;
        while (bvh.tri_count != 0u)
        {
            if (node >= 0)
            {
                if (sweep_node_step<STACK>(bvh, s, best, stack, node, sp)) continue;
            }
            else
            {
                const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                for (uint32_t leaf = first; leaf <= last; ++leaf)
                {
                    const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                    if constexpr (FILTER)
                        if ((f.tri_mask[gid] & f.mask) == 0u) continue;
                    // (from here to the comparison below: sweep_contact above, word for word -- change both or neither)
                    const float4 t0 = bvh.tris[4 * (size_t)leaf + 0], t1 = bvh.tris[4 * (size_t)leaf + 1], t2 = bvh.tris[4 * (size_t)leaf + 2];
                    // (A) a start overlap is a contact at t = 0
                    float t = 0.f;
                    if (!(closest_dist2(t0, t1, t2, q0.x, q0.y, q0.z) <= r2))
                    {
                        // (B) the candidate, compared with best before (C) is paid for; best == 0 admits no t > 0
                        if (!(best > 0.f)) continue;
                        t = sweep_candidate(t0, t1, t2, q0, q1, r2, dd);
                        if (!(t < best || (t == best && gid < best_gid))) continue;
                        // (C) the centre at the candidate time touches the triangle by the closest-point function itself; (B)'s polish:
                        // a centre that rounding left outside is moved inwards by a Newton step on the distance plus the nudge, twice at the most
                        bool touches = false;
#pragma unroll 1
                        for (int k = 0; k < 3; ++k)
                        {
                            const float        cx = q0.x + t * q1.x, cy = q0.y + t * q1.y, cz = q0.z + t * q1.z;
                            const ClosestPoint c  = closest_record(t0, t1, t2, cx, cy, cz);
                            touches               = c.d2 <= r2k;
                            if (touches || k == 2) break;
                            const float dist = sqrtf(c.d2);
                            const float rate = -dot_c(cx - c.x, cy - c.y, cz - c.z, q1.x, q1.y, q1.z);
                            const float size = fmaxf(fmaxf(fmaxf(fabsf(cx), fabsf(cy)), fabsf(cz)), fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fabsf(c.z))) + q0.w;
                            const float tn   = t + (((dist - q0.w) + kSweepNudge * size) * dist) / rate;
                            if (!(rate > 0.f && tn <= q1.w)) break;
                            t = tn;
                        }
                        if (!touches) continue;
                    }
                    if (t < best || (t == best && gid < best_gid)) best = t, best_gid = gid;
                }
            }
            if (!sweep_pop(stack, sp, best, node)) break;
        }
        if (best_gid == kInvalidId)
        {
            sweep_write_miss(a.out + 2 * (size_t)i, q1.w);
            continue;
        }
        // (at t = 0 the record is the cascade's at o itself, not at fl(o + fl(0 d)), which may differ in the sign of a zero)
        const float4*      rec = bvh.tris_by_id + 4 * (size_t)best_gid;
        const bool         at0 = best == 0.f;
        const ClosestPoint c   = closest_record(rec[0], rec[1], rec[2], at0 ? q0.x : q0.x + best * q1.x, at0 ? q0.y : q0.y + best * q1.y,
                                                at0 ? q0.z : q0.z + best * q1.z);
        a.out[2 * (size_t)i]     = make_float4(c.x, c.y, c.z, best);
        a.out[2 * (size_t)i + 1] = make_float4(c.u, c.v, u2f(best_gid), u2f(c.feature));
    }
}
// ---- over the instance table (cap_sweep_instances) ----
// For every WORLD-space sweep the pair (instance, triangle) minimal in (t, instance, triangle), the per-pair function being
// sweep_contact above, unchanged, on the world record of cap_closest_instances (world_record, from M as the caller gave it).  One loop
// with three kinds of step, as k_closest_inst (point_query.hip), so that the lanes of a wave that are at the top level advance while
// others are inside an instance.  The prune stays in world space at both levels: at the top the stored world boxes, below an instance
// every child box of the object's tree mapped to its world box under M (cap_near.h overlap_world_box), each given sweep_slab against
// the world ray over [0, best] and grown by R_i = sweep_prune_radius(r, |o|_inf, Xw_i) -- the table's largest Xw at the top level.  No
// object-space ray is walked: the rounding of W d would be multiplied by t, and tmax = +inf is legal.  DESIGN.md "Sphere sweep queries
// over instances" has the argument.  The top level's ordering key is the entry time; every test is <=, so a box, instance or triangle
// entered exactly at `best` is opened and the lower (instance, triangle) wins.
__device__ __forceinline__ TopWalk sweep_top_step(const TlasDev& tl, const uint32_t* lds_off, const SweepRay& s, float best, TopWalk t)
{
    const float4* c = tl.tlas + 2 * (size_t)(lds_off[t.level - 1u] + 2u * t.idx);
    const float4  lo0 = c[0], hi0 = c[1], lo1 = c[2], hi1 = c[3];
    float         d0, d1;
    const bool    k0 = sweep_slab(s, lo0.x, lo0.y, lo0.z, hi0.x, hi0.y, hi0.z, best, d0);
    const bool    k1 = sweep_slab(s, lo1.x, lo1.y, lo1.z, hi1.x, hi1.y, hi1.z, best, d1);
    // (a record with k < 0 holds nothing: an inert instance or the padding of a level)
    const bool h0 = lo0.w >= 0.0f && k0, h1 = lo1.w >= 0.0f && k1;
    return top_advance(t, h0, h1, h0 && h1 && d1 < d0, f2u(hi0.w), f2u(hi1.w), d0, d1);  // the earlier entry first
}

// An inner node of the object's tree: sweep_node_step with both child boxes mapped to world space first.  m: the 12 words of M.
template <int STACK>
__device__ __forceinline__ bool sweep_world_node_step(const BvhDev& bvh, const float m[12], const SweepRay& s, float best, uint2* stack, int& node, int& sp)
{
    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
    float        lo0[3], hi0[3], lo1[3], hi1[3], t0, t1;
    overlap_world_box(m, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, lo0, hi0);
    overlap_world_box(m, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, lo1, hi1);
    const bool k0 = sweep_slab(s, lo0[0], lo0[1], lo0[2], hi0[0], hi0[1], hi0[2], best, t0);
    const bool k1 = sweep_slab(s, lo1[0], lo1[1], lo1[2], hi1[0], hi1[1], hi1[2], best, t1);
    const int  c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
    if (k0 && k1)
    {
        const bool swap = t1 < t0;
        if (sp < STACK) stack[(sp++) * kBlock] = make_uint2(f2u(swap ? t0 : t1), (uint32_t)(swap ? c0 : c1));
        node = swap ? c1 : c0;
        return true;
    }
    if (k0 || k1)
    {
        node = k0 ? c0 : c1;
        return true;
    }
    return false;
}

// Workgroups per CU: the stack's LDS and the 104 bytes of level offsets, as closest_inst_blocks (point_query.hip).  Registers
// (tools/kernel_regs.sh; the table is in DESIGN.md "Sphere sweep queries over instances").
constexpr int sweep_inst_blocks(int STACK) { return STACK <= 16 ? 4 : STACK <= 24 ? 3 : STACK <= 32 ? 2 : 1; }

// FILTER: a mesh-mask table is installed (f.tri_mask by global id); the instance's own mask is tested either way, at entry.
template <int STACK, bool FILTER>
__global__ __launch_bounds__(kBlock, sweep_inst_blocks(STACK)) void k_sweep_inst(BvhDev bvh, SweepInstArgs ia, TlasDev tl, RayFilter f)
{
    __shared__ uint2    lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint2* const        stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const SweepArgs& a      = ia.a;
    const float      xw_all = u2f(ia.xw_max[0]);  // the largest Xw of the table: the top level's prune radius holds for every instance
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.n; j += gridDim.x * kBlock)
    {
        const float4 q0 = a.sweeps[2 * (size_t)j], q1 = a.sweeps[2 * (size_t)j + 1];
        if (!sweep_ok(q0, q1))
        {
            sweep_write_miss(a.out + 2 * (size_t)j, 0.f);
            if (ia.inst_out) ia.inst_out[j] = kInvalidId;
            continue;
        }
        const float r2 = q0.w * q0.w, r2k = r2 * kSweepAccept;
        const float dd = dot_c(q1.x, q1.y, q1.z, q1.x, q1.y, q1.z);
        // (dd == 0: part (A) only, nothing beyond t = 0 can be an answer)
        float       best     = dd == 0.f ? 0.f : q1.w;
        uint32_t    best_gid = kInvalidId, best_inst = kInvalidId;
        const float omax     = fmaxf(fabsf(q0.x), fmaxf(fabsf(q0.y), fabsf(q0.z)));
        SweepRay    s{q0.x, q0.y, q0.z, 1.0f / q1.x, 1.0f / q1.y, 1.0f / q1.z, 0.f};
        const float grow_top = sweep_prune_radius(q0.w, omax, xw_all);
        TopWalk     t        = top_start(tl);
        // bottom level: the instance being walked, its M and its own prune radius
        bool     in_blas = false;
        float    m[12]   = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float    grow    = 0.f;
        uint32_t inst = 0u, imask = 0u;
        int      node = 0, sp = 0;
        bool     walk = bvh.tri_count != 0u;
        while (walk)
        {
            if (in_blas)
            {
                s.grow = grow;
                if (node >= 0)
                {
                    if (sweep_world_node_step<STACK>(bvh, m, s, best, stack, node, sp)) continue;
                }
                else
                {
                    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                    for (uint32_t leaf = first; leaf <= last; ++leaf)
                    {
                        const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                        if constexpr (FILTER)
                            if ((f.tri_mask[gid] & imask) == 0u) continue;
                        const WorldRecord w = world_record(make_float4(m[0], m[1], m[2], m[3]), make_float4(m[4], m[5], m[6], m[7]),
                                                           make_float4(m[8], m[9], m[10], m[11]), bvh.tris[4 * (size_t)leaf + 0],
                                                           bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2]);
                        const bool  wins = inst < best_inst || (inst == best_inst && gid < best_gid);
                        const float tc   = sweep_contact(w.t0, w.t1, w.t2, q0, q1, r2, r2k, dd, best, wins);
                        if (tc < best || (tc == best && wins)) best = tc, best_inst = inst, best_gid = gid;
                    }
                }
                in_blas = sweep_pop(stack, sp, best, node);
                continue;
            }
            if (t.todo0 != kInvalidId)
            {
                // the head of the queue, if its entry time still passes against the bound as it is now: its mask joined with the
                // call's (0 for an inert instance; the mesh byte joins it per triangle), then M, the instance's prune radius and
                // the root of the object's tree
                inst             = t.todo0;
                const bool still = t.todo0_d <= sweep_padded(best);
                t                = top_pop(t);
                if (!still) continue;
                const float4 w3 = tl.rec[4 * (size_t)inst + 3];
                imask           = f2u(w3.x) & f.mask;
                if (imask == 0u) continue;
                const float4 m0 = ia.descs[4 * (size_t)inst], m1 = ia.descs[4 * (size_t)inst + 1], m2 = ia.descs[4 * (size_t)inst + 2];
                m[0] = m0.x, m[1] = m0.y, m[2] = m0.z, m[3] = m0.w, m[4] = m1.x, m[5] = m1.y, m[6] = m1.z, m[7] = m1.w;
                m[8] = m2.x, m[9] = m2.y, m[10] = m2.z, m[11] = m2.w;
                grow = sweep_prune_radius(q0.w, omax, ia.near[inst].y);  // (g, Xw): g is not read, the test stays in world space
                node = (int)f2u(w3.y), sp = 0, in_blas = true;
                continue;
            }
            if (t.done) break;
            s.grow = grow_top;
            t      = sweep_top_step(tl, lds_off, s, best, t);
        }
        if (ia.inst_out) ia.inst_out[j] = best_inst;
        if (best_gid == kInvalidId)
        {
            sweep_write_miss(a.out + 2 * (size_t)j, q1.w);
            continue;
        }
        // the winner's world record again, from the records in id order and the instance's transform, the same operations
        const float4*      rec = bvh.tris_by_id + 4 * (size_t)best_gid;
        const float4*      md  = ia.descs + 4 * (size_t)best_inst;
        const WorldRecord  w   = world_record(md[0], md[1], md[2], rec[0], rec[1], rec[2]);
        const bool         at0 = best == 0.f;
        const ClosestPoint c   = closest_record(w.t0, w.t1, w.t2, at0 ? q0.x : q0.x + best * q1.x, at0 ? q0.y : q0.y + best * q1.y,
                                                at0 ? q0.z : q0.z + best * q1.z);
        a.out[2 * (size_t)j]     = make_float4(c.x, c.y, c.z, best);
        a.out[2 * (size_t)j + 1] = make_float4(c.u, c.v, u2f(best_gid), u2f(c.feature));
    }
}
}  // namespace

void launch_sweep_instances(const LaunchCfg& cfg, const BvhDev& bvh, const SweepInstArgs& a, const TlasDev& tl, const RayFilter& f, uint32_t depth)
{
    // (depth: of the deepest bottom-level tree)
    with_stack_class(depth, [&](auto S) {
        with_flag(f.tri_mask != nullptr, [&](auto FILTER) { launch_points<k_sweep_inst<decltype(S)::value, decltype(FILTER)::value>>(cfg, a.a.n, bvh, a, tl, f); });
    });
}

void launch_sweep_spheres(const LaunchCfg& cfg, const BvhDev& bvh, const SweepArgs& a, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const RayFilter rf = f ? *f : RayFilter{};
    with_stack_class(depth, [&](auto S) {
        with_flag(f && f->tri_mask, [&](auto FILTER) { launch_points<k_sweep_spheres<decltype(S)::value, decltype(FILTER)::value>>(cfg, a.n, b, a, rf); });
    });
}
}  // namespace cap
