// point_query.hip — closest-point queries (cap_closest_points) on the binary tree, gfx950: for every point the triangle minimal in
// (dist2, triangle) among those within the radius, by the per-triangle function of include/capsaicin_hip.h ("closest-point queries").
//
// One lane per point, a grid-stride loop over the chunk as in k_query_binary_multi.  The walk is ordered and pruned by the squared
// distance from the point to a child's box: a node fetch yields both child boxes, the nearer child is entered first and the other one
// pushed if it survives the prune.  A stack entry is (box distance, child) in LDS, 8 bytes strided by kBlock: a popped entry is tested
// again against the bound as it stands then with one LDS read.  (The alternative, 4-byte entries (parent, slot) and the box distance
// computed again from the parent, halves the LDS but pays a dependent 64-byte fetch for every pop, and most pops are rejects: after the
// first leaf the bound has shrunk below almost everything the first descent pushed.  Registers are the same, see DESIGN.md.)
//
// Pruning (DESIGN.md "Closest-point queries" has the argument): a box is skipped only when its computed squared distance exceeds
//   bound2 = fl-up((sqrt(best) (1 + 16 eps) + slack)^2),  slack = 64 eps max|scene coordinate|,
// which no triangle inside it can reach with a contract dist2 <= best.  best starts at r2 with the id ~0, so `dist2 <= r2` and the
// tie rule are one comparison.  bound2 > best unless both are 0 or inf, and the test is a strict >: a subtree at exactly the best
// distance is opened, its lower id may win.
//
// The multi form (cap_closest_points_multi, k_closest_points_multi) is the same walk with the sorted list HitList<K> of cap_hit_list.h
// in the place of the single best pair; "best" above reads "k-th best", slot K - 1 of the list.
#include "cap_hit_list.h"
#include "cap_kernels.h"

namespace cap
{
namespace
{
// dot of the contract: no fused multiply-add (the build has -ffp-contract=off; fmaf is nowhere written)
__device__ __forceinline__ float dot_c(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

struct ClosestPoint
{
    float    x, y, z, d2, u, v;
    uint32_t feature;
};

// (u, v, feature) of the cascade for the record (v0, e1, e2) and ap = p - v0
__device__ __forceinline__ void closest_uv(const float4 t0, const float4 t1, const float4 t2, float apx, float apy, float apz, float& u, float& v,
                                           uint32_t& feature)
{
    const float e1x = t0.w, e1y = t1.x, e1z = t1.y, e2x = t1.z, e2y = t1.w, e2z = t2.x;
    const float d1 = dot_c(e1x, e1y, e1z, apx, apy, apz), d2 = dot_c(e2x, e2y, e2z, apx, apy, apz);
    if (d1 <= 0.f && d2 <= 0.f)
    {
        u = 0.f, v = 0.f, feature = 4u;
        return;
    }
    const float bpx = apx - e1x, bpy = apy - e1y, bpz = apz - e1z;
    const float d3 = dot_c(e1x, e1y, e1z, bpx, bpy, bpz), d4 = dot_c(e2x, e2y, e2z, bpx, bpy, bpz);
    if (d3 >= 0.f && d4 <= d3)
    {
        u = 1.f, v = 0.f, feature = 5u;
        return;
    }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f)
    {
        u = d1 / (d1 - d3), v = 0.f, feature = 1u;
        return;
    }
    const float cpx = apx - e2x, cpy = apy - e2y, cpz = apz - e2z;
    const float d5 = dot_c(e1x, e1y, e1z, cpx, cpy, cpz), d6 = dot_c(e2x, e2y, e2z, cpx, cpy, cpz);
    if (d6 >= 0.f && d5 <= d6)
    {
        u = 0.f, v = 1.f, feature = 6u;
        return;
    }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f)
    {
        u = 0.f, v = d2 / (d2 - d6), feature = 3u;
        return;
    }
    const float va = d3 * d6 - d5 * d4;
    const float a43 = d4 - d3, a56 = d5 - d6;
    if (va <= 0.f && a43 >= 0.f && a56 >= 0.f)
    {
        const float w = a43 / (a43 + a56);
        u = 1.f - w, v = w, feature = 2u;
        return;
    }
    const float s = (va + vb) + vc;
    u = vb / s, v = vc / s, feature = 0u;
}

// dist2 of the contract alone: what the walk compares
__device__ __forceinline__ float closest_dist2(const float4 t0, const float4 t1, const float4 t2, float px, float py, float pz)
{
    const float apx = px - t0.x, apy = py - t0.y, apz = pz - t0.z;
    float       u, v;
    uint32_t    feature;
    closest_uv(t0, t1, t2, apx, apy, apz, u, v, feature);
    const float dx = apx - (t0.w * u + t1.z * v), dy = apy - (t1.x * u + t1.w * v), dz = apz - (t1.y * u + t2.x * v);
    return dot_c(dx, dy, dz, dx, dy, dz);
}

// the whole record, for the winner (the same operations: the same dist2 bits)
__device__ __forceinline__ ClosestPoint closest_record(const float4 t0, const float4 t1, const float4 t2, float px, float py, float pz)
{
    const float  apx = px - t0.x, apy = py - t0.y, apz = pz - t0.z;
    ClosestPoint c;
    closest_uv(t0, t1, t2, apx, apy, apz, c.u, c.v, c.feature);
    const float mx = t0.w * c.u + t1.z * c.v, my = t1.x * c.u + t1.w * c.v, mz = t1.y * c.u + t2.x * c.v;
    const float dx = apx - mx, dy = apy - my, dz = apz - mz;
    c.d2 = dot_c(dx, dy, dz, dx, dy, dz);
    c.x = t0.x + mx, c.y = t0.y + my, c.z = t0.z + mz;
    return c;
}

// squared distance from p to the box [lo, hi], 0 inside
__device__ __forceinline__ float box_dist2(float px, float py, float pz, float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    const float dx = fmaxf(fmaxf(lox - px, px - hix), 0.f), dy = fmaxf(fmaxf(loy - py, py - hiy), 0.f), dz = fmaxf(fmaxf(loz - pz, pz - hiz), 0.f);
    return (dx * dx + dy * dy) + dz * dz;
}

// The pruning bound of a best squared distance: 16 eps holds the proof's 8 eps, sqrtf's error and the roundings of the four operations here.
__device__ __forceinline__ float prune_bound2(float best, float slack)
{
    const float b = sqrtf(best) * (1.0f + 16.0f * 5.9604645e-8f) + slack;
    return (b * b) * (1.0f + 4.0f * 5.9604645e-8f);
}

__device__ __forceinline__ bool point_ok(const float4 p)
{
    const float inf = __builtin_inff();
    return fabsf(p.x) < inf && fabsf(p.y) < inf && fabsf(p.z) < inf && p.w >= 0.f;  // (a NaN fails its comparison)
}

// Workgroups per CU: the stack is 8 B x STACK x kBlock of the CU's 160 KB of LDS
constexpr int closest_blocks(int STACK) { return STACK <= 16 ? 5 : STACK <= 24 ? 3 : STACK <= 32 ? 2 : 1; }

// FILTER: the mesh-mask table (RayFilter::tri_mask by global id), read before the cascade: a rejected triangle is as if it were not in
// the scene.  One body, FILTER a template flag of the kernel itself: there is no older plain kernel whose schedule a shared function
// could disturb, and the plain instantiation carries no trace of the filter (tools/kernel_regs.sh: the same registers).
template <int STACK, bool FILTER>
__global__ __launch_bounds__(kBlock, closest_blocks(STACK)) void k_closest_points(BvhDev bvh, ClosestArgs a, RayFilter f)
{
    __shared__ uint2 lds_stack[STACK * kBlock];
    uint2* const     stack = lds_stack + threadIdx.x;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock)
    {
        const float4 p = a.points[i];
        if (!point_ok(p))
        {
            a.out[2 * (size_t)i]     = make_float4(0.f, 0.f, 0.f, 0.f);
            a.out[2 * (size_t)i + 1] = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
            continue;
        }
        const float r2       = p.w * p.w;
        float       best     = r2, bound2 = prune_bound2(r2, a.slack);
        uint32_t    best_gid = kInvalidId;
        int         node = bvh.root, sp = 0;
        while (bvh.tri_count != 0u)
        {
            if (node >= 0)
            {
                const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                             q3 = bvh.nodes[4 * node + 3];
                const float b0 = box_dist2(p.x, p.y, p.z, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y);
                const float b1 = box_dist2(p.x, p.y, p.z, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w);
                const int   c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
                const bool  k0 = !(b0 > bound2), k1 = !(b1 > bound2);
                if (k0 && k1)
                {
                    const bool swap = b1 < b0;
                    if (sp < STACK) stack[(sp++) * kBlock] = make_uint2(f2u(swap ? b0 : b1), (uint32_t)(swap ? c0 : c1));
                    node = swap ? c1 : c0;
                    continue;
                }
                if (k0 || k1)
                {
                    node = k0 ? c0 : c1;
                    continue;
                }
            }
            else
            {
                const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                for (uint32_t leaf = first; leaf <= last; ++leaf)
                {
                    const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                    if constexpr (FILTER)
                        if ((f.tri_mask[gid] & f.mask) == 0u) continue;
                    const float4 t0 = bvh.tris[4 * (size_t)leaf + 0], t1 = bvh.tris[4 * (size_t)leaf + 1], t2 = bvh.tris[4 * (size_t)leaf + 2];
                    const float  d2 = closest_dist2(t0, t1, t2, p.x, p.y, p.z);
                    if (d2 < best || (d2 == best && gid < best_gid))
                    {
                        if (d2 < best) bound2 = prune_bound2(d2, a.slack);
                        best = d2, best_gid = gid;
                    }
                }
            }
            bool more = false;
            while (sp > 0)
            {
                const uint2 e = stack[(--sp) * kBlock];
                if (!(u2f(e.x) > bound2))
                {
                    node = (int)e.y, more = true;
                    break;
                }
            }
            if (!more) break;
        }
        if (best_gid == kInvalidId)
        {
            a.out[2 * (size_t)i]     = make_float4(0.f, 0.f, 0.f, r2);
            a.out[2 * (size_t)i + 1] = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
            continue;
        }
        // the winner's record from the records in id order (byte copies of the tree's, see multi_write in query.hip)
        const float4*      rec = bvh.tris_by_id + 4 * (size_t)best_gid;
        const ClosestPoint c   = closest_record(rec[0], rec[1], rec[2], p.x, p.y, p.z);
        a.out[2 * (size_t)i]     = make_float4(c.x, c.y, c.z, c.d2);
        a.out[2 * (size_t)i + 1] = make_float4(c.u, c.v, u2f(best_gid), u2f(c.feature));
    }
}

template <int STACK, bool FILTER>
void launch_closest_s(const LaunchCfg& cfg, const BvhDev& b, const ClosestArgs& a, const RayFilter& f)
{
    uint32_t want = (a.n + kBlock - 1) / kBlock;
    if (want == 0) want = 1;
    hipLaunchKernelGGL((k_closest_points<STACK, FILTER>), dim3(resident_grid<k_closest_points<STACK, FILTER>>(cfg, want)), dim3(kBlock), 0, cfg.stream,
                       b, a, f);
}

// ---- k nearest and in-radius (cap_closest_points_multi) ----
// A point's first k candidates in (dist2, triangle) order, the number of its candidates, or both.  k_closest_points' walk with
// HitList<K> (dist2 in the place of a ray's t) instead of the single best pair: the K - k placeholders in front, the k live slots
// starting as (r2, ~0), so `dist2 <= r2`, the tie rule and "not full yet" are admits()' one comparison.  The pruning bound is
// prune_bound2 of slot K - 1's dist2 -- r2 until the list holds k candidates, then the k-th -- computed again only when that slot
// changes; with COUNT every candidate within the radius has to be seen and it stays prune_bound2(r2).  The test is the same strict >
// at every push, descent and pop: a subtree at exactly the k-th distance is opened and an equal-dist2 triangle with a lower id still
// displaces the k-th entry, so the list is exact whatever the visiting order (DESIGN.md "Multi closest-point queries").
// Paging: only candidates above the cursor (dist2_c, g_c) -- words 3 and 6 of slot k - 1 of the point's page, (-inf, 0) otherwise --
// are counted and offered.  The cursor prunes nothing: a subtree wholly below it is still walked (skipping those whose farthest corner
// lies below dist2_c is left out).  Unlike a ray's hit (t < tmax) a candidate may lie AT the limit, and a triangle beyond it passes a
// miss record's cursor (r2, ~0) only by failing dist2 <= r2: COUNT tests that itself, the list's admits() implies it.
// Write-out: only (dist2, gid) live in the list; each listed triangle's record is computed again from tris_by_id as k_closest_points
// does for its winner -- the same operations on the same words, the same dist2 bits.  The slot is picked by a chain of K selects
// inside a loop over the k slots rather than K unrolled cascades.
struct ClosestCursor
{
    float    d2;
    uint32_t gid;
};

// Workgroups per CU: closest_blocks(STACK) is what the LDS stack allows; the list's 2 K registers (and the cursor and count) take it
// down to the most that leave every instantiation without scratch (tools/kernel_regs.sh; the table is in DESIGN.md): up to K = 8 the
// list fits five (96 VGPRs; 77 used), K = 16 runs four (128; 110 used) -- five spill 48 to 52 bytes.  Only STACK = 16 has LDS for that many.
constexpr int closest_multi_blocks(int STACK, int K)
{
    const int by_regs = K <= 8 ? 5 : 4;
    return closest_blocks(STACK) < by_regs ? closest_blocks(STACK) : by_regs;
}

template <int STACK, int K, bool COUNT, bool FILTER>
__global__ __launch_bounds__(kBlock, closest_multi_blocks(STACK, K)) void k_closest_points_multi(BvhDev bvh, ClosestMultiArgs m, RayFilter f)
{
    __shared__ uint2 lds_stack[STACK * kBlock];
    uint2* const     stack = lds_stack + threadIdx.x;
    const int        skip  = K - (int)m.k;  // the placeholders
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m.a.n; i += gridDim.x * kBlock)
    {
        const float4  p    = m.a.points[i];
        float4* const page = m.a.out + 2 * (size_t)i * m.k;
        const bool    ok   = point_ok(p);
        const float   r2   = ok ? p.w * p.w : 0.f;
        HitList<K>    L;
        L.init(m.k, r2);
        uint32_t count = 0u;
        if (ok)
        {
            ClosestCursor c{-__builtin_inff(), 0u};
            if (m.resume) c = ClosestCursor{page[2 * (m.k - 1u)].w, f2u(page[2 * (m.k - 1u) + 1].z)};
            float bound2 = prune_bound2(r2, m.a.slack);
            int   node = bvh.root, sp = 0;
            while (bvh.tri_count != 0u)
            {
                if (node >= 0)
                {
                    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                                 q3 = bvh.nodes[4 * node + 3];
                    const float b0 = box_dist2(p.x, p.y, p.z, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y);
                    const float b1 = box_dist2(p.x, p.y, p.z, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w);
                    const int   c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
                    const bool  k0 = !(b0 > bound2), k1 = !(b1 > bound2);
                    if (k0 && k1)
                    {
                        const bool swap = b1 < b0;
                        if (sp < STACK) stack[(sp++) * kBlock] = make_uint2(f2u(swap ? b0 : b1), (uint32_t)(swap ? c0 : c1));
                        node = swap ? c1 : c0;
                        continue;
                    }
                    if (k0 || k1)
                    {
                        node = k0 ? c0 : c1;
                        continue;
                    }
                }
                else
                {
                    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                    for (uint32_t leaf = first; leaf <= last; ++leaf)
                    {
                        const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                        if constexpr (FILTER)
                            if ((f.tri_mask[gid] & f.mask) == 0u) continue;
                        const float4 t0 = bvh.tris[4 * (size_t)leaf + 0], t1 = bvh.tris[4 * (size_t)leaf + 1], t2 = bvh.tris[4 * (size_t)leaf + 2];
                        const float  d2 = closest_dist2(t0, t1, t2, p.x, p.y, p.z);
                        // multi_offer's rule (query.hip) with dist2 in the place of t; a NaN fails every comparison
                        if ((d2 > c.d2 || (d2 == c.d2 && gid > c.gid)) && (!COUNT || d2 <= r2))
                        {
                            if (COUNT) ++count;
                            if (L.admits(d2, gid))
                            {
                                const float kth = L.t[K - 1];
                                L.insert(d2, gid);
                                if (!COUNT && L.t[K - 1] != kth) bound2 = prune_bound2(L.t[K - 1], m.a.slack);
                            }
                        }
                    }
                }
                bool more = false;
                while (sp > 0)
                {
                    const uint2 e = stack[(--sp) * kBlock];
                    if (!(u2f(e.x) > bound2))
                    {
                        node = (int)e.y, more = true;
                        break;
                    }
                }
                if (!more) break;
            }
        }
        // (a query that was not traversed: the list as init left it, k miss records with dist2 = r2 = 0, and count 0)
        if (COUNT) m.counts[i] = count;
        for (uint32_t s = 0; s < m.k; ++s)
        {
            uint32_t gid = kInvalidId;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j - skip == (int)s) gid = L.g[j];
            if (gid == kInvalidId)
            {
                page[2 * s]     = make_float4(0.f, 0.f, 0.f, r2);
                page[2 * s + 1] = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
                continue;
            }
            const float4*      rec = bvh.tris_by_id + 4 * (size_t)gid;
            const ClosestPoint c   = closest_record(rec[0], rec[1], rec[2], p.x, p.y, p.z);
            page[2 * s]     = make_float4(c.x, c.y, c.z, c.d2);
            page[2 * s + 1] = make_float4(c.u, c.v, u2f(gid), u2f(c.feature));
        }
    }
}

template <int STACK, int K, bool COUNT, bool FILTER>
void launch_closest_multi_k(const LaunchCfg& cfg, const BvhDev& b, const ClosestMultiArgs& m, const RayFilter& f)
{
    uint32_t want = (m.a.n + kBlock - 1) / kBlock;
    if (want == 0) want = 1;
    hipLaunchKernelGGL((k_closest_points_multi<STACK, K, COUNT, FILTER>), dim3(resident_grid<k_closest_points_multi<STACK, K, COUNT, FILTER>>(cfg, want)),
                       dim3(kBlock), 0, cfg.stream, b, m, f);
}

template <int STACK, int K>
void launch_closest_multi_s(const LaunchCfg& cfg, const BvhDev& b, const ClosestMultiArgs& m, bool filter, const RayFilter& f)
{
    if (m.counts)
        filter ? launch_closest_multi_k<STACK, K, true, true>(cfg, b, m, f) : launch_closest_multi_k<STACK, K, true, false>(cfg, b, m, f);
    else
        filter ? launch_closest_multi_k<STACK, K, false, true>(cfg, b, m, f) : launch_closest_multi_k<STACK, K, false, false>(cfg, b, m, f);
}

template <int STACK>
void launch_closest_multi(const LaunchCfg& cfg, const BvhDev& b, const ClosestMultiArgs& m, bool filter, const RayFilter& f)
{
    switch (multi_bucket(m.k))
    {
    case 1: launch_closest_multi_s<STACK, 1>(cfg, b, m, filter, f); break;
    case 4: launch_closest_multi_s<STACK, 4>(cfg, b, m, filter, f); break;
    case 8: launch_closest_multi_s<STACK, 8>(cfg, b, m, filter, f); break;
    default: launch_closest_multi_s<STACK, 16>(cfg, b, m, filter, f); break;
    }
}
}  // namespace

void launch_closest_points(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestArgs& a, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const bool      filter = f && f->tri_mask;
    const RayFilter rf     = f ? *f : RayFilter{};
    // a walk pushes at most one entry per level it descends
#define CAP_CLOSEST(S)                                    \
    if (filter)                                           \
        launch_closest_s<S, true>(cfg, b, a, rf);         \
    else                                                  \
        launch_closest_s<S, false>(cfg, b, a, rf);
    if (depth <= 16)
    {
        CAP_CLOSEST(16)
    }
    else if (depth <= 24)
    {
        CAP_CLOSEST(24)
    }
    else if (depth <= 32)
    {
        CAP_CLOSEST(32)
    }
    else
    {
        CAP_CLOSEST(64)
    }
#undef CAP_CLOSEST
}

void launch_closest_points_multi(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestMultiArgs& m, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const bool      filter = f && f->tri_mask;
    const RayFilter rf     = f ? *f : RayFilter{};
    if (depth <= 16)
        launch_closest_multi<16>(cfg, b, m, filter, rf);
    else if (depth <= 24)
        launch_closest_multi<24>(cfg, b, m, filter, rf);
    else if (depth <= 32)
        launch_closest_multi<32>(cfg, b, m, filter, rf);
    else
        launch_closest_multi<64>(cfg, b, m, filter, rf);
}
}  // namespace cap
