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
// The signed form (cap_signed_distance) is the same kernel with the flag SIGNED: the sign of the winner's delta against the pseudonormal
// of the feature it lies on (pseudonormal.hip builds the table), in an epilogue the unsigned instantiations do not have.
//
// The multi form (cap_closest_points_multi, k_closest_points_multi) is the same walk with the sorted list HitList<K> of cap_hit_list.h
// in the place of the single best pair; "best" above reads "k-th best", slot K - 1 of the list.
//
// The instanced forms (cap_closest_instances, k_closest_inst; cap_closest_instances_multi, k_closest_inst_multi) are at the end of the
// file: nearest, and the k nearest, in world space over the instance table.  cap_signed_distance_instances is k_closest_inst with
// SIGNED: the world record, and the sign from a flat walk of the winning instance's object tree at p' = W p.
#include "cap_closest.h"  // the cascade: closest_uv, closest_dist2, closest_record
#include "cap_hit_list.h"
#include "cap_kernels.h"
#include "cap_near.h"  // box_dist2, and the bound of the instanced form
#include "cap_query_walk.h"  // TopWalk, and the launch dispatchers

namespace cap
{
namespace
{
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

// ---- the steps every walk below is made of ----
// An inner node of a scene or object tree, measured from (px, py, pz): one fetch yields both child boxes; the nearer child that survives
// the prune is entered and the other one pushed with its box distance.  false: neither survives, the caller pops.  near_skip (cap_near.h)
// is the strict > of the pruning argument above.  A walk pushes at most one entry per level it descends and STACK is at least the tree's
// depth (with_stack_class, cap_query_walk.h).
template <int STACK>
__device__ __forceinline__ bool closest_node_step(const BvhDev& bvh, float px, float py, float pz, float bound2, uint2* stack, int& node, int& sp)
{
    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
    const float  b0 = box_dist2(px, py, pz, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y);
    const float  b1 = box_dist2(px, py, pz, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w);
    const int    c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
    const bool   k0 = !near_skip(b0, bound2), k1 = !near_skip(b1, bound2);
    if (k0 && k1)
    {
        const bool swap = b1 < b0;
        if (sp < STACK) stack[(sp++) * kBlock] = make_uint2(f2u(swap ? b0 : b1), (uint32_t)(swap ? c0 : c1));
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

// The next stack entry that still passes the bound as it stands now, one LDS read per entry; false: the stack is empty
__device__ __forceinline__ bool closest_pop(uint2* stack, int& sp, float bound2, int& node)
{
    while (sp > 0)
    {
        const uint2 e = stack[(--sp) * kBlock];
        if (!near_skip(u2f(e.x), bound2))
        {
            node = (int)e.y;
            return true;
        }
    }
    return false;
}

// A leaf of a scene or object tree for the single nearest triangle in (dist2, triangle) order, measured from (px, py, pz) on the stored
// records: the flat query's leaf, and the second phase of the signed instanced one (k_closest_inst), which walks an object's tree from
// p'.  FILTER: tri_mask by global id against `mask`, read before the cascade.  A NaN dist2 fails both comparisons.
template <bool FILTER>
__device__ __forceinline__ void closest_leaf_step(const BvhDev& bvh, int node, const uint8_t* tri_mask, uint32_t mask, float slack, float px, float py,
                                                  float pz, float& best, uint32_t& best_gid, float& bound2)
{
    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
    for (uint32_t leaf = first; leaf <= last; ++leaf)
    {
        const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
        if constexpr (FILTER)
            if ((tri_mask[gid] & mask) == 0u) continue;
        const float4 t0 = bvh.tris[4 * (size_t)leaf + 0], t1 = bvh.tris[4 * (size_t)leaf + 1], t2 = bvh.tris[4 * (size_t)leaf + 2];
        const float  d2 = closest_dist2(t0, t1, t2, px, py, pz);
        if (d2 < best || (d2 == best && gid < best_gid))
        {
            if (d2 < best) bound2 = prune_bound2(d2, slack);
            best = d2, best_gid = gid;
        }
    }
}

// A record slot without a triangle: dist2 = r2, the point's squared radius (0 for a point that was not traversed)
__device__ __forceinline__ void write_miss(float4* slot, float r2)
{
    slot[0] = make_float4(0.f, 0.f, 0.f, r2);
    slot[1] = make_float4(0.f, 0.f, u2f(kInvalidId), 0.f);
}
__device__ __forceinline__ void write_record(float4* slot, const ClosestPoint& c, uint32_t gid)
{
    slot[0] = make_float4(c.x, c.y, c.z, c.d2);
    slot[1] = make_float4(c.u, c.v, u2f(gid), u2f(c.feature));
}
// Only (dist2, ids) live in registers during a walk: the record of a triangle that is written out is computed again from the records in
// id order (byte copies of the tree's, see multi_write in query.hip) -- the same operations on the same words, the same dist2 bits.
__device__ __forceinline__ ClosestPoint scene_record(const BvhDev& bvh, uint32_t gid, const float4 p)
{
    const float4* rec = bvh.tris_by_id + 4 * (size_t)gid;
    return closest_record(rec[0], rec[1], rec[2], p.x, p.y, p.z);
}

// FILTER: the mesh-mask table (RayFilter::tri_mask by global id), read before the cascade: a rejected triangle is as if it were not in
// the scene.  One body, FILTER a template flag of the kernel itself: there is no older plain kernel whose schedule a shared function
// could disturb, and the plain instantiation carries no trace of the filter (tools/kernel_regs.sh: the same registers).
// SIGNED (cap_signed_distance): the same walk and record, and an epilogue on the winner's own delta -- one 12-byte gather from the
// pseudonormal table, dot_c, a square root.  Again a flag of the kernel: the unsigned instantiations keep their registers.
template <int STACK, bool FILTER, bool SIGNED = false>
__global__ __launch_bounds__(kBlock, closest_blocks(STACK)) void k_closest_points(BvhDev bvh, ClosestArgs a, RayFilter f, SignedArgs s)
{
    __shared__ uint2 lds_stack[STACK * kBlock];
    uint2* const     stack = lds_stack + threadIdx.x;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock)
    {
        const float4 p = a.points[i];
        if (!point_ok(p))
        {
            write_miss(a.out + 2 * (size_t)i, 0.f);
            if constexpr (SIGNED) s.signed_out[i] = __builtin_inff();
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
                if (closest_node_step<STACK>(bvh, p.x, p.y, p.z, bound2, stack, node, sp)) continue;
            }
            else
            {
                closest_leaf_step<FILTER>(bvh, node, f.tri_mask, f.mask, a.slack, p.x, p.y, p.z, best, best_gid, bound2);
            }
            if (!closest_pop(stack, sp, bound2, node)) break;
        }
        if (best_gid == kInvalidId)
        {
            write_miss(a.out + 2 * (size_t)i, r2);
            if constexpr (SIGNED) s.signed_out[i] = __builtin_inff();
            continue;
        }
        const ClosestPoint c = scene_record(bvh, best_gid, p);
        write_record(a.out + 2 * (size_t)i, c, best_gid);
        if constexpr (SIGNED)
        {
            // d == 0 (dist2 == 0 among them) and a NaN take the positive sign
            const float* const nn   = s.normals + 21 * (size_t)best_gid + 3u * c.feature;
            const float        d    = dot_c(c.dx, c.dy, c.dz, nn[0], nn[1], nn[2]);
            const float        dist = sqrtf(c.d2);
            s.signed_out[i]         = d < 0.f ? -dist : dist;
        }
    }
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
// Write-out: scene_record per listed triangle.  The slot is picked by a chain of K selects inside a loop over the k slots rather than K
// unrolled cascades.
struct ClosestCursor
{
    float    d2;
    uint32_t gid;
};

// Workgroups per CU: closest_blocks(STACK) is what the LDS stack allows; the list's 2 K registers (and the cursor and count) take it
// down to the most that leave every instantiation without scratch (tools/kernel_regs.sh; the table is in DESIGN.md): up to K = 8 the
// list fits five (96 VGPRs; 77 used), K = 16 runs four (128; 111 used) -- five spill 48 to 52 bytes.  Only STACK = 16 has LDS for that many.
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
                    if (closest_node_step<STACK>(bvh, p.x, p.y, p.z, bound2, stack, node, sp)) continue;
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
                if (!closest_pop(stack, sp, bound2, node)) break;
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
                write_miss(page + 2 * s, r2);
            else
                write_record(page + 2 * s, scene_record(bvh, gid, p), gid);
        }
    }
}

// ---- over the instance table (cap_closest_instances) ----
// For every point the pair (instance, triangle) minimal in (dist2, instance, triangle), dist2 the cascade's on the WORLD record
//   v0w_r = fl(dot_c(M_r.xyz, v0) + M_r.w),  e1w_r = dot_c(M_r.xyz, e1),  e2w_r = dot_c(M_r.xyz, e2)
// of the instance's transform M as the caller gave it (a.descs), no fused multiply-add: include/capsaicin_hip.h has the contract.
// One loop with three kinds of step, as k_query_inst (instance.hip), so that the lanes of a wave that are at the top level advance
// while others are inside an instance:
//   * a top-level node (top_step);
//   * entering an instance (enter_instance);
//   * a bottom-level node or leaf: the walk of the object's tree with its LDS stack of (box distance, child), the boxes measured from
//     p' and pruned against bound2, the world bound mapped into object space through g <= sigma_min(M) (cap_near.h
//     near_bound2_object).  A leaf builds the world record and runs the cascade.
// Both bounds are computed again only when `best` improves; every test is a strict >, so an instance, subtree or triangle at exactly
// the best distance is still opened and the lower (instance, triangle) wins whatever the visiting order.  DESIGN.md "Closest-point
// queries over instances" has the argument that no skipped box holds a candidate.  (world_record: cap_query_walk.h.)
// scene_record for a listed pair: the world record again from the records in id order and the instance's transform
__device__ __forceinline__ ClosestPoint instance_record(const BvhDev& bvh, const float4* descs, uint32_t inst, uint32_t gid, const float4 p)
{
    const float4*     rec = bvh.tris_by_id + 4 * (size_t)gid;
    const float4*     md  = descs + 4 * (size_t)inst;
    const WorldRecord w   = world_record(md[0], md[1], md[2], rec[0], rec[1], rec[2]);
    return closest_record(w.t0, w.t1, w.t2, p.x, p.y, p.z);
}

// One top-level node: the two children ordered by the squared distance from p to their stored world boxes and pruned against
// bound2_top; then down into the nearer one, or their instances into the queue, or up to the nearest level that owes a child.
__device__ __forceinline__ TopWalk top_step(const TlasDev& tl, const uint32_t* lds_off, float px, float py, float pz, float bound2_top, TopWalk t)
{
    const float4* c = tl.tlas + 2 * (size_t)(lds_off[t.level - 1u] + 2u * t.idx);
    const float4  lo0 = c[0], hi0 = c[1], lo1 = c[2], hi1 = c[3];
    const float   d0 = box_dist2(px, py, pz, lo0.x, lo0.y, lo0.z, hi0.x, hi0.y, hi0.z);
    const float   d1 = box_dist2(px, py, pz, lo1.x, lo1.y, lo1.z, hi1.x, hi1.y, hi1.z);
    // (a record with k < 0 holds nothing: an inert instance or the padding of a level)
    const bool h0 = lo0.w >= 0.0f && !near_skip(d0, bound2_top), h1 = lo1.w >= 0.0f && !near_skip(d1, bound2_top);
    return top_advance(t, h0, h1, h0 && h1 && d1 < d0, f2u(hi0.w), f2u(hi1.w), d0, d1);  // the nearer box first
}
// Entering an instance: its mask joined with the call's (the mesh byte joins it per triangle), M for the leaves' world records,
// p' = W p + W_t, which only the pruning sees, (g, slack) of cap_near.h and the root of the object's tree.  The caller maps its bound into
// object space: near_bound2_object(sqrt of its best or k-th dist2, slack, g).  false: the mask excludes the instance (0 for an inert one);
// the mask word is loaded first and the rest only for an instance it lets in.  The results go straight into the kernel's own variables:
// returned by value, or filled into one struct of the kernel's, they made the compiler allocate k_closest_inst_multi anew (DESIGN.md "One
// copy of each step").
__device__ __forceinline__ bool enter_instance(const TlasDev& tl, const ClosestInstArgs& ia, uint32_t mask, uint32_t inst, const float4 p, float pmax,
                                               uint32_t& imask, float4& m0, float4& m1, float4& m2, float& ox, float& oy, float& oz, float& g, float& slack,
                                               int& root)
{
    const float4 w3 = tl.rec[4 * (size_t)inst + 3];
    imask           = f2u(w3.x) & mask;
    if (imask == 0u) return false;
    const float4 w0 = tl.rec[4 * (size_t)inst], w1 = tl.rec[4 * (size_t)inst + 1], w2 = tl.rec[4 * (size_t)inst + 2];
    const float  w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    near_to_object(w, p.x, p.y, p.z, ox, oy, oz);
    m0 = ia.descs[4 * (size_t)inst], m1 = ia.descs[4 * (size_t)inst + 1], m2 = ia.descs[4 * (size_t)inst + 2];
    const float2 nr = ia.near[inst];
    g = nr.x, slack = near_slack(pmax, nr.y);
    root = (int)f2u(w3.y);
    return true;
}

// Workgroups per CU: the stack's LDS (and the 104 bytes of level offsets, which take the fifth workgroup of STACK = 16 away)
constexpr int closest_inst_blocks(int STACK) { return STACK <= 16 ? 4 : STACK <= 24 ? 3 : STACK <= 32 ? 2 : 1; }

// The sign of cap_signed_distance_instances for a point whose world winner is (inst, gid): the flat signed query at p' = W p over the
// instance's own candidates, radius +inf -- inside and outside are the same in object space, whatever the transform (a mirror
// included), and object space is where the pseudonormal table lives.  The walk is k_closest_points' on the object's tree from p', with
// the flat bound prune_bound2(best', slack) and the scene's slack (DESIGN.md "Signed distance over instances"); best' is seeded with
// the world winner's own triangle at p', a candidate by construction, so the walk starts with a tight bound and the winner under the
// tie rule (dist2', triangle) is what it would be without the seed.  true: d = dot_c(delta', N[g'][feature']) < 0.  An overflowed p'
// or no candidate with a dist2' that is not NaN: false.
template <int STACK, bool FILTER>
__device__ __forceinline__ bool object_sign_negative(const BvhDev& bvh, const TlasDev& tl, const RayFilter& f, const float* normals, float slack,
                                                     uint32_t inst, uint32_t gid, const float4 p, uint2* stack)
{
    const float4   w0 = tl.rec[4 * (size_t)inst], w1 = tl.rec[4 * (size_t)inst + 1], w2 = tl.rec[4 * (size_t)inst + 2], w3 = tl.rec[4 * (size_t)inst + 3];
    const uint32_t imask = f2u(w3.x) & f.mask;
    const float    w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    float4         o     = make_float4(0.f, 0.f, 0.f, 0.f);
    near_to_object(w, p.x, p.y, p.z, o.x, o.y, o.z);
    if (!point_ok(o)) return false;
    const float4* seed = bvh.tris_by_id + 4 * (size_t)gid;
    const float   d2s  = closest_dist2(seed[0], seed[1], seed[2], o.x, o.y, o.z);
    const bool    some = d2s == d2s;
    float         best = some ? d2s : __builtin_inff(), bound2 = prune_bound2(best, slack);
    uint32_t      best_gid = some ? gid : kInvalidId;
    int           node = (int)f2u(w3.y), sp = 0;
    for (;;)
    {
        if (node >= 0)
        {
            if (closest_node_step<STACK>(bvh, o.x, o.y, o.z, bound2, stack, node, sp)) continue;
        }
        else
            closest_leaf_step<FILTER>(bvh, node, f.tri_mask, imask, slack, o.x, o.y, o.z, best, best_gid, bound2);
        if (!closest_pop(stack, sp, bound2, node)) break;
    }
    if (best_gid == kInvalidId) return false;
    const ClosestPoint c  = scene_record(bvh, best_gid, o);
    const float* const nn = normals + 21 * (size_t)best_gid + 3u * c.feature;
    return dot_c(c.dx, c.dy, c.dz, nn[0], nn[1], nn[2]) < 0.f;
}

// FILTER: a mesh-mask table is installed (f.tri_mask by global id); the instance's own mask is tested either way.
// SIGNED (cap_signed_distance_instances): the same walk and record, then a second phase in the same lane on the same stack slice,
// object_sign_negative above, and the signed value from the WORLD record's dist2.  A flag of the kernel: the unsigned instantiations keep
// their registers (tools/kernel_regs.sh).  ia.a.slack is the scene's flat slack for the signed launch and is not read otherwise.
template <int STACK, bool FILTER, bool SIGNED = false>
__global__ __launch_bounds__(kBlock, closest_inst_blocks(STACK)) void k_closest_inst(BvhDev bvh, ClosestInstArgs ia, TlasDev tl, RayFilter f, SignedArgs s)
{
    __shared__ uint2    lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint2* const        stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const ClosestArgs& a      = ia.a;
    const float        xw_all = u2f(ia.xw_max[0]);  // the largest Xw of the table: the top level's slack holds for every instance
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.n; j += gridDim.x * kBlock)
    {
        const float4 p = a.points[j];
        if (!point_ok(p))
        {
            write_miss(a.out + 2 * (size_t)j, 0.f);
            if (ia.inst_out) ia.inst_out[j] = kInvalidId;
            if constexpr (SIGNED) s.signed_out[j] = __builtin_inff();
            continue;
        }
        const float r2   = p.w * p.w;
        const float pmax = fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z)));
        float       best = r2, sqrt_best = sqrtf(r2);
        uint32_t    best_gid = kInvalidId, best_inst = kInvalidId;
        const float slack_top  = near_slack(pmax, xw_all);
        float       bound2_top = near_bound2_world(sqrt_best, slack_top);
        TopWalk     t          = top_start(tl);
        // bottom level: the instance being walked
        bool     in_blas = false;
        float4   m0 = make_float4(0.f, 0.f, 0.f, 0.f), m1 = m0, m2 = m0;
        float    ox = 0.f, oy = 0.f, oz = 0.f, g = 1.f, slack = 0.f, bound2 = 0.f;
        uint32_t inst = 0u, imask = 0u;
        int      node = 0, sp = 0;
        bool     walk = bvh.tri_count != 0u;
        while (walk)
        {
            if (in_blas)
            {
                if (node >= 0)
                {
                    if (closest_node_step<STACK>(bvh, ox, oy, oz, bound2, stack, node, sp)) continue;
                }
                else
                {
                    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                    for (uint32_t leaf = first; leaf <= last; ++leaf)
                    {
                        const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                        if constexpr (FILTER)
                            if ((f.tri_mask[gid] & imask) == 0u) continue;
                        const WorldRecord w  = world_record(m0, m1, m2, bvh.tris[4 * (size_t)leaf + 0], bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2]);
                        const float       d2 = closest_dist2(w.t0, w.t1, w.t2, p.x, p.y, p.z);
                        if (d2 < best || (d2 == best && (inst < best_inst || (inst == best_inst && gid < best_gid))))
                        {
                            if (d2 < best)
                            {
                                sqrt_best  = sqrtf(d2);
                                bound2     = near_bound2_object(sqrt_best, slack, g);
                                bound2_top = near_bound2_world(sqrt_best, slack_top);
                            }
                            best = d2, best_gid = gid, best_inst = inst;
                        }
                    }
                }
                in_blas = closest_pop(stack, sp, bound2, node);
                continue;
            }
            if (t.todo0 != kInvalidId)
            {
                // the head of the queue, if its box still passes against the bound as it is now
                inst             = t.todo0;
                const bool still = !near_skip(t.todo0_d, bound2_top);
                t                = top_pop(t);
                if (still && enter_instance(tl, ia, f.mask, inst, p, pmax, imask, m0, m1, m2, ox, oy, oz, g, slack, node))
                {
                    bound2  = near_bound2_object(sqrt_best, slack, g);
                    sp      = 0;
                    in_blas = true;
                }
                continue;
            }
            if (t.done) break;
            t = top_step(tl, lds_off, p.x, p.y, p.z, bound2_top, t);
        }
        if (ia.inst_out) ia.inst_out[j] = best_inst;
        if (best_gid == kInvalidId)
        {
            write_miss(a.out + 2 * (size_t)j, r2);
            if constexpr (SIGNED) s.signed_out[j] = __builtin_inff();
            continue;
        }
        const ClosestPoint c = instance_record(bvh, ia.descs, best_inst, best_gid, p);
        write_record(a.out + 2 * (size_t)j, c, best_gid);
        if constexpr (SIGNED)
        {
            // dist2 == 0 is +0.0 whatever the object-space walk says
            const float dist = sqrtf(c.d2);
            const bool  neg  = c.d2 != 0.f && object_sign_negative<STACK, FILTER>(bvh, tl, f, s.normals, a.slack, best_inst, best_gid, p, stack);
            s.signed_out[j]  = neg ? -dist : dist;
        }
    }
}

// ---- k nearest and in-radius over the instance table (cap_closest_instances_multi) ----
// A point's first k candidate pairs in (dist2, instance, triangle) order, the number of its pairs, or both: k_closest_inst's loop with
// InstHitList<K> of cap_hit_list.h in the place of (best, best_inst, best_gid), as k_closest_points_multi stands to k_closest_points.
// The list moved to that header rather than being copied here: k_query_inst_multi's code is unchanged by it (tools/kernel_regs.sh: the
// same rows).
// Bounds: bound2 and bound2_top derive from slot K - 1's dist2 -- r2 until the list holds k pairs, then the k-th -- through one sqrtf,
// computed again only when that slot's value changes (and bound2 on entering an instance, from the value as it stands); with COUNT
// every pair within the radius has to be seen and both stay at r2's.  Every test is near_skip's strict >: an instance, subtree or
// triangle at exactly the k-th distance is opened and an equal-dist2 pair with a lower (instance, triangle) still displaces the k-th
// entry, so the list is exact whatever the visiting order (DESIGN.md "Multi closest-point queries over instances").
// Offer: above the cursor (dist2_c, i_c, g_c) -- words 3 and 6 of slot k - 1 of the record page and slot k - 1 of the instance page,
// (-inf, 0, 0) otherwise --; with COUNT `dist2 <= r2` itself and ++count (a pair may lie AT the limit, and one beyond it passes a miss
// record's cursor (r2, ~0, ~0)); then admits / insert.  The cursor prunes nothing.
// Write-out: instance_record per listed pair.  The slot is picked by a chain of K selects inside a loop over the k slots; the cursor is
// read before anything is written; k = 0 dereferences neither page.
// The mesh-mask table is a wave-uniform test of f.tri_mask per leaf, as in k_query_inst_multi, not a template flag: with the list in
// registers the flag would double 32 instantiations for the two SGPR pairs it saves.

// Workgroups per CU: closest_inst_blocks(STACK) is what the LDS allows; the list's 3 K registers (and cursor and count) take it down to
// the most that leave every instantiation without scratch (tools/kernel_regs.sh; the table is in DESIGN.md): up to K = 4 the LDS's four
// (128 VGPRs; 86 to 98 used at K = 1, 128 at K = 4 in the 16-entry class, which has not one to spare), two (256; about 200 used) at K = 8 -- three (168) spill 104 to 120 bytes --
// and one (512; about 260 used) at K = 16 -- two spill 12 to 28 bytes.  The compiler keeps the list twice across insert()'s
// compare-swaps, as in k_query_inst_multi, so a slot costs six registers rather than three.
constexpr int closest_inst_multi_blocks(int STACK, int K)
{
    const int by_regs = K <= 4 ? 4 : K <= 8 ? 2 : 1;
    return closest_inst_blocks(STACK) < by_regs ? closest_inst_blocks(STACK) : by_regs;
}

template <int STACK, int K, bool COUNT>
__global__ __launch_bounds__(kBlock, closest_inst_multi_blocks(STACK, K)) void k_closest_inst_multi(BvhDev bvh, ClosestInstMultiArgs m, TlasDev tl,
                                                                                                       RayFilter f)
{
    __shared__ uint2    lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint2* const        stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const ClosestInstArgs& ia     = m.ia;
    const float            xw_all = u2f(ia.xw_max[0]);
    const int              skip   = K - (int)m.k;  // the placeholders
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < ia.a.n; j += gridDim.x * kBlock)
    {
        const float4    p     = ia.a.points[j];
        float4* const   page  = ia.a.out + 2 * (size_t)j * m.k;
        uint32_t* const ipage = ia.inst_out + (size_t)j * m.k;
        const bool      ok    = point_ok(p);
        const float     r2    = ok ? p.w * p.w : 0.f;
        InstHitList<K>  L;
        L.init(m.k, r2);
        // the cursor: slot k - 1 of both pages when paging, else (-inf, 0, 0), below every pair
        float    dc = -__builtin_inff();
        uint32_t ic = 0u, gc = 0u, count = 0u;
        if (m.resume && ok) dc = page[2 * (m.k - 1u)].w, gc = f2u(page[2 * (m.k - 1u) + 1].z), ic = ipage[m.k - 1u];
        const float pmax      = fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z)));
        float       sqrt_kth  = sqrtf(r2);
        const float slack_top = near_slack(pmax, xw_all);
        float       bound2_top = near_bound2_world(sqrt_kth, slack_top);
        TopWalk     t          = top_start(tl);
        // bottom level: the instance being walked
        bool     in_blas = false;
        float4   m0 = make_float4(0.f, 0.f, 0.f, 0.f), m1 = m0, m2 = m0;
        float    ox = 0.f, oy = 0.f, oz = 0.f, g = 1.f, slack = 0.f, bound2 = 0.f;
        uint32_t inst = 0u, imask = 0u;
        int      node = 0, sp = 0;
        bool     walk = ok && bvh.tri_count != 0u;
        while (walk)
        {
            if (in_blas)
            {
                if (node >= 0)
                {
                    if (closest_node_step<STACK>(bvh, ox, oy, oz, bound2, stack, node, sp)) continue;
                }
                else
                {
                    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                    for (uint32_t leaf = first; leaf <= last; ++leaf)
                    {
                        const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                        if (f.tri_mask && (f.tri_mask[gid] & imask) == 0u) continue;
                        const WorldRecord w  = world_record(m0, m1, m2, bvh.tris[4 * (size_t)leaf + 0], bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2]);
                        const float       d2 = closest_dist2(w.t0, w.t1, w.t2, p.x, p.y, p.z);
                        // k_closest_points_multi's offer with the instance between dist2 and the triangle; a NaN fails every comparison
                        if (InstHitList<K>::before(dc, ic, gc, d2, inst, gid) && (!COUNT || d2 <= r2))
                        {
                            if (COUNT) ++count;
                            if (L.admits(d2, inst, gid))
                            {
                                const float kth = L.t[K - 1];
                                L.insert(d2, inst, gid);
                                if (!COUNT && L.t[K - 1] != kth)
                                {
                                    sqrt_kth   = sqrtf(L.t[K - 1]);
                                    bound2     = near_bound2_object(sqrt_kth, slack, g);
                                    bound2_top = near_bound2_world(sqrt_kth, slack_top);
                                }
                            }
                        }
                    }
                }
                in_blas = closest_pop(stack, sp, bound2, node);
                continue;
            }
            if (t.todo0 != kInvalidId)
            {
                // the head of the queue, if its box still passes against the bound as it is now
                inst             = t.todo0;
                const bool still = !near_skip(t.todo0_d, bound2_top);
                t                = top_pop(t);
                if (still && enter_instance(tl, ia, f.mask, inst, p, pmax, imask, m0, m1, m2, ox, oy, oz, g, slack, node))
                {
                    bound2  = near_bound2_object(sqrt_kth, slack, g);
                    sp      = 0;
                    in_blas = true;
                }
                continue;
            }
            if (t.done) break;
            t = top_step(tl, lds_off, p.x, p.y, p.z, bound2_top, t);
        }
        // (a point that was not traversed: the list as init left it, k miss records with dist2 = r2 = 0 and instance ~0, and count 0)
        if (COUNT) m.counts[j] = count;
        for (uint32_t s = 0; s < m.k; ++s)
        {
            uint32_t gid = kInvalidId, li = kInvalidId;
#pragma unroll
            for (int q = 0; q < K; ++q)
                if (q - skip == (int)s) gid = L.g[q], li = L.i[q];
            ipage[s] = li;
            if (gid == kInvalidId)
                write_miss(page + 2 * s, r2);
            else
                write_record(page + 2 * s, instance_record(bvh, ia.descs, li, gid, p), gid);
        }
    }
}

// ---- launchers ----
// cap_closest_points and, SIGNED, cap_signed_distance
template <bool SIGNED>
void launch_closest(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestArgs& a, const SignedArgs& s, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const RayFilter rf = f ? *f : RayFilter{};
    with_stack_class(depth, [&](auto S) {
        with_flag(f && f->tri_mask, [&](auto FILTER) { launch_points<k_closest_points<decltype(S)::value, decltype(FILTER)::value, SIGNED>>(cfg, a.n, b, a, rf, s); });
    });
}
}  // namespace

void launch_closest_points(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestArgs& a, const RayFilter* f, uint32_t depth)
{
    launch_closest<false>(cfg, bvh, a, SignedArgs{}, f, depth);
}

void launch_signed_distance(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestArgs& a, const SignedArgs& s, const RayFilter* f, uint32_t depth)
{
    launch_closest<true>(cfg, bvh, a, s, f, depth);
}

void launch_closest_points_multi(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestMultiArgs& m, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const RayFilter rf = f ? *f : RayFilter{};
    with_stack_class(depth, [&](auto S) {
        with_k_bucket(m.k, [&](auto K) {
            with_flag(m.counts != nullptr, [&](auto COUNT) {
                with_flag(f && f->tri_mask, [&](auto FILTER) {
                    launch_points<k_closest_points_multi<decltype(S)::value, decltype(K)::value, decltype(COUNT)::value, decltype(FILTER)::value>>(cfg, m.a.n, b, m, rf);
                });
            });
        });
    });
}

void launch_closest_instances(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestInstArgs& a, const TlasDev& tl, const RayFilter& f, uint32_t depth)
{
    // (depth: of the deepest bottom-level tree)
    with_stack_class(depth, [&](auto S) {
        with_flag(f.tri_mask != nullptr, [&](auto FILTER) { launch_points<k_closest_inst<decltype(S)::value, decltype(FILTER)::value>>(cfg, a.a.n, bvh, a, tl, f, SignedArgs{}); });
    });
}

void launch_signed_distance_instances(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestInstArgs& a, const SignedArgs& s, const TlasDev& tl,
                                      const RayFilter& f, uint32_t depth)
{
    with_stack_class(depth, [&](auto S) {
        with_flag(f.tri_mask != nullptr, [&](auto FILTER) { launch_points<k_closest_inst<decltype(S)::value, decltype(FILTER)::value, true>>(cfg, a.a.n, bvh, a, tl, f, s); });
    });
}

void launch_closest_instances_multi(const LaunchCfg& cfg, const BvhDev& bvh, const ClosestInstMultiArgs& m, const TlasDev& tl, const RayFilter& f,
                                    uint32_t depth)
{
    with_stack_class(depth, [&](auto S) {
        with_k_bucket(m.k, [&](auto K) {
            with_flag(m.counts != nullptr, [&](auto COUNT) {
                launch_points<k_closest_inst_multi<decltype(S)::value, decltype(K)::value, decltype(COUNT)::value>>(cfg, m.ia.a.n, bvh, m, tl, f);
            });
        });
    });
}
}  // namespace cap
