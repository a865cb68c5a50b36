// cap_query_walk.h — what the per-lane query kernels of query.hip, instance.hip, point_query.hip and winding.hip share: the binary tree's
// node step and pop for a ray, the state and the tail of the instance table's stack-free top-level walk, and the host-side dispatch from run-time values
// (stack class, list capacity, flags) to kernel instantiations.  Every device helper is __forceinline__; how its state crosses it is
// deliberate (DESIGN.md "How state crosses a helper decides what the compiler makes of it").
#pragma once

#include <type_traits>

#include "cap_kernels.h"
#include "cap_trace.h"

namespace cap
{
// The kernels handed to the dispatchers live in their files' anonymous namespaces, so these helpers are internal to each file as well.
namespace
{
// ---- the binary tree under a ray ----
// An inner node: one fetch yields both child boxes; `slab` on each against the caller's box ray rb (its tmin is the caller's lower
// bound) and far bound; both hit: the nearer child is entered and the other one pushed; one hit: it is entered.  false: neither is
// hit, the caller pops.  A walk pushes at most one entry per level it descends and the host picks STACK from the tree's depth; the
// guard drops a push beyond it rather than write outside the lane's LDS column.
template <int STACK>
__device__ __forceinline__ bool ray_node_step(const BvhDev& bvh, const Ray& rb, float tfar, uint32_t* stack, int& node, int& sp)
{
    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
    float        tn0, tn1;
    const bool   h0 = slab(rb, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tfar, tn0);
    const bool   h1 = slab(rb, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tfar, tn1);
    const int    c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
    if (h0 && h1)
    {
        const bool swap = tn1 < tn0;
        if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)(swap ? c0 : c1);
        node = swap ? c1 : c0;
        return true;
    }
    if (h0 || h1)
    {
        node = h0 ? c0 : c1;
        return true;
    }
    return false;
}

// The next stack entry; false: the stack is empty
__device__ __forceinline__ bool ray_pop(const uint32_t* stack, int& sp, int& node)
{
    if (sp == 0) return false;
    node = (int)stack[(--sp) * kBlock];
    return true;
}

// ---- the world record of an instanced triangle (cap_closest_instances' contract; cap_overlap_instances takes it unchanged) ----
// dot of the contracts: no fused multiply-add (the build has -ffp-contract=off; fmaf is nowhere written)
__device__ __forceinline__ float dot_c(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// (v0w, e1w, e2w) of the stored record (t0, t1, t2) = (v0, e1, e2) under the rows m0 .. m2 of the instance's transform M as the caller
// gave it:  v0w_r = fl(dot_c(M_r.xyz, v0) + M_r.w),  e1w_r = dot_c(M_r.xyz, e1),  e2w_r = dot_c(M_r.xyz, e2), packed like a stored record
struct WorldRecord
{
    float4 t0, t1, t2;
};
__device__ __forceinline__ WorldRecord world_record(const float4 m0, const float4 m1, const float4 m2, const float4 t0, const float4 t1, const float4 t2)
{
    WorldRecord w;
    w.t0 = make_float4(dot_c(m0.x, m0.y, m0.z, t0.x, t0.y, t0.z) + m0.w, dot_c(m1.x, m1.y, m1.z, t0.x, t0.y, t0.z) + m1.w,
                       dot_c(m2.x, m2.y, m2.z, t0.x, t0.y, t0.z) + m2.w, dot_c(m0.x, m0.y, m0.z, t0.w, t1.x, t1.y));
    w.t1 = make_float4(dot_c(m1.x, m1.y, m1.z, t0.w, t1.x, t1.y), dot_c(m2.x, m2.y, m2.z, t0.w, t1.x, t1.y), dot_c(m0.x, m0.y, m0.z, t1.z, t1.w, t2.x),
                       dot_c(m1.x, m1.y, m1.z, t1.z, t1.w, t2.x));
    w.t2 = make_float4(dot_c(m2.x, m2.y, m2.z, t1.z, t1.w, t2.x), 0.f, 0.f, 0.f);
    return w;
}

// ---- the top level of the instanced kernels: the implicit tree without a stack ----
// This state crosses a step BY VALUE, in and out (t = step(.., t)): handed over as eight reference parameters it cost every instanced
// closest-point instantiation 20 bytes of scratch.
struct TopWalk
{
    uint32_t level, idx;      // the node whose two children (level - 1, 2 idx + {0, 1}) are tested next
    uint32_t pending;         // bit l: the other child of the node entered at level l is still owed
    bool     done;            // nothing is owed any more
    uint32_t todo0, todo1;    // the two instances under a level-1 node wait here, the nearer first (~0: none) ...
    float    todo0_d, todo1_d;  // ... with their boxes' distances: each is tested again against the bound as it stands when its turn comes
};
__device__ __forceinline__ TopWalk top_start(const TlasDev& tl) { return TopWalk{tl.top + 1u, 0u, 0u, false, kInvalidId, kInvalidId, 0.f, 0.f}; }

// the queue without its head
__device__ __forceinline__ TopWalk top_pop(TopWalk t)
{
    t.todo0 = t.todo1, t.todo0_d = t.todo1_d, t.todo1 = kInvalidId;
    return t;
}

// The tail of a top-level step, after the caller's own test of the node's two children (h0, h1: which pass; far_first: both pass and
// child 1 goes first; i0, i1: word 7 of the two, the instances at level 1; d0, d1: their distances for the queue): down into the first
// child that passes, marking the other as owed; or, at level 1, the instances into the queue; or up to the nearest level that owes a
// child.
__device__ __forceinline__ TopWalk top_advance(TopWalk t, bool h0, bool h1, bool far_first, uint32_t i0, uint32_t i1, float d0, float d1)
{
    if (t.level > 1u)
    {
        if (h0 || h1)
        {
            if (h0 && h1) t.pending |= 1u << (t.level - 1u);
            t.idx   = 2u * t.idx + ((h0 && h1) ? (far_first ? 1u : 0u) : (h1 ? 1u : 0u));
            t.level = t.level - 1u;
            return t;
        }
    }
    else if (h0 || h1)
    {
        if (h0 && h1)
            t.todo0 = far_first ? i1 : i0, t.todo0_d = far_first ? d1 : d0, t.todo1 = far_first ? i0 : i1, t.todo1_d = far_first ? d0 : d1;
        else
            t.todo0 = h0 ? i0 : i1, t.todo0_d = h0 ? d0 : d1;
    }
    const uint32_t owed = t.pending >> t.level;
    if (owed == 0u)
    {
        t.done = true;
        return t;
    }
    const uint32_t up = (uint32_t)__builtin_ctz(owed);
    t.idx     = (t.idx >> up) ^ 1u;
    t.level   = t.level + up;
    t.pending = t.pending & ~(1u << t.level);
    return t;
}

// ---- launchers ----
// f(S) with S a stack class as a std::integral_constant; one dispatcher per list of classes that exists as kernels.
// The closest-point kernels' classes: the smallest that holds `depth` entries, a walk pushes at most one entry per level it descends
template <typename F>
void with_stack_class(uint32_t depth, F&& f)
{
    if (depth <= 16)
        f(std::integral_constant<int, 16>{});
    else if (depth <= 24)
        f(std::integral_constant<int, 24>{});
    else if (depth <= 32)
        f(std::integral_constant<int, 32>{});
    else
        f(std::integral_constant<int, 64>{});
}
// The scene's binary ray kernels: the context's stack size (LaunchCfg::stack_entries, chosen from the tree's depth), 32 or 64
template <typename F>
void with_binary_stack(const LaunchCfg& cfg, F&& f)
{
    if (cfg.stack_entries <= 32)
        f(std::integral_constant<int, 32>{});
    else
        f(std::integral_constant<int, 64>{});
}
// The instanced ray kernels: the bottom-level stack, bounded by the deepest object tree's depth.  An instanced object is usually small,
// and a 24-entry slice lets six workgroups share a CU's LDS where the 32-entry one of the plain binary kernels lets four.
template <typename F>
void with_instance_stack(const LaunchCfg& cfg, uint32_t depth, F&& f)
{
    if (depth <= 24 && cfg.stack_entries <= 32)
        f(std::integral_constant<int, 24>{});
    else
        with_binary_stack(cfg, f);
}
// f(K) with K the list capacity of pages of k records
template <typename F>
void with_k_bucket(uint32_t k, F&& f)
{
    switch (multi_bucket(k))
    {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
    }
}
template <typename F>
void with_flag(bool on, F&& f)
{
    if (on)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// One lane per query on the grid that is resident at once.  deferred: n is an upper bound, the count is on the device and is normally
// small -- one workgroup per CU at most.
template <auto Kernel, typename... Args>
void launch_lanes(const LaunchCfg& cfg, uint32_t n, bool deferred, const Args&... args)
{
    uint32_t want = (n + kBlock - 1) / kBlock;
    if (deferred && cfg.cu_count && want > cfg.cu_count) want = cfg.cu_count;
    if (want == 0) want = 1;
    hipLaunchKernelGGL(Kernel, dim3(resident_grid<Kernel>(cfg, want)), dim3(kBlock), 0, cfg.stream, args...);
}
template <auto Kernel, typename... Args>
void launch_points(const LaunchCfg& cfg, uint32_t n, const Args&... args)
{
    launch_lanes<Kernel>(cfg, n, false, args...);
}
}  // namespace
}  // namespace cap
