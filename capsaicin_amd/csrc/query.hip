// query.hip — ray queries of caller-supplied rays (cap_trace_rays / cap_trace_occlusion, their multi-hit and filtered forms) on the
// compressed 8-wide view (cap_wide.h), gfx950.
//
// The render's extension-ray kernel (trace8.hip k_trace_closest8) reads its rays from a class-partitioned queue; these kernels read the
// caller's CapRayDesc array instead, with no copy: a 32-B record is exactly the (origin, tmin) (direction, tmax) float4 pair the LDS ray
// buffer holds.  Everything else is the same form: one ray per lane, persistent waves, 64-ray chunks taken one chunk ahead from ONE
// linear work counter, lane refill from the wave's LDS buffer once CAP_W8_REFILL lanes are idle, while-while over node and triangle
// steps, the LDS + spill-slice pair stack.  Hit rule and boxes are those of the render (DESIGN.md "Intersection contract"), so a
// query's record is bit-identical to every other traversal of the build and to the oracle's brute force.
//
// Two things a caller's ray can do that the render's rays cannot:
//   * be degenerate (NaN or infinite origin / direction component, zero direction, tmax <= tmin or NaN): such a lane writes the miss
//     record at once and stays idle;
//   * start far outside the scene.  The wide boxes are padded for the quantised slab test's rounding error with origins near the
//     scene (wide_builder.cpp: error <= eps |1/d| (|o| + |p - o| + 2 |P - o|), padding kWidePad * M).  With every origin component
//     within kQuerySafeScale * M the error is at most eps |1/d| (4 * 4 M + 3 M) = 19 eps M |1/d|, below the padding's 33.5 eps M |1/d|.
//     A ray whose origin lies beyond is not traced here: its index goes to a list that the binary tree's kernel (kernels.hip
//     k_query_binary, whose slab test carries its own relative slack) answers right behind this launch.
//
// Each step is written once: the feed, the set-up, the load sequence and the tail of the three wide bodies below (closest / first,
// occlusion, multi-hit) as helpers of this file; the binary tree's node step and pop, and the dispatch from run-time values to
// instantiations, in cap_query_walk.h, shared with instance.hip and point_query.hip.  Leaf and triangle handling stay in the bodies:
// what a triangle is offered to is what they differ in.  k_query_binary_multi and k_query_binary_multi_f alone keep their own
// loops (see there).
#include "cap_hit_list.h"
#include "cap_kernels.h"
#include "cap_query_walk.h"
#include "cap_wide_trace.h"

namespace cap
{
#ifndef CAP_W8_LDS
#define CAP_W8_LDS 8  // LDS stack entries (8 B) per lane: the value trace8.hip uses (the host checks the tree depth against it)
#endif
#ifndef CAP_W8_BLOCKS
#define CAP_W8_BLOCKS 6
#endif
#ifndef CAP_W8_REFILL
#define CAP_W8_REFILL 16
#endif
constexpr int kQueryLds = CAP_W8_LDS;

// CapRayDesc of ray i: rays[2 i] = (origin, tmin), rays[2 i + 1] = (direction, tmax)
__device__ __forceinline__ bool query_origin_safe(const float4 a, float safe)
{
    return fabsf(a.x) <= safe && fabsf(a.y) <= safe && fabsf(a.z) <= safe;
}

// The feed: wave-uniform chunk starts from work[0], the next chunk one ahead in registers (pa, pb), the current one parked in LDS (rbuf).
struct QueryFeedState
{
    uint32_t grab, pend_n, pend_base, buf_n, buf_pos, buf_base;
    float4   pa, pb;
};

__device__ __forceinline__ void query_fetch(QueryFeedState& s, const QueryArgs& q, uint32_t lane)
{
    const uint32_t start = grab_value(s.grab) * 64u;
    s.pend_n             = 0;
    if (start >= q.n) return;  // the feed has ended
    s.pend_n    = q.n - start < 64u ? q.n - start : 64u;
    s.pend_base = start;
    if (lane < s.pend_n) s.pa = q.rays[2 * (size_t)(start + lane)], s.pb = q.rays[2 * (size_t)(start + lane) + 1];
    s.grab = grab_issue(q.work, 0);
}

// Hands the rest of the parked chunk (then, once, the start of the next one) to the idle lanes of the wave; take_ray(org_tmin, dir_tmax,
// ray index) runs on every lane that gets a ray and returns whether the lane now traces it.
template <typename Take>
__device__ __forceinline__ void query_refill(QueryFeedState& s, const QueryArgs& q, float4* rbuf, uint32_t lane, bool& alive,
                                             unsigned long long& m_alive, Take take_ray)
{
    for (int rep = 0; rep < 2; ++rep)
    {
        if (s.buf_pos >= s.buf_n)
        {
            if (s.pend_n == 0) break;
            if (lane < s.pend_n) rbuf[lane] = s.pa, rbuf[64u + lane] = s.pb;
            s.buf_n = s.pend_n, s.buf_pos = 0, s.buf_base = s.pend_base;
            query_fetch(s, q, lane);
            wave_handoff();
        }
        const unsigned long long idle = ~m_alive;
        const uint32_t n_idle = (uint32_t)__popcll(idle), avail = s.buf_n - s.buf_pos;
        const uint32_t take   = avail < n_idle ? avail : n_idle;
        const uint32_t rank   = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
        if (!alive && rank < take)
        {
            const uint32_t e = s.buf_pos + rank;
            alive            = take_ray(rbuf[e], rbuf[64u + e], s.buf_base + e);
        }
        s.buf_pos += take;
        m_alive = __ballot(alive);
        if (m_alive == ~0ull) break;
    }
}

// A lane's ray that the wide walk does not trace: a degenerate ray, answered by write_miss(), or a ray for the binary tree, whose index
// goes to the list.  Returns whether the wide walk takes it.
template <typename Miss>
__device__ __forceinline__ bool query_admit(const QueryArgs& q, float4 a, float4 b, uint32_t out, Miss write_miss)
{
    if (!query_ray_ok(a, b))
    {
        write_miss();
        return false;
    }
    if (!query_origin_safe(a, q.safe))
    {
        q.defer[atomicAdd(q.work + kCounterStride, 1u)] = out;
        return false;
    }
    return true;
}

// ---- what the three wide bodies below share ----
// A lane's state stays in the kernel's own variables and crosses these helpers by reference: gathered into one struct, even with every
// step written out in the kernel, k_query_closest8 spilled 24 bytes instead of 12 (DESIGN.md "Ray queries", "One copy of each step").
// With these forms the three plain and the two filtered single-hit kernels compile to the parent's instruction counts.
// Feed and stack set-up: the first chunk is on its way, every lane idle at the root.
__device__ __forceinline__ void wide_start(const BvhDev& bvh, const QueryArgs& q, uint32_t& lane, float4*& rbuf, QueryFeedState& s, WideStack<kQueryLds>& st,
                                           bool& alive, Ray& r, WideRay& w, WideCursor& c)
{
    __shared__ uint2  lds_stack[kQueryLds * kBlock];
    __shared__ float4 lds_rays[2 * kBlock];  // per wave: 64 x (origin, tmin) then 64 x (direction, tmax)
    lane = threadIdx.x & 63u;
    rbuf = lds_rays + (threadIdx.x >> 6) * 128u;
    s    = QueryFeedState{grab_issue(q.work, 0), 0, 0, 0, 0, 0, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    query_fetch(s, q, lane);
    st    = WideStack<kQueryLds>{lds_stack + threadIdx.x, wide_spill_of_thread(bvh), 0};
    alive = false;
    r     = make_ray(mk3(0, 0, 0), mk3(0, 0, 1), 0.f, 0.f);
    w     = make_wide_ray(r.o, r.d);
    wide_cursor_root(c);
}

// The ray (a, b) starts at the root
__device__ __forceinline__ void wide_take(float4 a, float4 b, Ray& r, WideRay& w, WideCursor& c, WideStack<kQueryLds>& st)
{
    r = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
    w = make_wide_ray(r.o, r.d);
    wide_cursor_root(c);
    st.sp = 0;
}

__device__ __forceinline__ bool wide_feed_ended(const QueryFeedState& s) { return s.buf_pos >= s.buf_n && s.pend_n == 0; }

// Pick the source, push the rest, load the record: one load sequence serves node and triangle lanes (see k_trace_closest8).  oct: the
// visiting order, w.octinv or kAnyOct of it.  TRI48: a triangle lane reads 48 of its record's 64 bytes (the plain occlusion test needs no id).
template <bool TRI48>
__device__ __forceinline__ void wide_load(const BvhDev& bvh, uint32_t oct, bool alive, bool tri_lane, bool node_lane, WideCursor& c, WideStack<kQueryLds>& st,
                                          WideNode& nd)
{
    const float4* src = bvh.nodes8;
    if (tri_lane)
        src = bvh.tris8 + 4 * (size_t)wide_pick_triangle(c);
    else if (node_lane)
    {
        bool           rest;
        const uint32_t node = wide_pick_child(c, oct, rest);
        if (rest) st.push(c.g_base, c.g_mask);
        src = bvh.nodes8 + (kWideNodeStride / 4u) * (size_t)node;
    }
#define CAP_DEF4(v) asm volatile("" : "=v"((v).x), "=v"((v).y), "=v"((v).z), "=v"((v).w))  // (see k_trace_closest8)
    CAP_DEF4(nd.h0);
    CAP_DEF4(nd.h1);
    CAP_DEF4(nd.q2);
    CAP_DEF4(nd.q3);
    CAP_DEF4(nd.q4);
#undef CAP_DEF4
    if (alive)
    {
        nd.h0 = src[0], nd.h1 = src[1], nd.q2 = src[2];
        if (!TRI48) nd.q3 = src[3];
    }
    if (node_lane)
    {
        if (TRI48) nd.q3 = src[3];
        nd.q4 = src[4];
    }
}

// The tail: a live lane with neither triangles nor children due takes the next stack entry; with none left write_out() stores its
// answer and the lane retires.  The write-out is a parameter so that the branches nest as the bodies always had them: with a helper
// that returns "write now" the list kernels were allocated anew (one more VGPR) and ran up to a quarter faster at K = 16 -- a
// register-allocation effect that wants a change of its own, DESIGN.md.
template <typename Write>
__device__ __forceinline__ void wide_retire_or_pop(bool& alive, WideCursor& c, WideStack<kQueryLds>& st, Write write_out)
{
    if (alive && c.t_hits == 0u && (c.g_mask >> 24) == 0u)
    {
        if (st.sp == 0)
        {
            write_out();
            alive = false;
        }
        else
            st.pop(c);
    }
}

// Ray flags and instance masks (cap_trace_*_ex): every kernel of this file exists in a plain and a filtered (_f) form; the wide ones
// are made from one body, FILTER a template flag, and the plain kernels are instruction for instruction what they were without it.
// The cull sits inside the triangle test (tri_test_cull); the mask byte of a triangle is read only once the triangle has passed that test, and only when the
// call filters by mask (wave-uniform branch).  A rejected triangle is as if it were not in the scene: it never reaches best_t, the
// list or the count, so nothing is pruned by it.
__device__ __forceinline__ bool filter_admits(const RayFilter& f, uint32_t gid) { return !f.tri_mask || (f.tri_mask[gid] & f.mask) != 0u; }

template <bool FILTER>
__device__ __forceinline__ bool query_tri_test(const Ray& r, const float4 t0, const float4 t1, const float4 t2, const RayFilter& f, float& t,
                                               float& u, float& v)
{
    if constexpr (FILTER)
        return tri_test_cull(r, t0, t1, t2, f.cull_and, f.cull_xor, t, u, v);
    else
        return tri_test(r, t0, t1, t2, t, u, v);
}

// Closest hit: CapHit (t, u, v, asfloat(triangle)) per ray; a miss is (tmax, 0, 0, ~0).  FIRST (CAP_RAY_FLAG_ACCEPT_FIRST_HIT): the
// lane writes the first hit it accepts and retires, as k_query_any8's lanes do at their first occluder.
template <bool FILTER, bool FIRST>
__device__ __forceinline__ void query_closest8(const BvhDev& bvh, const QueryArgs& q, uint32_t refill_idle, const RayFilter& f)
{
    float4* const        hits = static_cast<float4*>(q.out);
    uint32_t             lane, out = 0;
    float4*              rbuf;
    QueryFeedState       s;
    WideStack<kQueryLds> st;
    bool                 alive;
    Ray                  r;
    WideRay              w;
    WideCursor           c;
    wide_start(bvh, q, lane, rbuf, s, st, alive, r, w, c);
    float    best_t = 0.f, best_u = 0.f, best_v = 0.f;
    uint32_t best_gid = kInvalidId;
    while (true)
    {
        unsigned long long m_alive = __ballot(alive);
        if (64u - (uint32_t)__popcll(m_alive) >= refill_idle)
            query_refill(s, q, rbuf, lane, alive, m_alive, [&](float4 a, float4 b, uint32_t i) {
                if (!query_admit(q, a, b, i, [&] { hits[i] = make_float4(b.w, 0.f, 0.f, u2f(kInvalidId)); })) return false;
                wide_take(a, b, r, w, c, st);
                out = i;
                best_t = r.tmax, best_u = 0.f, best_v = 0.f, best_gid = kInvalidId;
                return true;
            });
        if (m_alive == 0ull)
        {
            if (wide_feed_ended(s)) break;  // feed ended and every lane retired
            continue;
        }
        const bool tri_lane = alive && c.t_hits != 0u, node_lane = alive && c.t_hits == 0u;
        WideNode   nd;
        wide_load<false>(bvh, w.octinv, alive, tri_lane, node_lane, c, st, nd);
        if (tri_lane)
        {
            float t, u, v;
            if (query_tri_test<FILTER>(r, nd.h0, nd.h1, nd.q2, f, t, u, v))
            {
                const uint32_t gid = f2u(nd.q3.x);
                if (!FILTER || filter_admits(f, gid))
                {
                    if (FIRST)
                    {
                        hits[out] = make_float4(t, u, v, u2f(gid));
                        alive     = false;
                    }
                    else if (t < best_t || (t == best_t && gid < best_gid))
                        best_t = t, best_u = u, best_v = v, best_gid = gid;
                }
            }
        }
        if (node_lane) wide_node_test(nd, w, r.tmin, best_t, c);
        wide_retire_or_pop(alive, c, st, [&] { hits[out] = make_float4(best_t, best_u, best_v, u2f(best_gid)); });
    }
}

__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_closest8(BvhDev bvh, QueryArgs q, uint32_t refill_idle)
{
    query_closest8<false, false>(bvh, q, refill_idle, RayFilter{});
}
__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_closest8_f(BvhDev bvh, QueryArgs q, uint32_t refill_idle, RayFilter f)
{
    query_closest8<true, false>(bvh, q, refill_idle, f);
}
__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_first8_f(BvhDev bvh, QueryArgs q, uint32_t refill_idle, RayFilter f)
{
    query_closest8<true, true>(bvh, q, refill_idle, f);
}

// Occlusion: 1 when some triangle has tmin det < T < tmax det (tri_occludes), else 0, one word per ray.  The lane-refill form of
// k_trace_any8_refill with the caller's rays: per-lane octant (caller rays share no light direction), back-to-front visiting order
// (kAnyOrder) and early exit at the first occluder.  FILTER: a triangle lane reads all 64 bytes of its record, for the id in word 12.
template <bool FILTER>
__device__ __forceinline__ void query_any8(const BvhDev& bvh, const QueryArgs& q, uint32_t refill_idle, const RayFilter& f)
{
    uint32_t* const      occ = static_cast<uint32_t*>(q.out);
    uint32_t             lane, out = 0;
    float4*              rbuf;
    QueryFeedState       s;
    WideStack<kQueryLds> st;
    bool                 alive;
    Ray                  r;
    WideRay              w;
    WideCursor           c;
    wide_start(bvh, q, lane, rbuf, s, st, alive, r, w, c);
    while (true)
    {
        unsigned long long m_alive = __ballot(alive);
        if (64u - (uint32_t)__popcll(m_alive) >= refill_idle)
            query_refill(s, q, rbuf, lane, alive, m_alive, [&](float4 a, float4 b, uint32_t i) {
                if (!query_admit(q, a, b, i, [&] { occ[i] = 0u; })) return false;
                wide_take(a, b, r, w, c, st);
                out = i;
                return true;
            });
        if (m_alive == 0ull)
        {
            if (wide_feed_ended(s)) break;
            continue;
        }
        const bool tri_lane = alive && c.t_hits != 0u, node_lane = alive && c.t_hits == 0u;
        WideNode   nd;
        wide_load<!FILTER>(bvh, kAnyOct(w.octinv), alive, tri_lane, node_lane, c, st, nd);
        bool occluded = false;
        if constexpr (FILTER)
        {
            if (tri_lane) occluded = tri_occludes_cull(r, nd.h0, nd.h1, nd.q2, f.cull_and, f.cull_xor);
            if (occluded) occluded = filter_admits(f, f2u(nd.q3.x));
        }
        else if (tri_lane)
            occluded = tri_occludes(r, nd.h0, nd.h1, nd.q2);
        if (node_lane) wide_node_test<kAnyOrder>(nd, w, r.tmin, r.tmax, c);
        if (occluded)
        {
            occ[out] = 1u;
            alive    = false;
        }
        else
            wide_retire_or_pop(alive, c, st, [&] { occ[out] = 0u; });
    }
}

__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_any8(BvhDev bvh, QueryArgs q, uint32_t refill_idle)
{
    query_any8<false>(bvh, q, refill_idle, RayFilter{});
}
__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_any8_f(BvhDev bvh, QueryArgs q, uint32_t refill_idle, RayFilter f)
{
    query_any8<true>(bvh, q, refill_idle, f);
}

bool query8_stack_matches() { return (uint32_t)kQueryLds + kSpillEntries / 2u == wide8_stack_pairs(); }

// ---- launching the wide kernels ----
// The refill threshold (clamped as trace8.hip w8_refill_idle does)
static uint32_t query_refill_idle(const LaunchCfg& cfg)
{
    const long v = (long)cfg.sw_get(SW_W8_REFILL, CAP_W8_REFILL);
    return (uint32_t)(v < 1 ? 1 : v > 64 ? 64 : v);
}

// The persistent grid: one workgroup per kBlock rays, at most per_cu a CU, and no more threads than there are spill slices
static uint32_t wide_query_grid(const LaunchCfg& cfg, const BvhDev& bvh, uint32_t n, int per_cu)
{
    uint32_t g   = (n + kBlock - 1) / kBlock;
    uint32_t cap = cfg.cu_count ? cfg.cu_count * (uint32_t)per_cu : cfg.grid_blocks;
    if ((uint64_t)cap * kBlock > bvh.spill_threads) cap = bvh.spill_threads / kBlock;  // every thread owns a spill slice
    if (g > cap) g = cap;
    return g ? g : 1;
}

// Kernel(bvh, a, refill_idle[, filter]) over the n rays of a
template <auto Kernel, typename Args, typename... Filter>
static void launch_wide(const LaunchCfg& cfg, const BvhDev& bvh, int per_cu, const Args& a, uint32_t n, const Filter&... f)
{
    hipLaunchKernelGGL(Kernel, dim3(wide_query_grid(cfg, bvh, n, per_cu)), dim3(kBlock), 0, cfg.stream, bvh, a, query_refill_idle(cfg), f...);
}

void launch_query8(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, bool any, const RayFilter* f, bool first_hit)
{
    if (!f)
    {
        if (any)
            launch_wide<k_query_any8>(cfg, bvh, CAP_W8_BLOCKS, q, q.n);
        else
            launch_wide<k_query_closest8>(cfg, bvh, CAP_W8_BLOCKS, q, q.n);
    }
    else if (any)
        launch_wide<k_query_any8_f>(cfg, bvh, CAP_W8_BLOCKS, q, q.n, *f);
    else if (first_hit)
        launch_wide<k_query_first8_f>(cfg, bvh, CAP_W8_BLOCKS, q, q.n, *f);
    else
        launch_wide<k_query_closest8_f>(cfg, bvh, CAP_W8_BLOCKS, q, q.n, *f);
}

// ---- multi-hit queries (cap_trace_rays_multi) ----
// A ray's first k hits in (t, triangle) order, its hit count, or both.  Each lane keeps a sorted list of K (t, gid) pairs in VGPRs, K a
// compile-time bucket >= k; every index into it is a compile-time constant, so it never goes to scratch.  The first K - k slots hold
// (-inf, 0) placeholders, the last k start as the miss (tmax, ~0).  A hit below slot K - 1 replaces it and bubbles towards the front by
// K - 1 compare-swaps; no hit (t > tmin >= -inf) ever passes a placeholder.  Slot K - 1 is the pruning bound: tmax until the list
// holds k hits, then the k-th.  Both box tests keep a child whose interval touches [lower bound, bound] (wide_node_test's differences
// are negative only for a strict miss, slab is inclusive), so a box entered exactly at the k-th t is still opened and an equal-t
// triangle with a lower id still displaces the k-th entry: the list is exact whatever the visiting order.
// Paging (CAP_MULTI_CONTINUE): a hit is counted only above the cursor (t_c, g_c) read from slot k - 1 of the page, (-inf, 0) otherwise.
// Hits below the cursor's t lie outside every page after it, so the box tests may take max(tmin, t_c) as their lower bound: still
// inclusive, a triangle at t_c with a higher id is kept.  The list itself is HitList<K> of cap_hit_list.h.

// The hit (t, gid) of the contract's rule, against a ray's cursor and list.  COUNT: every hit above the cursor adds one.
template <int K, bool COUNT>
__device__ __forceinline__ void multi_offer(HitList<K>& L, uint32_t& count, float tc, uint32_t gc, float t, uint32_t gid)
{
    if (t > tc || (t == tc && gid > gc))
    {
        if (COUNT) ++count;
        if (L.admits(t, gid)) L.insert(t, gid);
    }
}

// The cursor of ray i: slot k - 1 of its page when paging, else (-inf, 0), below every hit.
__device__ __forceinline__ void multi_cursor(const MultiArgs& m, uint32_t i, float& tc, uint32_t& gc)
{
    tc = -__builtin_inff(), gc = 0u;
    if (m.resume)
    {
        const float4 e = static_cast<const float4*>(m.q.out)[(size_t)i * m.k + (m.k - 1u)];
        tc = e.x, gc = f2u(e.w);
    }
}

// A ray the traversal does not answer: k miss records (tmax, 0, 0, ~0) and count 0.
__device__ __forceinline__ void multi_write_miss(const MultiArgs& m, uint32_t i, float tmax)
{
    if (m.counts) m.counts[i] = 0u;
    float4* const page = static_cast<float4*>(m.q.out) + (size_t)i * m.k;
    for (uint32_t j = 0; j < m.k; ++j) page[j] = make_float4(tmax, 0.f, 0.f, u2f(kInvalidId));
}

// Writes ray i's page and count.  (u, v) are not kept in the list (2K registers instead of 4K): the winner's record is tested again
// from bvh.tris_by_id, the records in global id order.  tris8 (and the binary tree's tris) are byte copies of those records
// (tri_raw -> tris_sorted -> k_gather_wide, and again after cap_bvh_refit), and tri_test on the same ray and record gives the same
// bits, so the t found here is the listed one and (u, v) are those of the traversal.
template <int K, bool COUNT>
__device__ __forceinline__ void multi_write(const MultiArgs& m, const BvhDev& bvh, uint32_t i, const Ray& r, const HitList<K>& L, uint32_t count)
{
    if (COUNT) m.counts[i] = count;
    float4* const page = static_cast<float4*>(m.q.out) + (size_t)i * m.k;
    const int     skip = K - (int)m.k;  // the placeholders
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j >= skip)
        {
            float u = 0.f, v = 0.f;
            if (L.g[j] != kInvalidId)
            {
                const float4* rec = bvh.tris_by_id + 4 * (size_t)L.g[j];
                float         t;
                tri_test(r, rec[0], rec[1], rec[2], t, u, v);
            }
            page[j - skip] = make_float4(L.t[j], u, v, u2f(L.g[j]));
        }
}

// Workgroups per CU each K is register-allocated for (waves per SIMD; VGPRs 512 / waves): k_query_closest8 runs six (80 VGPRs, with a
// spill); with the list, the cursor and the count the most that leave every instantiation without scratch (tools/kernel_regs.sh) are
// 5 (96) at K = 1, 4 (128) at K = 4, 3 (168) at K = 8 and 2 (256) at K = 16.
constexpr int multi8_blocks(int K) { return K <= 1 ? 5 : K <= 4 ? 4 : K <= 8 ? 3 : 2; }

// Multi-hit on the wide tree: k_query_closest8's feed, refill, pair stack and hand-over of far origins, with the list instead of the
// single best record.
template <int K, bool COUNT, bool FILTER>
__device__ __forceinline__ void query_multi8(const BvhDev& bvh, const MultiArgs& m, uint32_t refill_idle, const RayFilter& f)
{
    const QueryArgs&     q = m.q;
    uint32_t             lane, out = 0;
    float4*              rbuf;
    QueryFeedState       s;
    WideStack<kQueryLds> st;
    bool                 alive;
    Ray                  r;
    WideRay              w;
    WideCursor           c;
    wide_start(bvh, q, lane, rbuf, s, st, alive, r, w, c);
    HitList<K> L;
    L.init(m.k, 0.f);
    float    tc = 0.f, lo = 0.f;
    uint32_t gc = 0u, count = 0u;
    while (true)
    {
        unsigned long long m_alive = __ballot(alive);
        if (64u - (uint32_t)__popcll(m_alive) >= refill_idle)
            query_refill(s, q, rbuf, lane, alive, m_alive, [&](float4 a, float4 b, uint32_t i) {
                if (!query_admit(q, a, b, i, [&] { multi_write_miss(m, i, b.w); })) return false;
                wide_take(a, b, r, w, c, st);
                out = i;
                L.init(m.k, r.tmax);
                multi_cursor(m, i, tc, gc);
                lo    = fmaxf(r.tmin, tc);
                count = 0u;
                return true;
            });
        if (m_alive == 0ull)
        {
            if (wide_feed_ended(s)) break;
            continue;
        }
        const bool tri_lane = alive && c.t_hits != 0u, node_lane = alive && c.t_hits == 0u;
        WideNode   nd;
        wide_load<false>(bvh, w.octinv, alive, tri_lane, node_lane, c, st, nd);
        if (tri_lane)
        {
            float t, u, v;
            if (query_tri_test<FILTER>(r, nd.h0, nd.h1, nd.q2, f, t, u, v) && (!FILTER || filter_admits(f, f2u(nd.q3.x))))
                multi_offer<K, COUNT>(L, count, tc, gc, t, f2u(nd.q3.x));
        }
        if (node_lane) wide_node_test(nd, w, lo, COUNT ? r.tmax : L.t[K - 1], c);
        wide_retire_or_pop(alive, c, st, [&] { multi_write<K, COUNT>(m, bvh, out, r, L, count); });
    }
}

template <int K, bool COUNT>
__global__ __launch_bounds__(kBlock, multi8_blocks(K)) void k_query_multi8(BvhDev bvh, MultiArgs m, uint32_t refill_idle)
{
    query_multi8<K, COUNT, false>(bvh, m, refill_idle, RayFilter{});
}
template <int K, bool COUNT>
__global__ __launch_bounds__(kBlock, multi8_blocks(K)) void k_query_multi8_f(BvhDev bvh, MultiArgs m, uint32_t refill_idle, RayFilter f)
{
    query_multi8<K, COUNT, true>(bvh, m, refill_idle, f);
}

// Multi-hit on the binary tree, one lane per ray: traverse_closest's loop (kernels.hip) with the list; every ray where the wide view
// is not used, and the rays k_query_multi8 handed over.  Workgroups per CU as the binary query kernels (stack_residency: 4 with
// 32-entry stacks, 2 with 64), except K = 16 on 32 entries: 3, for the registers.
// These two kernels keep the node step and the pop written out, and stay two: their code is a knife-edge of the compiler.  Any other
// spelling -- ray_node_step, ray_pop alone in place of the two pop lines, the step's arguments by value, one body with a FILTER
// flag -- yields one and the same other allocation (K = 16: 113 VGPRs instead of 136, so four workgroups per CU instead of three)
// and schedule: measured on the hall without the wide view, K = 16 ran 0.68-0.72 of the parent's time, K = 1 1.07-1.19 and counts
// 1.04-1.13 on the incoherent ray sets.  A refactor takes neither (DESIGN.md "Ray queries", "One copy of each step").
constexpr int multi_binary_blocks(int STACK, int K) { return STACK <= 32 ? (K <= 8 ? 4 : 3) : 2; }

template <int STACK, int K, bool COUNT>
__global__ __launch_bounds__(kBlock, multi_binary_blocks(STACK, K)) void k_query_binary_multi(BvhDev bvh, MultiArgs m, uint32_t deferred)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    const QueryArgs&    q     = m.q;
    const uint32_t      n     = deferred ? q.work[kCounterStride] : q.n;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock)
    {
        const uint32_t i = deferred ? q.defer[j] : j;
        const float4   a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];
        if (!query_ray_ok(a, b))
        {
            multi_write_miss(m, i, b.w);
            continue;
        }
        const Ray  r = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
        HitList<K> L;
        L.init(m.k, r.tmax);
        float    tc;
        uint32_t gc, count = 0u;
        multi_cursor(m, i, tc, gc);
        Ray rb  = r;  // the box tests' interval: lower bound max(tmin, t_c)
        rb.tmin = fmaxf(r.tmin, tc);
        int node = bvh.root, sp = 0;
        while (bvh.tri_count != 0u)
        {
            const float tfar = COUNT ? r.tmax : L.t[K - 1];
            if (node >= 0)
            {
                const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                             q3 = bvh.nodes[4 * node + 3];
                float      tn0, tn1;
                const bool h0 = slab(rb, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tfar, tn0);
                const bool h1 = slab(rb, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tfar, tn1);
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
                const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                for (uint32_t leaf = first; leaf <= last; ++leaf)
                {
                    const float4 t0 = bvh.tris[4 * leaf + 0], t1 = bvh.tris[4 * leaf + 1], t2 = bvh.tris[4 * leaf + 2];
                    float        t, u, v;
                    if (tri_test(r, t0, t1, t2, t, u, v)) multi_offer<K, COUNT>(L, count, tc, gc, t, f2u(bvh.tris[4 * leaf + 3].x));
                }
            }
            if (sp == 0) break;
            node = (int)stack[(--sp) * kBlock];
        }
        multi_write<K, COUNT>(m, bvh, i, r, L, count);
    }
}

// k_query_binary_multi under a filter (cap_trace_rays_multi_ex): the same loop with tri_test_cull and the mask in the leaf.  A kernel
// of its own rather than a second instantiation of one body, for the reason above.
template <int STACK, int K, bool COUNT>
__global__ __launch_bounds__(kBlock, multi_binary_blocks(STACK, K)) void k_query_binary_multi_f(BvhDev bvh, MultiArgs m, uint32_t deferred, RayFilter f)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    const QueryArgs&    q     = m.q;
    const uint32_t      n     = deferred ? q.work[kCounterStride] : q.n;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock)
    {
        const uint32_t i = deferred ? q.defer[j] : j;
        const float4   a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];
        if (!query_ray_ok(a, b))
        {
            multi_write_miss(m, i, b.w);
            continue;
        }
        const Ray  r = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
        HitList<K> L;
        L.init(m.k, r.tmax);
        float    tc;
        uint32_t gc, count = 0u;
        multi_cursor(m, i, tc, gc);
        Ray rb  = r;  // the box tests' interval: lower bound max(tmin, t_c)
        rb.tmin = fmaxf(r.tmin, tc);
        int node = bvh.root, sp = 0;
        while (bvh.tri_count != 0u)
        {
            const float tfar = COUNT ? r.tmax : L.t[K - 1];
            if (node >= 0)
            {
                const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2],
                             q3 = bvh.nodes[4 * node + 3];
                float      tn0, tn1;
                const bool h0 = slab(rb, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tfar, tn0);
                const bool h1 = slab(rb, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tfar, tn1);
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
                const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                for (uint32_t leaf = first; leaf <= last; ++leaf)
                {
                    const float4 t0 = bvh.tris[4 * leaf + 0], t1 = bvh.tris[4 * leaf + 1], t2 = bvh.tris[4 * leaf + 2];
                    float        t, u, v;
                    if (!tri_test_cull(r, t0, t1, t2, f.cull_and, f.cull_xor, t, u, v)) continue;
                    const uint32_t gid = f2u(bvh.tris[4 * leaf + 3].x);
                    if (filter_admits(f, gid)) multi_offer<K, COUNT>(L, count, tc, gc, t, gid);
                }
            }
            if (sp == 0) break;
            node = (int)stack[(--sp) * kBlock];
        }
        multi_write<K, COUNT>(m, bvh, i, r, L, count);
    }
}

// Closest / first / occlusion on the binary tree under a filter, one lane per ray: k_query_binary's place (kernels.hip) for the _ex
// calls -- every ray where the wide view is not used, and the rays the filtered wide kernels handed over.  The loop is
// traverse_closest's over ray_node_step / ray_pop (cap_query_walk.h), with tri_test_cull and the mask in front of the best record.  MODE 0: closest; 1: first accepted hit ends the
// walk; 2: occlusion (tri_occludes_cull, the division-free interval; the visiting order does not change the answer).
template <int STACK, int MODE>
__global__ __launch_bounds__(kBlock, multi_binary_blocks(STACK, 1)) void k_query_binary_f(BvhDev bvh, QueryArgs q, uint32_t deferred, RayFilter f)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    const uint32_t      n     = deferred ? q.work[kCounterStride] : q.n;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock)
    {
        const uint32_t i = deferred ? q.defer[j] : j;
        const float4   a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];
        const Ray      r = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
        float          best_t = b.w, best_u = 0.f, best_v = 0.f;
        uint32_t       best_gid = kInvalidId;
        bool           found = false;  // MODE 1, 2: the walk is over
        int            node = bvh.root, sp = 0;
        const bool     ok = query_ray_ok(a, b);
        while (ok && bvh.tri_count != 0u)
        {
            if (node >= 0)
            {
                if (ray_node_step<STACK>(bvh, r, best_t, stack, node, sp)) continue;
            }
            else
            {
                const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                for (uint32_t leaf = first; leaf <= last && !found; ++leaf)
                {
                    const float4 t0 = bvh.tris[4 * leaf + 0], t1 = bvh.tris[4 * leaf + 1], t2 = bvh.tris[4 * leaf + 2];
                    float        t = 0.f, u = 0.f, v = 0.f;
                    const bool   hit = MODE == 2 ? tri_occludes_cull(r, t0, t1, t2, f.cull_and, f.cull_xor)
                                                 : tri_test_cull(r, t0, t1, t2, f.cull_and, f.cull_xor, t, u, v);
                    if (!hit) continue;
                    const uint32_t gid = f2u(bvh.tris[4 * leaf + 3].x);
                    if (!filter_admits(f, gid)) continue;
                    if (MODE != 0)
                        best_t = t, best_u = u, best_v = v, best_gid = gid, found = true;
                    else if (t < best_t || (t == best_t && gid < best_gid))
                        best_t = t, best_u = u, best_v = v, best_gid = gid;
                }
                if (found) break;
            }
            if (!ray_pop(stack, sp, node)) break;
        }
        if (MODE == 2)
            static_cast<uint32_t*>(q.out)[i] = found ? 1u : 0u;
        else
            static_cast<float4*>(q.out)[i] = make_float4(best_t, best_u, best_v, u2f(best_gid));
    }
}

uint32_t multi_bucket(uint32_t k) { return k <= 1 ? 1u : k <= 4 ? 4u : k <= 8 ? 8u : 16u; }

void launch_query8_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, const RayFilter* f)
{
    with_k_bucket(m.k, [&](auto K) {
        with_flag(m.counts != nullptr, [&](auto COUNT) {
            constexpr int  k = decltype(K)::value;
            constexpr bool c = decltype(COUNT)::value;
            if (f)
                launch_wide<k_query_multi8_f<k, c>>(cfg, bvh, multi8_blocks(k), m, m.q.n, *f);
            else
                launch_wide<k_query_multi8<k, c>>(cfg, bvh, multi8_blocks(k), m, m.q.n);
        });
    });
}

// The binary kernels, one lane per ray (launch_lanes: `deferred` caps the grid of a handed-over list)
void launch_query_binary_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, bool deferred, const RayFilter* f)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    with_binary_stack(cfg, [&](auto S) {
        with_k_bucket(m.k, [&](auto K) {
            with_flag(m.counts != nullptr, [&](auto COUNT) {
                constexpr int  s = decltype(S)::value, k = decltype(K)::value;
                constexpr bool c = decltype(COUNT)::value;
                if (f)
                    launch_lanes<k_query_binary_multi_f<s, k, c>>(cfg, m.q.n, deferred, b, m, deferred ? 1u : 0u, *f);
                else
                    launch_lanes<k_query_binary_multi<s, k, c>>(cfg, m.q.n, deferred, b, m, deferred ? 1u : 0u);
            });
        });
    });
}

void launch_query_binary_filtered(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, const RayFilter& f, bool any, bool first_hit, bool deferred)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    with_binary_stack(cfg, [&](auto S) {
        constexpr int s = decltype(S)::value;
        if (any)
            launch_lanes<k_query_binary_f<s, 2>>(cfg, q.n, deferred, b, q, deferred ? 1u : 0u, f);
        else if (first_hit)
            launch_lanes<k_query_binary_f<s, 1>>(cfg, q.n, deferred, b, q, deferred ? 1u : 0u, f);
        else
            launch_lanes<k_query_binary_f<s, 0>>(cfg, q.n, deferred, b, q, deferred ? 1u : 0u, f);
    });
}
}  // namespace cap
