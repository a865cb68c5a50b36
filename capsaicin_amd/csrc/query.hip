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
#include "cap_hit_list.h"
#include "cap_kernels.h"
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

// A lane's ray that the wide walk does not trace: the miss record of a degenerate ray, or the index of a ray for the binary tree.
// Returns whether the wide walk takes it.
template <bool ANY>
__device__ __forceinline__ bool query_admit(const QueryArgs& q, float4 a, float4 b, uint32_t out)
{
    if (!query_ray_ok(a, b))
    {
        if (ANY)
            static_cast<uint32_t*>(q.out)[out] = 0u;
        else
            static_cast<float4*>(q.out)[out] = make_float4(b.w, 0.f, 0.f, u2f(kInvalidId));
        return false;
    }
    if (!query_origin_safe(a, q.safe))
    {
        q.defer[atomicAdd(q.work + kCounterStride, 1u)] = out;
        return false;
    }
    return true;
}

// Ray flags and instance masks (cap_trace_*_ex): every kernel of this file exists in a plain and a filtered (_f) form; the wide ones
// are made from one body, FILTER a template flag, and the plain kernels are instruction for instruction what they were without it.  The cull sits inside the
// triangle test (tri_test_cull); the mask byte of a triangle is read only once the triangle has passed that test, and only when the
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
    __shared__ uint2  lds_stack[kQueryLds * kBlock];
    __shared__ float4 lds_rays[2 * kBlock];  // per wave: 64 x (origin, tmin) then 64 x (direction, tmax)
    const uint32_t lane = threadIdx.x & 63u;
    float4* const  rbuf = lds_rays + (threadIdx.x >> 6) * 128u;
    float4* const  hits = static_cast<float4*>(q.out);
    QueryFeedState s{grab_issue(q.work, 0), 0, 0, 0, 0, 0, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    query_fetch(s, q, lane);

    WideStack<kQueryLds> st{lds_stack + threadIdx.x, wide_spill_of_thread(bvh), 0};
    bool              alive = false;
    Ray               r     = make_ray(mk3(0, 0, 0), mk3(0, 0, 1), 0.f, 0.f);
    WideRay           w     = make_wide_ray(r.o, r.d);
    WideCursor        c;
    wide_cursor_root(c);
    float    best_t = 0.f, best_u = 0.f, best_v = 0.f;
    uint32_t best_gid = kInvalidId, out = 0;
    while (true)
    {
        unsigned long long m_alive = __ballot(alive);
        if (64u - (uint32_t)__popcll(m_alive) >= refill_idle)
            query_refill(s, q, rbuf, lane, alive, m_alive, [&](float4 a, float4 b, uint32_t i) {
                if (!query_admit<false>(q, a, b, i)) return false;
                r      = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
                w      = make_wide_ray(r.o, r.d);
                best_t = r.tmax, best_u = 0.f, best_v = 0.f, best_gid = kInvalidId;
                out    = i;
                wide_cursor_root(c);
                st.sp = 0;
                return true;
            });
        if (m_alive == 0ull)
        {
            if (s.buf_pos >= s.buf_n && s.pend_n == 0) break;  // feed ended and every lane retired
            continue;
        }
        // one load sequence serves node and triangle lanes (see k_trace_closest8)
        const bool    tri_lane = alive && c.t_hits != 0u, node_lane = alive && c.t_hits == 0u;
        const float4* src      = bvh.nodes8;
        if (tri_lane)
            src = bvh.tris8 + 4 * (size_t)wide_pick_triangle(c);
        else if (node_lane)
        {
            bool           rest;
            const uint32_t node = wide_pick_child(c, w.octinv, rest);
            if (rest) st.push(c.g_base, c.g_mask);
            src = bvh.nodes8 + (kWideNodeStride / 4u) * (size_t)node;
        }
        WideNode nd;
#define CAP_DEF4(v) asm volatile("" : "=v"((v).x), "=v"((v).y), "=v"((v).z), "=v"((v).w))  // (see k_trace_closest8)
        CAP_DEF4(nd.h0);
        CAP_DEF4(nd.h1);
        CAP_DEF4(nd.q2);
        CAP_DEF4(nd.q3);
        CAP_DEF4(nd.q4);
#undef CAP_DEF4
        if (alive) nd.h0 = src[0], nd.h1 = src[1], nd.q2 = src[2], nd.q3 = src[3];
        if (node_lane) nd.q4 = src[4];
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
        if (alive && c.t_hits == 0u && (c.g_mask >> 24) == 0u)
        {
            if (st.sp == 0)
            {
                hits[out] = make_float4(best_t, best_u, best_v, u2f(best_gid));
                alive     = false;
            }
            else
                st.pop(c);
        }
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
    __shared__ uint2  lds_stack[kQueryLds * kBlock];
    __shared__ float4 lds_rays[2 * kBlock];
    const uint32_t  lane = threadIdx.x & 63u;
    float4* const   rbuf = lds_rays + (threadIdx.x >> 6) * 128u;
    uint32_t* const occ  = static_cast<uint32_t*>(q.out);
    QueryFeedState  s{grab_issue(q.work, 0), 0, 0, 0, 0, 0, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    query_fetch(s, q, lane);

    WideStack<kQueryLds> st{lds_stack + threadIdx.x, wide_spill_of_thread(bvh), 0};
    bool              alive = false;
    Ray               r     = make_ray(mk3(0, 0, 0), mk3(0, 0, 1), 0.f, 0.f);
    WideRay           w     = make_wide_ray(r.o, r.d);
    WideCursor        c;
    wide_cursor_root(c);
    uint32_t out = 0;
    while (true)
    {
        unsigned long long m_alive = __ballot(alive);
        if (64u - (uint32_t)__popcll(m_alive) >= refill_idle)
            query_refill(s, q, rbuf, lane, alive, m_alive, [&](float4 a, float4 b, uint32_t i) {
                if (!query_admit<true>(q, a, b, i)) return false;
                r   = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
                w   = make_wide_ray(r.o, r.d);
                out = i;
                wide_cursor_root(c);
                st.sp = 0;
                return true;
            });
        if (m_alive == 0ull)
        {
            if (s.buf_pos >= s.buf_n && s.pend_n == 0) break;
            continue;
        }
        const bool    tri_lane = alive && c.t_hits != 0u, node_lane = alive && c.t_hits == 0u;
        const float4* src      = bvh.nodes8;
        if (tri_lane)
            src = bvh.tris8 + 4 * (size_t)wide_pick_triangle(c);
        else if (node_lane)
        {
            bool           rest;
            const uint32_t node = wide_pick_child(c, kAnyOct(w.octinv), rest);
            if (rest) st.push(c.g_base, c.g_mask);
            src = bvh.nodes8 + (kWideNodeStride / 4u) * (size_t)node;
        }
        WideNode nd;
#define CAP_DEF4(v) asm volatile("" : "=v"((v).x), "=v"((v).y), "=v"((v).z), "=v"((v).w))
        CAP_DEF4(nd.h0);
        CAP_DEF4(nd.h1);
        CAP_DEF4(nd.q2);
        CAP_DEF4(nd.q3);
        CAP_DEF4(nd.q4);
#undef CAP_DEF4
        if (alive) nd.h0 = src[0], nd.h1 = src[1], nd.q2 = src[2];
        if (FILTER && tri_lane) nd.q3 = src[3];
        if (node_lane) nd.q3 = src[3], nd.q4 = src[4];  // (a plain occlusion test reads 48 of a triangle record's 64 bytes)
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
        else if (alive && c.t_hits == 0u && (c.g_mask >> 24) == 0u)
        {
            if (st.sp == 0)
            {
                occ[out] = 0u;
                alive    = false;
            }
            else
                st.pop(c);
        }
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

void launch_query8(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, bool any, const RayFilter* f, bool first_hit)
{
    uint32_t       g   = (q.n + kBlock - 1) / kBlock;
    uint32_t       cap = cfg.cu_count ? cfg.cu_count * (uint32_t)CAP_W8_BLOCKS : cfg.grid_blocks;
    if ((uint64_t)cap * kBlock > bvh.spill_threads) cap = bvh.spill_threads / kBlock;  // every thread owns a spill slice
    if (g > cap) g = cap;
    if (g == 0) g = 1;
    const long     v      = (long)cfg.sw_get(SW_W8_REFILL, CAP_W8_REFILL);  // (clamped as trace8.hip w8_refill_idle does)
    const uint32_t refill = (uint32_t)(v < 1 ? 1 : v > 64 ? 64 : v);
    if (f)
    {
        if (any)
            hipLaunchKernelGGL(k_query_any8_f, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill, *f);
        else if (first_hit)
            hipLaunchKernelGGL(k_query_first8_f, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill, *f);
        else
            hipLaunchKernelGGL(k_query_closest8_f, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill, *f);
    }
    else if (any)
        hipLaunchKernelGGL(k_query_any8, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill);
    else
        hipLaunchKernelGGL(k_query_closest8, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill);
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
    __shared__ uint2  lds_stack[kQueryLds * kBlock];
    __shared__ float4 lds_rays[2 * kBlock];
    const QueryArgs& q    = m.q;
    const uint32_t   lane = threadIdx.x & 63u;
    float4* const    rbuf = lds_rays + (threadIdx.x >> 6) * 128u;
    QueryFeedState   s{grab_issue(q.work, 0), 0, 0, 0, 0, 0, make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    query_fetch(s, q, lane);

    WideStack<kQueryLds> st{lds_stack + threadIdx.x, wide_spill_of_thread(bvh), 0};
    bool              alive = false;
    Ray               r     = make_ray(mk3(0, 0, 0), mk3(0, 0, 1), 0.f, 0.f);
    WideRay           w     = make_wide_ray(r.o, r.d);
    WideCursor        c;
    wide_cursor_root(c);
    HitList<K> L;
    L.init(m.k, 0.f);
    float    tc = 0.f, lo = 0.f;
    uint32_t gc = 0u, count = 0u, out = 0;
    while (true)
    {
        unsigned long long m_alive = __ballot(alive);
        if (64u - (uint32_t)__popcll(m_alive) >= refill_idle)
            query_refill(s, q, rbuf, lane, alive, m_alive, [&](float4 a, float4 b, uint32_t i) {
                if (!query_ray_ok(a, b))
                {
                    multi_write_miss(m, i, b.w);
                    return false;
                }
                if (!query_origin_safe(a, q.safe))
                {
                    q.defer[atomicAdd(q.work + kCounterStride, 1u)] = i;
                    return false;
                }
                r = make_ray(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, b.w);
                w = make_wide_ray(r.o, r.d);
                L.init(m.k, r.tmax);
                multi_cursor(m, i, tc, gc);
                lo    = fmaxf(r.tmin, tc);
                count = 0u;
                out   = i;
                wide_cursor_root(c);
                st.sp = 0;
                return true;
            });
        if (m_alive == 0ull)
        {
            if (s.buf_pos >= s.buf_n && s.pend_n == 0) break;
            continue;
        }
        const bool    tri_lane = alive && c.t_hits != 0u, node_lane = alive && c.t_hits == 0u;
        const float4* src      = bvh.nodes8;
        if (tri_lane)
            src = bvh.tris8 + 4 * (size_t)wide_pick_triangle(c);
        else if (node_lane)
        {
            bool           rest;
            const uint32_t node = wide_pick_child(c, w.octinv, rest);
            if (rest) st.push(c.g_base, c.g_mask);
            src = bvh.nodes8 + (kWideNodeStride / 4u) * (size_t)node;
        }
        WideNode nd;
#define CAP_DEF4(v) asm volatile("" : "=v"((v).x), "=v"((v).y), "=v"((v).z), "=v"((v).w))  // (see k_trace_closest8)
        CAP_DEF4(nd.h0);
        CAP_DEF4(nd.h1);
        CAP_DEF4(nd.q2);
        CAP_DEF4(nd.q3);
        CAP_DEF4(nd.q4);
#undef CAP_DEF4
        if (alive) nd.h0 = src[0], nd.h1 = src[1], nd.q2 = src[2], nd.q3 = src[3];
        if (node_lane) nd.q4 = src[4];
        if (tri_lane)
        {
            float t, u, v;
            if (query_tri_test<FILTER>(r, nd.h0, nd.h1, nd.q2, f, t, u, v) && (!FILTER || filter_admits(f, f2u(nd.q3.x))))
                multi_offer<K, COUNT>(L, count, tc, gc, t, f2u(nd.q3.x));
        }
        if (node_lane) wide_node_test(nd, w, lo, COUNT ? r.tmax : L.t[K - 1], c);
        if (alive && c.t_hits == 0u && (c.g_mask >> 24) == 0u)
        {
            if (st.sp == 0)
            {
                multi_write<K, COUNT>(m, bvh, out, r, L, count);
                alive = false;
            }
            else
                st.pop(c);
        }
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

// k_query_binary_multi under a filter (cap_trace_rays_multi_ex).  A kernel of its own rather than a second instantiation of one body:
// here, unlike in the wide kernels, wrapping the loop in a shared function changed the plain kernel's instruction schedule.
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
// traverse_closest's with tri_test_cull and the mask in front of the best record.  MODE 0: closest; 1: first accepted hit ends the
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
            if (sp == 0) break;
            node = (int)stack[(--sp) * kBlock];
        }
        if (MODE == 2)
            static_cast<uint32_t*>(q.out)[i] = found ? 1u : 0u;
        else
            static_cast<float4*>(q.out)[i] = make_float4(best_t, best_u, best_v, u2f(best_gid));
    }
}

uint32_t multi_bucket(uint32_t k) { return k <= 1 ? 1u : k <= 4 ? 4u : k <= 8 ? 8u : 16u; }

template <int K, bool COUNT>
static void launch_multi8_k(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, uint32_t refill, const RayFilter* f)
{
    uint32_t g   = (m.q.n + kBlock - 1) / kBlock;
    uint32_t cap = cfg.cu_count ? cfg.cu_count * (uint32_t)multi8_blocks(K) : cfg.grid_blocks;
    if ((uint64_t)cap * kBlock > bvh.spill_threads) cap = bvh.spill_threads / kBlock;  // every thread owns a spill slice
    if (g > cap) g = cap;
    if (g == 0) g = 1;
    if (f)
        hipLaunchKernelGGL((k_query_multi8_f<K, COUNT>), dim3(g), dim3(kBlock), 0, cfg.stream, bvh, m, refill, *f);
    else
        hipLaunchKernelGGL((k_query_multi8<K, COUNT>), dim3(g), dim3(kBlock), 0, cfg.stream, bvh, m, refill);
}

void launch_query8_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, const RayFilter* f)
{
    const long     v      = (long)cfg.sw_get(SW_W8_REFILL, CAP_W8_REFILL);
    const uint32_t refill = (uint32_t)(v < 1 ? 1 : v > 64 ? 64 : v);
#define CAP_MULTI8(K)                                                         \
    if (m.counts)                                                             \
        launch_multi8_k<K, true>(cfg, bvh, m, refill, f);                     \
    else                                                                      \
        launch_multi8_k<K, false>(cfg, bvh, m, refill, f);
    switch (multi_bucket(m.k))
    {
    case 1: CAP_MULTI8(1) break;
    case 4: CAP_MULTI8(4) break;
    case 8: CAP_MULTI8(8) break;
    default: CAP_MULTI8(16) break;
    }
#undef CAP_MULTI8
}

template <int STACK, int K, bool COUNT>
static void launch_binary_multi_k(const LaunchCfg& cfg, const BvhDev& b, const MultiArgs& m, bool deferred, const RayFilter* f)
{
    uint32_t want = (m.q.n + kBlock - 1) / kBlock;
    // (deferred: the count is on the device and is normally small -- one workgroup per CU at most)
    if (deferred && cfg.cu_count && want > cfg.cu_count) want = cfg.cu_count;
    if (want == 0) want = 1;
    if (f)
        hipLaunchKernelGGL((k_query_binary_multi_f<STACK, K, COUNT>), dim3(resident_grid<k_query_binary_multi_f<STACK, K, COUNT>>(cfg, want)),
                           dim3(kBlock), 0, cfg.stream, b, m, deferred ? 1u : 0u, *f);
    else
        hipLaunchKernelGGL((k_query_binary_multi<STACK, K, COUNT>), dim3(resident_grid<k_query_binary_multi<STACK, K, COUNT>>(cfg, want)),
                           dim3(kBlock), 0, cfg.stream, b, m, deferred ? 1u : 0u);
}

template <int STACK>
static void launch_binary_multi_s(const LaunchCfg& cfg, const BvhDev& b, const MultiArgs& m, bool deferred, const RayFilter* f)
{
#define CAP_MULTI_BIN(K)                                                      \
    if (m.counts)                                                             \
        launch_binary_multi_k<STACK, K, true>(cfg, b, m, deferred, f);        \
    else                                                                      \
        launch_binary_multi_k<STACK, K, false>(cfg, b, m, deferred, f);
    switch (multi_bucket(m.k))
    {
    case 1: CAP_MULTI_BIN(1) break;
    case 4: CAP_MULTI_BIN(4) break;
    case 8: CAP_MULTI_BIN(8) break;
    default: CAP_MULTI_BIN(16) break;
    }
#undef CAP_MULTI_BIN
}

void launch_query_binary_multi(const LaunchCfg& cfg, const BvhDev& bvh, const MultiArgs& m, bool deferred, const RayFilter* f)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    if (cfg.stack_entries <= 32)
        launch_binary_multi_s<32>(cfg, b, m, deferred, f);
    else
        launch_binary_multi_s<64>(cfg, b, m, deferred, f);
}

template <int STACK, int MODE>
static void launch_binary_f(const LaunchCfg& cfg, const BvhDev& b, const QueryArgs& q, const RayFilter& f, bool deferred)
{
    uint32_t want = (q.n + kBlock - 1) / kBlock;
    if (deferred && cfg.cu_count && want > cfg.cu_count) want = cfg.cu_count;  // (as launch_query_binary)
    if (want == 0) want = 1;
    hipLaunchKernelGGL((k_query_binary_f<STACK, MODE>), dim3(resident_grid<k_query_binary_f<STACK, MODE>>(cfg, want)), dim3(kBlock), 0, cfg.stream,
                       b, q, deferred ? 1u : 0u, f);
}

void launch_query_binary_filtered(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, const RayFilter& f, bool any, bool first_hit, bool deferred)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
#define CAP_BIN_F(S)                                               \
    if (any)                                                       \
        launch_binary_f<S, 2>(cfg, b, q, f, deferred);             \
    else if (first_hit)                                            \
        launch_binary_f<S, 1>(cfg, b, q, f, deferred);             \
    else                                                           \
        launch_binary_f<S, 0>(cfg, b, q, f, deferred);
    if (cfg.stack_entries <= 32)
    {
        CAP_BIN_F(32)
    }
    else
    {
        CAP_BIN_F(64)
    }
#undef CAP_BIN_F
}
}  // namespace cap
