// query.hip — ray queries of caller-supplied rays (cap_trace_rays / cap_trace_occlusion) on the compressed 8-wide view (cap_wide.h),
// gfx950.
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

// Closest hit: CapHit (t, u, v, asfloat(triangle)) per ray; a miss is (tmax, 0, 0, ~0).
__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_closest8(BvhDev bvh, QueryArgs q, uint32_t refill_idle)
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
            if (tri_test(r, nd.h0, nd.h1, nd.q2, t, u, v))
            {
                const uint32_t gid = f2u(nd.q3.x);
                if (t < best_t || (t == best_t && gid < best_gid)) best_t = t, best_u = u, best_v = v, best_gid = gid;
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

// Occlusion: 1 when some triangle has tmin det < T < tmax det (tri_occludes), else 0, one word per ray.  The lane-refill form of
// k_trace_any8_refill with the caller's rays: per-lane octant (caller rays share no light direction), back-to-front visiting order
// (kAnyOrder) and early exit at the first occluder.
__global__ __launch_bounds__(kBlock, CAP_W8_BLOCKS) void k_query_any8(BvhDev bvh, QueryArgs q, uint32_t refill_idle)
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
        if (node_lane) nd.q3 = src[3], nd.q4 = src[4];  // (an occlusion test reads 48 of a triangle record's 64 bytes)
        bool occluded = false;
        if (tri_lane) occluded = tri_occludes(r, nd.h0, nd.h1, nd.q2);
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

bool query8_stack_matches() { return (uint32_t)kQueryLds + kSpillEntries / 2u == wide8_stack_pairs(); }

void launch_query8(const LaunchCfg& cfg, const BvhDev& bvh, const QueryArgs& q, bool any)
{
    uint32_t       g   = (q.n + kBlock - 1) / kBlock;
    uint32_t       cap = cfg.cu_count ? cfg.cu_count * (uint32_t)CAP_W8_BLOCKS : cfg.grid_blocks;
    if ((uint64_t)cap * kBlock > bvh.spill_threads) cap = bvh.spill_threads / kBlock;  // every thread owns a spill slice
    if (g > cap) g = cap;
    if (g == 0) g = 1;
    const long     v      = (long)cfg.sw_get(SW_W8_REFILL, CAP_W8_REFILL);  // (clamped as trace8.hip w8_refill_idle does)
    const uint32_t refill = (uint32_t)(v < 1 ? 1 : v > 64 ? 64 : v);
    if (any)
        hipLaunchKernelGGL(k_query_any8, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill);
    else
        hipLaunchKernelGGL(k_query_closest8, dim3(g), dim3(kBlock), 0, cfg.stream, bvh, q, refill);
}
}  // namespace cap
