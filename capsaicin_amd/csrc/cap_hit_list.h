// cap_hit_list.h -- the sorted per-lane list of the multi queries: the k nearest (key, triangle) pairs in (key, triangle) order.  The key
// is a ray's t (query.hip k_query_multi8 / k_query_binary_multi) or a point's dist2 (point_query.hip k_closest_points_multi);
// InstHitList below is the same structure with the instance between the key and the triangle, for the queries over the instance table
// (instance.hip k_query_inst_multi, point_query.hip k_closest_inst_multi).
//
// K pairs in VGPRs, K a compile-time bucket >= k; every index is a compile-time constant, so the list never goes to scratch.  The
// first K - k slots hold (-inf, 0) placeholders no candidate passes (every key is > -inf), the last k start as the miss (limit, ~0):
// "key <= limit", the tie rule and "the list is not full yet" are the one comparison of admits().  A pair below slot K - 1 replaces it
// and bubbles towards the front by K - 1 compare-swaps.  Slot K - 1 is the pruning bound: the limit until the list holds k pairs, then
// the k-th.
#pragma once
#include "cap_device.h"

namespace cap
{
template <int K>
struct HitList
{
    float    t[K];
    uint32_t g[K];
    __device__ __forceinline__ void init(uint32_t k, float tmax)
    {
#pragma unroll
        for (int j = 0; j < K; ++j)
        {
            const bool live = j >= K - (int)k;
            t[j] = live ? tmax : -__builtin_inff(), g[j] = live ? kInvalidId : 0u;
        }
    }
    __device__ __forceinline__ bool admits(float tt, uint32_t gg) const { return tt < t[K - 1] || (tt == t[K - 1] && gg < g[K - 1]); }
    __device__ __forceinline__ void insert(float tt, uint32_t gg)
    {
        t[K - 1] = tt, g[K - 1] = gg;
#pragma unroll
        for (int j = K - 1; j > 0; --j)
        {
            const bool     sw = t[j] < t[j - 1] || (t[j] == t[j - 1] && g[j] < g[j - 1]);
            const float    ta = t[j - 1], tb = t[j];
            const uint32_t ga = g[j - 1], gb = g[j];
            t[j - 1] = sw ? tb : ta, t[j] = sw ? ta : tb;
            g[j - 1] = sw ? gb : ga, g[j] = sw ? ga : gb;
        }
    }
};

// K (key, inst, gid) triples in VGPRs: the first K - k slots hold (-inf, 0, 0) placeholders no candidate passes, the last k start as the
// miss (limit, ~0, ~0).  A pair below slot K - 1 replaces it and bubbles towards the front by K - 1 compare-swaps.
template <int K>
struct InstHitList
{
    float    t[K];
    uint32_t i[K], g[K];
    static __device__ __forceinline__ bool before(float ta, uint32_t ia, uint32_t ga, float tb, uint32_t ib, uint32_t gb)
    {
        return ta < tb || (ta == tb && (ia < ib || (ia == ib && ga < gb)));
    }
    __device__ __forceinline__ void init(uint32_t k, float tmax)
    {
#pragma unroll
        for (int j = 0; j < K; ++j)
        {
            const bool live = j >= K - (int)k;
            t[j] = live ? tmax : -__builtin_inff(), i[j] = live ? kInvalidId : 0u, g[j] = live ? kInvalidId : 0u;
        }
    }
    __device__ __forceinline__ bool admits(float tt, uint32_t ii, uint32_t gg) const { return before(tt, ii, gg, t[K - 1], i[K - 1], g[K - 1]); }
    __device__ __forceinline__ void insert(float tt, uint32_t ii, uint32_t gg)
    {
        t[K - 1] = tt, i[K - 1] = ii, g[K - 1] = gg;
#pragma unroll
        for (int j = K - 1; j > 0; --j)
        {
            const bool     sw = before(t[j], i[j], g[j], t[j - 1], i[j - 1], g[j - 1]);
            const float    ta = t[j - 1], tb = t[j];
            const uint32_t ia = i[j - 1], ib = i[j], ga = g[j - 1], gb = g[j];
            t[j - 1] = sw ? tb : ta, t[j] = sw ? ta : tb;
            i[j - 1] = sw ? ib : ia, i[j] = sw ? ia : ib;
            g[j - 1] = sw ? gb : ga, g[j] = sw ? ga : gb;
        }
    }
};
}  // namespace cap
