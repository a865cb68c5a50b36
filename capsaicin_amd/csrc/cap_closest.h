// cap_closest.h — the per-triangle function of the closest-point contract (include/capsaicin_hip.h "closest-point queries"): the
// Voronoi-region cascade on a stored record (v0, e1, e2), one rounded binary32 operation per operation of the contract.  Shared by the
// closest-point kernels (point_query.hip) and the sphere sweep (sweep.hip), whose contract evaluates it at the swept centre.
#pragma once

#include "cap_query_walk.h"  // dot_c

namespace cap
{
namespace
{
struct ClosestPoint
{
    float    x, y, z, d2, u, v;
    uint32_t feature;
    float    dx, dy, dz;  // delta = ap - m, what d2 is made of (cap_signed_distance's sign)
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
    c.dx = dx, c.dy = dy, c.dz = dz;
    return c;
}
}  // namespace
}  // namespace cap
