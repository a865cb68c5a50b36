// overlap.hip — box overlap queries (cap_overlap_boxes) on the binary tree, gfx950: for every axis-aligned box the triangles that meet
// it, by the 13-axis separating-axis predicate of include/capsaicin_hip.h ("box overlap queries") on the stored records (v0, e1, e2) --
// the first k of them in id order, their number, or both.
//
// One lane per box, a grid-stride loop over the chunk as in k_closest_points_multi.  The walk has no order to exploit and no bound that
// shrinks: a node fetch yields both child boxes, a child is skipped when it lies beyond the query box grown by the scene's slack on
// some axis, and of two children kept child 0 is entered and child 1 pushed.  A stack entry is the child alone, 4 bytes in LDS strided
// by kBlock -- half the closest-point stack, there is no distance to test again on a pop.
//
// Pruning (DESIGN.md "Box overlap queries" has the argument): the predicate's first three axes make "the predicate holds" imply "the box
// of the COMPUTED vertices a, fl(v0 + e1), fl(v0 + e2) meets [lo, hi]" exactly; the computed vertices lie within 3 eps M of the uploaded
// ones, which every node box above the triangle contains; so a node box that misses [fl(lo - slack), fl(hi + slack)],
// slack = 64 eps max|scene coordinate|, holds no candidate.  The comparisons are strict: a node box that touches the grown box is opened.
//
// The list is K ids in registers, ascending; it prunes nothing, so a walk with counts is the walk without them and the count is one
// register and one wave-uniform store: not a template flag.
#include "cap_kernels.h"
#include "cap_query_walk.h"  // the launch dispatchers

namespace cap
{
namespace
{
// dot of the contract: no fused multiply-add (the build has -ffp-contract=off; fmaf is nowhere written)
__device__ __forceinline__ float dot_c(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// min(x0, x1, x2) > r and max(x0, x1, x2) < r of the contract, whose min and max hand a NaN on: three comparisons each, so that a NaN
// among the three separates nothing (v_min3_f32 would drop it)
__device__ __forceinline__ bool all_above(float x0, float x1, float x2, float r) { return x0 > r && x1 > r && x2 > r; }
__device__ __forceinline__ bool all_below(float x0, float x1, float x2, float r) { return x0 < r && x1 < r && x2 < r; }

// The box in the predicate's centred frame: hl = lo / 2, hh = hi / 2, ctr = hl + hh, h = hh - hl -- computed once per box
struct BoxFrame
{
    float lox, loy, loz, hix, hiy, hiz;
    float cx, cy, cz, hx, hy, hz;
};
__device__ __forceinline__ BoxFrame box_frame(const float4 lo, const float4 hi)
{
    BoxFrame     b;
    const float hlx = lo.x * 0.5f, hly = lo.y * 0.5f, hlz = lo.z * 0.5f, hhx = hi.x * 0.5f, hhy = hi.y * 0.5f, hhz = hi.z * 0.5f;
    b.lox = lo.x, b.loy = lo.y, b.loz = lo.z, b.hix = hi.x, b.hiy = hi.y, b.hiz = hi.z;
    b.cx = hlx + hhx, b.cy = hly + hhy, b.cz = hlz + hhz;
    b.hx = hhx - hlx, b.hy = hhy - hly, b.hz = hhz - hlz;
    return b;
}

// One cross axis of edge f for the coordinate pair (m, n): s_j = f_m P_j,n - f_n P_j,m for all three vertices, r = h_m |f_n| + h_n |f_m|.
// true: the axis separates.  (A NaN fails both comparisons.)
__device__ __forceinline__ bool cross_axis(float fm, float fn, float hm, float hn, float p0m, float p0n, float p1m, float p1n, float p2m, float p2n)
{
    const float s0 = fm * p0n - fn * p0m, s1 = fm * p1n - fn * p1m, s2 = fm * p2n - fn * p2m;
    const float r  = hm * fabsf(fn) + hn * fabsf(fm);
    return all_above(s0, s1, s2, r) || all_below(s0, s1, s2, -r);
}
// the three cross axes of one edge: (m, n) = (y, z), (z, x), (x, y)
__device__ __forceinline__ bool edge_axes(const BoxFrame& b, float fx, float fy, float fz, float p0x, float p0y, float p0z, float p1x, float p1y, float p1z,
                                          float p2x, float p2y, float p2z)
{
    return cross_axis(fy, fz, b.hy, b.hz, p0y, p0z, p1y, p1z, p2y, p2z) || cross_axis(fz, fx, b.hz, b.hx, p0z, p0x, p1z, p1x, p2z, p2x) ||
           cross_axis(fx, fy, b.hx, b.hy, p0x, p0y, p1x, p1y, p2x, p2y);
}

// The predicate of the contract for the record (t0, t1, t2) = (v0, e1, e2): one rounded binary32 operation per operation written there.
__device__ __forceinline__ bool box_meets(const BoxFrame& b, const float4 t0, const float4 t1, const float4 t2)
{
    const float ax = t0.x, ay = t0.y, az = t0.z;
    const float e1x = t0.w, e1y = t1.x, e1z = t1.y, e2x = t1.z, e2y = t1.w, e2z = t2.x;
    const float bx = ax + e1x, by = ay + e1y, bz = az + e1z, cx = ax + e2x, cy = ay + e2y, cz = az + e2z;
    // 1. the box axes, absolute coordinates
    if (all_above(ax, bx, cx, b.hix) || all_below(ax, bx, cx, b.lox)) return false;
    if (all_above(ay, by, cy, b.hiy) || all_below(ay, by, cy, b.loy)) return false;
    if (all_above(az, bz, cz, b.hiz) || all_below(az, bz, cz, b.loz)) return false;
    // 2. the centred frame
    const float p0x = ax - b.cx, p0y = ay - b.cy, p0z = az - b.cz;
    const float p1x = bx - b.cx, p1y = by - b.cy, p1z = bz - b.cz;
    const float p2x = cx - b.cx, p2y = cy - b.cy, p2z = cz - b.cz;
    // 4. the triangle's plane (before the nine cross axes: it rejects most of what the box axes let through)
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float d  = dot_c(nx, ny, nz, p0x, p0y, p0z);
    const float r  = (b.hx * fabsf(nx) + b.hy * fabsf(ny)) + b.hz * fabsf(nz);
    if (d > r || d < -r) return false;
    // 3. the nine cross axes: f0 = e1, f1 = P2 - P1, f2 = P0 - P2
    if (edge_axes(b, e1x, e1y, e1z, p0x, p0y, p0z, p1x, p1y, p1z, p2x, p2y, p2z)) return false;
    if (edge_axes(b, p2x - p1x, p2y - p1y, p2z - p1z, p0x, p0y, p0z, p1x, p1y, p1z, p2x, p2y, p2z)) return false;
    if (edge_axes(b, p0x - p2x, p0y - p2y, p0z - p2z, p0x, p0y, p0z, p1x, p1y, p1z, p2x, p2y, p2z)) return false;
    return true;
}

// a box that is traversed: six finite coordinates, lo <= hi on every axis (a NaN fails its comparison)
__device__ __forceinline__ bool box_ok(const float4 lo, const float4 hi)
{
    const float inf = __builtin_inff();
    return fabsf(lo.x) < inf && fabsf(lo.y) < inf && fabsf(lo.z) < inf && fabsf(hi.x) < inf && fabsf(hi.y) < inf && fabsf(hi.z) < inf && lo.x <= hi.x &&
           lo.y <= hi.y && lo.z <= hi.z;
}

// The K smallest ids seen, ascending.  k < K: the K - k slots in front are placeholders holding 0, which no id displaces (nothing is
// below it), the k live slots start as ~0.  k = 0: placeholders only, nothing is ever listed.
template <int K>
struct IdList
{
    uint32_t g[K];
    __device__ __forceinline__ void init(uint32_t k)
    {
#pragma unroll
        for (int j = 0; j < K; ++j) g[j] = j >= K - (int)k ? kInvalidId : 0u;
    }
    // slot j takes the larger of its lower neighbour and min(id, itself): an id at or above slot K - 1 changes nothing
    __device__ __forceinline__ void offer(uint32_t id)
    {
#pragma unroll
        for (int j = K - 1; j > 0; --j) g[j] = max(g[j - 1], min(id, g[j]));
        g[0] = min(id, g[0]);
    }
};

// Workgroups per CU.  The stack is 4 B x STACK x kBlock of the CU's 160 KB of LDS: 16 / 24 / 32 / 64 KB per workgroup, which admits
// 10 / 6 / 5 / 2 of them.  A workgroup is one wave on each of the four SIMDs and a SIMD holds 8 waves, so 10 becomes 8.  The 512 VGPRs
// of a SIMD lane shared by N waves leave 64 (N = 8), 72 (7), 80 (6), 96 (5) each, in granules of 8.  Compiled without a limit that
// binds, the kernel takes 52 (K = 1), 59 (4), 67 (8) and 84 (16) of them (tools/kernel_regs.sh; the table is in DESIGN.md): 8, 8, 7
// and 5 workgroups are what those sizes admit anyway, so the limits below cost no instantiation a register, let alone scratch.
constexpr int overlap_blocks(int STACK, int K)
{
    const int by_lds  = STACK <= 16 ? 8 : STACK <= 24 ? 6 : STACK <= 32 ? 5 : 2;
    const int by_regs = K <= 4 ? 8 : K <= 8 ? 7 : 5;
    return by_lds < by_regs ? by_lds : by_regs;
}

// FILTER: the mesh-mask table (RayFilter::tri_mask by global id), read before the record: a rejected triangle is as if it were not in
// the scene.  A flag of the kernel, as in k_closest_points_multi.
template <int STACK, int K, bool FILTER>
__global__ __launch_bounds__(kBlock, overlap_blocks(STACK, K)) void k_overlap_boxes(BvhDev bvh, OverlapArgs a, RayFilter f)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    const int           skip  = K - (int)a.k;  // the placeholders
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock)
    {
        const float4    lo = a.boxes[2 * (size_t)i], hi = a.boxes[2 * (size_t)i + 1];
        uint32_t* const page = a.out + (size_t)i * a.k;
        IdList<K>       L;
        L.init(a.k);
        uint32_t count = 0u;
        if (box_ok(lo, hi))
        {
            // only ids above the cursor -- slot k - 1 of the box's page -- count and are listed; ~0 (a short page's last slot) admits nothing
            const bool     open = a.resume == 0u;
            const uint32_t gc   = open ? 0u : page[a.k - 1u];
            const BoxFrame b    = box_frame(lo, hi);
            const float    glx = lo.x - a.slack, gly = lo.y - a.slack, glz = lo.z - a.slack;
            const float    ghx = hi.x + a.slack, ghy = hi.y + a.slack, ghz = hi.z + a.slack;
            int            node = bvh.root, sp = 0;
            while (bvh.tri_count != 0u)
            {
                if (node >= 0)
                {
                    // child 0: lo (q0.x q0.y q0.z) hi (q0.w q1.x q1.y); child 1: lo (q1.z q1.w q2.x) hi (q2.y q2.z q2.w)
                    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
                    const bool   k0 = !(q0.w < glx || q0.x > ghx || q1.x < gly || q0.y > ghy || q1.y < glz || q0.z > ghz);
                    const bool   k1 = !(q2.y < glx || q1.z > ghx || q2.z < gly || q1.w > ghy || q2.w < glz || q2.x > ghz);
                    const int    c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
                    // a walk pushes at most one entry per level it descends and STACK is at least the tree's depth (with_stack_class);
                    // the guard drops a push beyond it rather than write outside the lane's LDS column
                    if (k0 && k1)
                    {
                        if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)c1;
                        node = c0;
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
                        if (!box_meets(b, t0, t1, t2)) continue;
                        if (open || gid > gc)
                        {
                            ++count;
                            L.offer(gid);
                        }
                    }
                }
                if (sp == 0) break;
                node = (int)stack[(--sp) * kBlock];
            }
        }
        // (a box that was not traversed: the list as init left it, k empty slots, and count 0)
        if (a.counts) a.counts[i] = count;
        for (uint32_t s = 0; s < a.k; ++s)
        {
            uint32_t gid = kInvalidId;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j - skip == (int)s) gid = L.g[j];
            page[s] = gid;
        }
    }
}
}  // namespace

void launch_overlap_boxes(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapArgs& a, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const RayFilter rf = f ? *f : RayFilter{};
    with_stack_class(depth, [&](auto S) {
        with_k_bucket(a.k, [&](auto K) {
            with_flag(f && f->tri_mask, [&](auto FILTER) {
                launch_points<k_overlap_boxes<decltype(S)::value, decltype(K)::value, decltype(FILTER)::value>>(cfg, a.n, b, a, rf);
            });
        });
    });
}
}  // namespace cap
