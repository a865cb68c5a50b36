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
//
// The instanced form (cap_overlap_instances, k_overlap_inst) is at the end of the file: world-space boxes over the instance table, the
// pairs (instance, triangle) whose world record meets the box, in (instance, triangle) order.
//
// Behind the instanced form: the triangle form (cap_overlap_triangles, k_overlap_triangles) -- a query triangle for the box, a 17-axis
// triangle-against-triangle predicate for the 13 axes, the same walk against the box of the query's vertices.  And last its instanced
// form (cap_overlap_triangles_instances, k_overlap_tri_inst): k_overlap_inst's loop with the triangle predicate, pruned in world space
// below an instance as well (world_node_step).
#include "cap_kernels.h"
#include "cap_near.h"        // the prune of the instanced form
#include "cap_query_walk.h"  // TopWalk, and the launch dispatchers

namespace cap
{
namespace
{
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

// An inner node against the grown query box [gl, gh]: one fetch yields both child boxes; a child is kept unless it lies beyond the box on
// some axis (cap_near.h overlap_miss: strict, touching opens, a NaN opens); both kept: child 0 is entered and child 1 pushed; one kept:
// it is entered.  false: neither is kept, the caller pops.  A walk pushes at most one entry per level it descends and STACK is at least
// the tree's depth (with_stack_class); the guard drops a push beyond it rather than write outside the lane's LDS column.
template <int STACK>
__device__ __forceinline__ bool box_node_step(const BvhDev& bvh, float glx, float gly, float glz, float ghx, float ghy, float ghz, uint32_t* stack, int& node,
                                              int& sp)
{
    // child 0: lo (q0.x q0.y q0.z) hi (q0.w q1.x q1.y); child 1: lo (q1.z q1.w q2.x) hi (q2.y q2.z q2.w)
    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
    const bool   k0 = !overlap_miss(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, glx, gly, glz, ghx, ghy, ghz);
    const bool   k1 = !overlap_miss(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, glx, gly, glz, ghx, ghy, ghz);
    const int    c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
    if (k0 && k1)
    {
        if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)c1;
        node = c0;
        return true;
    }
    if (k0 || k1)
    {
        node = k0 ? c0 : c1;
        return true;
    }
    return false;
}

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
                    if (box_node_step<STACK>(bvh, glx, gly, glz, ghx, ghy, ghz, stack, node, sp)) continue;
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

// ---- over the instance table (cap_overlap_instances) ----
// For every WORLD-space box the pairs (instance, triangle) whose world record -- cap_closest_instances' (world_record, cap_query_walk.h),
// from the transform M as the caller gave it -- meets the box under box_meets above, unchanged; the first k in (instance, triangle)
// order, their number, or both.  One loop with three kinds of step, as k_closest_inst (point_query.hip), so that the lanes of a wave
// that are at the top level advance while others are inside an instance:
//   * a top-level node: its two children's stored world boxes against the query box grown by the top-level slack (no order, no bound:
//     top_advance with far_first = false and distances of 0);
//   * entering an instance: mask, cursor, M, and the object-space image of the query box (cap_near.h overlap_image), once per pair of
//     box and instance;
//   * a bottom-level node or leaf: box_node_step on the object's tree against the image; a leaf builds the world record and calls
//     box_meets with the world-space BoxFrame.
// Every skip is overlap_miss's strict "x < y": touching opens, and so does an image that is not finite (lo = -FLT_MAX, hi = 0 under a
// scaling instance: c' + h' is -inf + inf).  DESIGN.md "Box overlap queries over instances" has the argument that no skipped box holds
// a candidate.
// The list is K keys (instance << 32 | triangle) in registers, ascending: two words per slot either way, and the 64-bit compare is one
// v_cmp_lt_u64 where the lexicographic offer of two words is two compares and an and-or.  The cursor (i_c, g_c) is such a key; an
// instance below i_c is not entered at all -- the major key of the order makes that exact, so it changes no result.
template <int K>
struct PairList
{
    uint64_t key[K];
    __device__ __forceinline__ void init(uint32_t k)
    {
#pragma unroll
        for (int j = 0; j < K; ++j) key[j] = j >= K - (int)k ? ~0ull : 0ull;
    }
    __device__ __forceinline__ void offer(uint64_t id)
    {
#pragma unroll
        for (int j = K - 1; j > 0; --j) key[j] = max(key[j - 1], min(id, key[j]));
        key[0] = min(id, key[0]);
    }
};
// the two pages of one query: slot s is list entry s + skip (skip = K - k placeholders in front), through the chain of K selects
template <int K>
__device__ __forceinline__ void write_pair_pages(const PairList<K>& L, uint32_t k, int skip, uint32_t* page, uint32_t* ipage)
{
    for (uint32_t s = 0; s < k; ++s)
    {
        uint64_t key = ~0ull;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (q - skip == (int)s) key = L.key[q];
        page[s]  = (uint32_t)key;
        ipage[s] = (uint32_t)(key >> 32);
    }
}

// One top-level node: both children's stored world boxes against the grown query box (a record with k < 0 holds nothing: an inert
// instance or the padding of a level); then down, or the instances into the queue, or up (top_advance)
__device__ __forceinline__ TopWalk overlap_top_step(const TlasDev& tl, const uint32_t* lds_off, float glx, float gly, float glz, float ghx, float ghy,
                                                    float ghz, TopWalk t)
{
    const float4* c = tl.tlas + 2 * (size_t)(lds_off[t.level - 1u] + 2u * t.idx);
    const float4  lo0 = c[0], hi0 = c[1], lo1 = c[2], hi1 = c[3];
    const bool    h0 = lo0.w >= 0.0f && !overlap_miss(lo0.x, lo0.y, lo0.z, hi0.x, hi0.y, hi0.z, glx, gly, glz, ghx, ghy, ghz);
    const bool    h1 = lo1.w >= 0.0f && !overlap_miss(lo1.x, lo1.y, lo1.z, hi1.x, hi1.y, hi1.z, glx, gly, glz, ghx, ghy, ghz);
    return top_advance(t, h0, h1, false, f2u(hi0.w), f2u(hi1.w), 0.f, 0.f);
}

// Workgroups per CU.  LDS as overlap_blocks', but for the 104 bytes of level offsets, which take the fifth workgroup of STACK = 32 away
// (5 x 32 872 B is 520 B more than the CU has).  Registers (tools/kernel_regs.sh; the table is in DESIGN.md "Box overlap queries over
// instances"): the walk holds M, the frame, the image and the top-level state beside the list's 2 K words.  Compiled without a limit
// that binds (STACK = 64, two workgroups) the kernel takes 86 to 88 VGPRs at K = 1, 100 to 102 at K = 4, 116 to 118 at K = 8 and 148 to
// 150 at K = 16: five waves per SIMD (96 each), four (128), four and three (168) are what those sizes admit anyway, so the limits below
// cost no instantiation a register, let alone scratch.  (Four workgroups at K = 16 leave 128 and spill 84 to 92 bytes.)
constexpr int overlap_inst_blocks(int STACK, int K)
{
    const int by_lds  = STACK <= 16 ? 8 : STACK <= 24 ? 6 : STACK <= 32 ? 4 : 2;
    const int by_regs = K <= 1 ? 5 : K <= 8 ? 4 : 3;
    return by_lds < by_regs ? by_lds : by_regs;
}

// FILTER: a mesh-mask table is installed (f.tri_mask by global id); the instance's own mask is tested either way.
template <int STACK, int K, bool FILTER>
__global__ __launch_bounds__(kBlock, overlap_inst_blocks(STACK, K)) void k_overlap_inst(BvhDev bvh, OverlapInstArgs ia, TlasDev tl, RayFilter f)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const OverlapArgs& a      = ia.a;
    const float        xw_all = u2f(ia.xw_max[0]);  // the largest Xw of the table: the top level's slack holds for every instance
    const int          skip   = K - (int)a.k;        // the placeholders
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.n; j += gridDim.x * kBlock)
    {
        const float4    lo = a.boxes[2 * (size_t)j], hi = a.boxes[2 * (size_t)j + 1];
        uint32_t* const page  = a.out + (size_t)j * a.k;
        uint32_t* const ipage = ia.inst_out + (size_t)j * a.k;
        PairList<K>     L;
        L.init(a.k);
        uint32_t count = 0u;
        if (box_ok(lo, hi) && bvh.tri_count != 0u)
        {
            // only pairs above the cursor -- slot k - 1 of the box's two pages -- count and are listed; (~0, ~0) admits nothing
            const bool     open = a.resume == 0u;
            const uint32_t ic   = open ? 0u : ipage[a.k - 1u];
            const uint64_t kc   = open ? 0ull : ((uint64_t)ic << 32) | page[a.k - 1u];
            const BoxFrame b    = box_frame(lo, hi);
            const float    bmax = overlap_box_max(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
            const float    slack_top = overlap_slack(bmax, xw_all);
            const float    glx = lo.x - slack_top, gly = lo.y - slack_top, glz = lo.z - slack_top;
            const float    ghx = hi.x + slack_top, ghy = hi.y + slack_top, ghz = hi.z + slack_top;
            TopWalk        t   = top_start(tl);
            // bottom level: the instance being walked
            bool     in_blas = false;
            float4   m0 = make_float4(0.f, 0.f, 0.f, 0.f), m1 = m0, m2 = m0;
            float    olo[3] = {0.f, 0.f, 0.f}, ohi[3] = {0.f, 0.f, 0.f};
            uint32_t inst = 0u, imask = 0u;
            int      node = 0, sp = 0;
            for (;;)
            {
                if (in_blas)
                {
                    if (node >= 0)
                    {
                        if (box_node_step<STACK>(bvh, olo[0], olo[1], olo[2], ohi[0], ohi[1], ohi[2], stack, node, sp)) continue;
                    }
                    else
                    {
                        const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                        for (uint32_t leaf = first; leaf <= last; ++leaf)
                        {
                            const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                            if constexpr (FILTER)
                                if ((f.tri_mask[gid] & imask) == 0u) continue;
                            const WorldRecord w = world_record(m0, m1, m2, bvh.tris[4 * (size_t)leaf + 0], bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2]);
                            if (!box_meets(b, w.t0, w.t1, w.t2)) continue;
                            const uint64_t key = ((uint64_t)inst << 32) | gid;
                            if (open || key > kc)
                            {
                                ++count;
                                L.offer(key);
                            }
                        }
                    }
                    in_blas = sp != 0;
                    if (in_blas) node = (int)stack[(--sp) * kBlock];
                    continue;
                }
                if (t.todo0 != kInvalidId)
                {
                    // the head of the queue: its mask joined with the call's (0 for an inert instance; the mesh byte joins it per
                    // triangle), the cursor's instance, then M, the image of the box under the stored W and the root of the object's tree
                    inst = t.todo0;
                    t    = top_pop(t);
                    const float4 w3 = tl.rec[4 * (size_t)inst + 3];
                    imask           = f2u(w3.x) & f.mask;
                    if (imask == 0u || inst < ic) continue;
                    const float4 w0 = tl.rec[4 * (size_t)inst], w1 = tl.rec[4 * (size_t)inst + 1], w2 = tl.rec[4 * (size_t)inst + 2];
                    const float  w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
                    const float2 nr = ia.near[inst];  // (g, Xw)
                    overlap_image(w, b.cx, b.cy, b.cz, b.hx, b.hy, b.hz, overlap_slack(bmax, nr.y) / nr.x, olo, ohi);
                    m0 = ia.descs[4 * (size_t)inst], m1 = ia.descs[4 * (size_t)inst + 1], m2 = ia.descs[4 * (size_t)inst + 2];
                    node = (int)f2u(w3.y), sp = 0, in_blas = true;
                    continue;
                }
                if (t.done) break;
                t = overlap_top_step(tl, lds_off, glx, gly, glz, ghx, ghy, ghz, t);
            }
        }
        // (a box that was not traversed: the list as init left it, k empty slots in both pages, and count 0)
        if (a.counts) a.counts[j] = count;
        write_pair_pages(L, a.k, skip, page, ipage);
    }
}

// ---- triangle against triangle (cap_overlap_triangles) ----
// For every query triangle (A0, A1, A2) the scene triangles that meet it, by the 17-axis separating-axis predicate of
// include/capsaicin_hip.h ("triangle overlap queries") in the frame at A0; pages, counts and cursor as k_overlap_boxes, whose walk this is.
//
// Pruning: step 1 of the predicate -- the coordinate axes, on absolute coordinates, exact -- makes "the predicate holds" imply "the box
// of the COMPUTED scene vertices meets the box [min A, max A] of the query's vertices" exactly: that is step (i) of DESIGN.md "Box overlap
// queries", Pruning, with [lo, hi] = [min A, max A], and steps (ii) to (iv) follow unchanged.  So the walk is box_node_step against that
// box grown by run.slack.
//
// Per query, once: p1, p2, n = cross(p1, p2), the three cross(n, f_i) and the [min s, max s] intervals of those four axes -- the
// operations of the contract, hoisted.  An interval with a NaN among its three values is stored as [-inf, +inf], which nothing lies
// beyond: the axis separates nothing, as the contract says.
__device__ __forceinline__ v3    cross_c(v3 u, v3 v) { return v3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ float dot_c(v3 a, v3 b) { return dot_c(a.x, a.y, a.z, b.x, b.y, b.z); }

// min > max of the contract for two triples, where min and max hand a NaN on: every t above every s or every t below every s, and
// nothing with a NaN among the six.  fminf and fmaxf drop a NaN, so the three unordered tests stand beside them.
__device__ __forceinline__ bool axis_separates(float s0, float s1, float s2, float t0, float t1, float t2)
{
    const bool  nan  = __builtin_isunordered(s0, s1) || __builtin_isunordered(s2, t0) || __builtin_isunordered(t1, t2);
    const float smin = fminf(fminf(s0, s1), s2), smax = fmaxf(fmaxf(s0, s1), s2);
    const float tmin = fminf(fminf(t0, t1), t2), tmax = fmaxf(fmaxf(t0, t1), t2);
    return !nan && (tmin > smax || tmax < smin);
}

// [min s, max s] of one of the query's own axes; with a NaN among them [-inf, +inf]
struct Interval
{
    float lo, hi;
};
__device__ __forceinline__ Interval interval_of(float s0, float s1, float s2)
{
    const float inf = __builtin_inff();
    const bool  nan = __builtin_isunordered(s0, s1) || __builtin_isunordered(s2, s2);
    return Interval{nan ? -inf : fminf(fminf(s0, s1), s2), nan ? inf : fmaxf(fmaxf(s0, s1), s2)};
}

struct TriFrame
{
    v3       a0, p1, p2;    // A0; p1 = A1 - A0, p2 = A2 - A0 (p0 = A0 - A0 is +0)
    v3       lo, hi;        // min / max of the three vertices, absolute: the coordinate axes
    v3       n, c0, c1, c2; // cross(p1, p2); cross(n, f_i), f0 = p1, f1 = p2 - p1, f2 = p0 - p2
    Interval in, i0, i1, i2;
};
__device__ __forceinline__ Interval interval_on(v3 L, v3 p0, v3 p1, v3 p2) { return interval_of(dot_c(L, p0), dot_c(L, p1), dot_c(L, p2)); }
__device__ __forceinline__ TriFrame tri_frame(const float4 qa, const float4 qb, const float4 qc)
{
    TriFrame t;
    const v3 a1 = mk3(qb.x, qb.y, qb.z), a2 = mk3(qc.x, qc.y, qc.z);
    t.a0 = mk3(qa.x, qa.y, qa.z);
    t.lo = mk3(fminf(fminf(t.a0.x, a1.x), a2.x), fminf(fminf(t.a0.y, a1.y), a2.y), fminf(fminf(t.a0.z, a1.z), a2.z));
    t.hi = mk3(fmaxf(fmaxf(t.a0.x, a1.x), a2.x), fmaxf(fmaxf(t.a0.y, a1.y), a2.y), fmaxf(fmaxf(t.a0.z, a1.z), a2.z));
    const v3 p0 = t.a0 - t.a0;
    t.p1 = a1 - t.a0, t.p2 = a2 - t.a0;
    t.n  = cross_c(t.p1, t.p2);
    t.c0 = cross_c(t.n, t.p1), t.c1 = cross_c(t.n, t.p2 - t.p1), t.c2 = cross_c(t.n, p0 - t.p2);
    t.in = interval_on(t.n, p0, t.p1, t.p2);
    t.i0 = interval_on(t.c0, p0, t.p1, t.p2), t.i1 = interval_on(t.c1, p0, t.p1, t.p2), t.i2 = interval_on(t.c2, p0, t.p1, t.p2);
    return t;
}

// one of the query's own axes against the scene triangle: the t_j beyond the stored interval
__device__ __forceinline__ bool own_axis(v3 L, Interval s, v3 q0, v3 q1, v3 q2)
{
    const float t0 = dot_c(L, q0), t1 = dot_c(L, q1), t2 = dot_c(L, q2);
    return all_above(t0, t1, t2, s.hi) || all_below(t0, t1, t2, s.lo);
}
// an axis that depends on the scene triangle: all six values
__device__ __forceinline__ bool pair_axis(v3 L, v3 p0, v3 p1, v3 p2, v3 q0, v3 q1, v3 q2)
{
    return axis_separates(dot_c(L, p0), dot_c(L, p1), dot_c(L, p2), dot_c(L, q0), dot_c(L, q1), dot_c(L, q2));
}

// The predicate of the contract for the record (t0, t1, t2) = (v0, e1, e2): one rounded binary32 operation per operation written there.
// Three groups of axes with one return each: the coordinate axes, the two normals, the other fifteen.
__device__ __forceinline__ bool tri_meets(const TriFrame& t, const float4 t0, const float4 t1, const float4 t2)
{
    const v3 b0 = mk3(t0.x, t0.y, t0.z), e1 = mk3(t0.w, t1.x, t1.y), e2 = mk3(t1.z, t1.w, t2.x);
    const v3 b1 = b0 + e1, b2 = b0 + e2;
    // 1. the coordinate axes, absolute coordinates
    if (all_above(b0.x, b1.x, b2.x, t.hi.x) || all_below(b0.x, b1.x, b2.x, t.lo.x) || all_above(b0.y, b1.y, b2.y, t.hi.y) ||
        all_below(b0.y, b1.y, b2.y, t.lo.y) || all_above(b0.z, b1.z, b2.z, t.hi.z) || all_below(b0.z, b1.z, b2.z, t.lo.z))
        return false;
    // 2. the frame at A0
    const v3 p0 = t.a0 - t.a0;
    const v3 q0 = b0 - t.a0, q1 = b1 - t.a0, q2 = b2 - t.a0;
    // 3. the two normals
    const v3 m = cross_c(e1, e2);
    if (own_axis(t.n, t.in, q0, q1, q2) || pair_axis(m, p0, t.p1, t.p2, q0, q1, q2)) return false;
    // the nine cross(f_i, g_j), the three cross(n, f_i), the three cross(m, g_j)
    const v3 f[3] = {t.p1, t.p2 - t.p1, p0 - t.p2};
    const v3 g[3] = {e1, q2 - q1, q0 - q2};
    bool     sep  = own_axis(t.c0, t.i0, q0, q1, q2) || own_axis(t.c1, t.i1, q0, q1, q2) || own_axis(t.c2, t.i2, q0, q1, q2);
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        sep |= pair_axis(cross_c(m, g[j]), p0, t.p1, t.p2, q0, q1, q2);
#pragma unroll
        for (int i = 0; i < 3; ++i) sep |= pair_axis(cross_c(f[i], g[j]), p0, t.p1, t.p2, q0, q1, q2);
    }
    return !sep;
}

// a query that is traversed: nine finite coordinates (a NaN fails its comparison)
__device__ __forceinline__ bool tri_ok(const float4 a, const float4 b, const float4 c)
{
    const float inf = __builtin_inff();
    return fabsf(a.x) < inf && fabsf(a.y) < inf && fabsf(a.z) < inf && fabsf(b.x) < inf && fabsf(b.y) < inf && fabsf(b.z) < inf && fabsf(c.x) < inf &&
           fabsf(c.y) < inf && fabsf(c.z) < inf;
}

// Workgroups per CU.  LDS is overlap_blocks'.  Registers: the frame is 35 words beside the grown box, the list and the walk, and the
// fifteen axes of the last group keep the scene triangle's nine frame coordinates and six edge words live across them.  Compiled
// without a limit that binds (STACK = 64, two workgroups) the kernel takes 99 (K = 1), 106 (4), 114 (8) and 130 (16) VGPRs
// (tools/kernel_regs.sh; the table is in DESIGN.md "Triangle overlap queries"): four waves per SIMD leave 128 each and three leave 168,
// which those sizes admit anyway, so the limits below cost no instantiation a register, let alone scratch.
constexpr int overlap_tri_blocks(int STACK, int K)
{
    const int by_lds  = STACK <= 16 ? 8 : STACK <= 24 ? 6 : STACK <= 32 ? 5 : 2;
    const int by_regs = K <= 8 ? 4 : 3;
    return by_lds < by_regs ? by_lds : by_regs;
}

// FILTER as in k_overlap_boxes.  a.queries: three float4 per query, (a, skip) (b, -) (c, -); a scene triangle whose global id is
// `skip` is as if it were not in the scene, like one the mask rejects.
template <int STACK, int K, bool FILTER>
__global__ __launch_bounds__(kBlock, overlap_tri_blocks(STACK, K)) void k_overlap_triangles(BvhDev bvh, OverlapTriArgs a, RayFilter f)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    const int           skip  = K - (int)a.k;  // the placeholders
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += gridDim.x * kBlock)
    {
        const float4    qa = a.queries[3 * (size_t)i], qb = a.queries[3 * (size_t)i + 1], qc = a.queries[3 * (size_t)i + 2];
        uint32_t* const page = a.out + (size_t)i * a.k;
        IdList<K>       L;
        L.init(a.k);
        uint32_t count = 0u;
        if (tri_ok(qa, qb, qc))
        {
            // only ids above the cursor -- slot k - 1 of the query's page -- count and are listed; ~0 (a short page's last slot) admits nothing
            const bool     open = a.resume == 0u;
            const uint32_t gc   = open ? 0u : page[a.k - 1u];
            const uint32_t own  = f2u(qa.w);
            const TriFrame t    = tri_frame(qa, qb, qc);
            const float    glx = t.lo.x - a.slack, gly = t.lo.y - a.slack, glz = t.lo.z - a.slack;
            const float    ghx = t.hi.x + a.slack, ghy = t.hi.y + a.slack, ghz = t.hi.z + a.slack;
            int            node = bvh.root, sp = 0;
            while (bvh.tri_count != 0u)
            {
                if (node >= 0)
                {
                    if (box_node_step<STACK>(bvh, glx, gly, glz, ghx, ghy, ghz, stack, node, sp)) continue;
                }
                else
                {
                    const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                    for (uint32_t leaf = first; leaf <= last; ++leaf)
                    {
                        const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                        if (gid == own) continue;
                        if constexpr (FILTER)
                            if ((f.tri_mask[gid] & f.mask) == 0u) continue;
                        const float4 t0 = bvh.tris[4 * (size_t)leaf + 0], t1 = bvh.tris[4 * (size_t)leaf + 1], t2 = bvh.tris[4 * (size_t)leaf + 2];
                        if (!tri_meets(t, t0, t1, t2)) continue;
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
        // (a query that was not traversed: the list as init left it, k empty slots, and count 0)
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

// ---- triangle against triangle over the instance table (cap_overlap_triangles_instances) ----
// For every WORLD-space query triangle the pairs (instance, triangle) whose world record (world_record, from M as given) meets it under
// tri_meets above, unchanged; pages, counts and cursor as k_overlap_inst, whose three-kind-of-step loop this is.  What differs is the
// prune below an instance.  k_overlap_inst tests the object's node boxes against the object-space image of the query box, which rests
// on the box predicate bringing a candidate within 15 eps U of the box itself.  The triangle predicate gives only its step 1 -- the
// computed world vertex box meets [min A, max A] -- and for the pairs the 17 axes cannot decide (two coplanar segments that do not
// cross) the scene triangle need not come anywhere near the query's box in any other frame.  So the walk prunes in WORLD space below
// an instance as well: every child box of the object's tree is mapped to its world box under M (cap_near.h overlap_world_box) and kept
// unless that misses [min A, max A] grown by the instance's slack.  DESIGN.md "Triangle overlap queries over instances" has the
// argument (it needs c2 = 26 of the shipped 96).
//
// An inner node of the object's tree against the grown world query box [gl, gh]: box_node_step with both child boxes mapped to world
// space first.  m: the 12 words of M.  The push, the enter and the guard are box_node_step's.
template <int STACK>
__device__ __forceinline__ bool world_node_step(const BvhDev& bvh, const float m[12], float glx, float gly, float glz, float ghx, float ghy, float ghz,
                                                uint32_t* stack, int& node, int& sp)
{
    const float4 q0 = bvh.nodes[4 * node + 0], q1 = bvh.nodes[4 * node + 1], q2 = bvh.nodes[4 * node + 2], q3 = bvh.nodes[4 * node + 3];
    float        lo0[3], hi0[3], lo1[3], hi1[3];
    overlap_world_box(m, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, lo0, hi0);
    overlap_world_box(m, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, lo1, hi1);
    const bool k0 = !overlap_miss(lo0[0], lo0[1], lo0[2], hi0[0], hi0[1], hi0[2], glx, gly, glz, ghx, ghy, ghz);
    const bool k1 = !overlap_miss(lo1[0], lo1[1], lo1[2], hi1[0], hi1[1], hi1[2], glx, gly, glz, ghx, ghy, ghz);
    const int  c0 = (int)f2u(q3.z), c1 = (int)f2u(q3.w);
    if (k0 && k1)
    {
        if (sp < STACK) stack[(sp++) * kBlock] = (uint32_t)c1;
        node = c0;
        return true;
    }
    if (k0 || k1)
    {
        node = k0 ? c0 : c1;
        return true;
    }
    return false;
}

// Workgroups per CU.  LDS is overlap_inst_blocks' (the stack and the 104 bytes of level offsets).  Registers (tools/kernel_regs.sh; the
// table is in DESIGN.md "Triangle overlap queries over instances"): the triangle frame's 35 words, M, the two grown boxes and the
// top-level state beside the list's 2 K words.  Compiled without a limit that binds (STACK = 64, two workgroups) the kernel takes 134
// to 135 VGPRs at K = 1, 147 to 149 at K = 4, 164 to 165 at K = 8 and 196 to 197 at K = 16: three waves per SIMD leave 168 each and
// two leave 256, which those sizes admit anyway, so the limits below cost no instantiation a register, let alone scratch.  (Four
// workgroups at K = 1 leave 128 and spill 12 bytes.)
constexpr int overlap_tri_inst_blocks(int STACK, int K)
{
    const int by_lds  = STACK <= 16 ? 8 : STACK <= 24 ? 6 : STACK <= 32 ? 4 : 2;
    const int by_regs = K <= 8 ? 3 : 2;
    return by_lds < by_regs ? by_lds : by_regs;
}

// FILTER as in k_overlap_inst.  ia.a.queries: three float4 per query, (a, skip) (b, skip_instance) (c, -): the pair (skip_instance, skip)
// is as if it were not in the table, like one the masks reject; no triangle has the id ~0, so a skip of ~0 skips nothing.
template <int STACK, int K, bool FILTER>
__global__ __launch_bounds__(kBlock, overlap_tri_inst_blocks(STACK, K)) void k_overlap_tri_inst(BvhDev bvh, OverlapTriInstArgs ia, TlasDev tl, RayFilter f)
{
    __shared__ uint32_t lds_stack[STACK * kBlock];
    __shared__ uint32_t lds_off[kTlasMaxLevels + 1];
    uint32_t* const     stack = lds_stack + threadIdx.x;
    if (threadIdx.x <= tl.top) lds_off[threadIdx.x] = tl.level_off[threadIdx.x];
    __syncthreads();
    const OverlapTriArgs& a      = ia.a;
    const float           xw_all = u2f(ia.xw_max[0]);  // the largest Xw of the table: the top level's slack holds for every instance
    const int             skip   = K - (int)a.k;        // the placeholders
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < a.n; j += gridDim.x * kBlock)
    {
        const float4    qa = a.queries[3 * (size_t)j], qb = a.queries[3 * (size_t)j + 1], qc = a.queries[3 * (size_t)j + 2];
        uint32_t* const page  = a.out + (size_t)j * a.k;
        uint32_t* const ipage = ia.inst_out + (size_t)j * a.k;
        PairList<K>     L;
        L.init(a.k);
        uint32_t count = 0u;
        if (tri_ok(qa, qb, qc) && bvh.tri_count != 0u)
        {
            // only pairs above the cursor -- slot k - 1 of the query's two pages -- count and are listed; (~0, ~0) admits nothing
            const bool     open = a.resume == 0u;
            const uint32_t ic   = open ? 0u : ipage[a.k - 1u];
            const uint64_t kc   = open ? 0ull : ((uint64_t)ic << 32) | page[a.k - 1u];
            const uint64_t own  = ((uint64_t)f2u(qb.w) << 32) | f2u(qa.w);  // the skip pair as a key
            const TriFrame t    = tri_frame(qa, qb, qc);
            const float    bmax = overlap_box_max(t.lo.x, t.lo.y, t.lo.z, t.hi.x, t.hi.y, t.hi.z);
            const float    slack_top = overlap_slack(bmax, xw_all);
            const float    glx = t.lo.x - slack_top, gly = t.lo.y - slack_top, glz = t.lo.z - slack_top;
            const float    ghx = t.hi.x + slack_top, ghy = t.hi.y + slack_top, ghz = t.hi.z + slack_top;
            TopWalk        w   = top_start(tl);
            // bottom level: the instance being walked, its M and the world query box grown by its own slack
            bool     in_blas = false;
            float    m[12]   = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float    slack   = 0.f;
            uint32_t inst = 0u, imask = 0u;
            int      node = 0, sp = 0;
            for (;;)
            {
                if (in_blas)
                {
                    if (node >= 0)
                    {
                        if (world_node_step<STACK>(bvh, m, t.lo.x - slack, t.lo.y - slack, t.lo.z - slack, t.hi.x + slack, t.hi.y + slack, t.hi.z + slack, stack,
                                                   node, sp))
                            continue;
                    }
                    else
                    {
                        const uint32_t code = (uint32_t)~node, first = code & kLeafFirstMask, last = first + (code >> kLeafCountShift);
                        for (uint32_t leaf = first; leaf <= last; ++leaf)
                        {
                            const uint32_t gid = f2u(bvh.tris[4 * (size_t)leaf + 3].x);
                            const uint64_t key = ((uint64_t)inst << 32) | gid;
                            if (key == own) continue;
                            if constexpr (FILTER)
                                if ((f.tri_mask[gid] & imask) == 0u) continue;
                            const WorldRecord r = world_record(make_float4(m[0], m[1], m[2], m[3]), make_float4(m[4], m[5], m[6], m[7]),
                                                               make_float4(m[8], m[9], m[10], m[11]), bvh.tris[4 * (size_t)leaf + 0],
                                                               bvh.tris[4 * (size_t)leaf + 1], bvh.tris[4 * (size_t)leaf + 2]);
                            if (!tri_meets(t, r.t0, r.t1, r.t2)) continue;
                            if (open || key > kc)
                            {
                                ++count;
                                L.offer(key);
                            }
                        }
                    }
                    in_blas = sp != 0;
                    if (in_blas) node = (int)stack[(--sp) * kBlock];
                    continue;
                }
                if (w.todo0 != kInvalidId)
                {
                    // the head of the queue: its mask joined with the call's (0 for an inert instance; the mesh byte joins it per
                    // triangle), the cursor's instance, then M, the instance's slack and the root of the object's tree
                    inst = w.todo0;
                    w    = top_pop(w);
                    const float4 w3 = tl.rec[4 * (size_t)inst + 3];
                    imask           = f2u(w3.x) & f.mask;
                    if (imask == 0u || inst < ic) continue;
                    const float4 m0 = ia.descs[4 * (size_t)inst], m1 = ia.descs[4 * (size_t)inst + 1], m2 = ia.descs[4 * (size_t)inst + 2];
                    m[0] = m0.x, m[1] = m0.y, m[2] = m0.z, m[3] = m0.w, m[4] = m1.x, m[5] = m1.y, m[6] = m1.z, m[7] = m1.w;
                    m[8] = m2.x, m[9] = m2.y, m[10] = m2.z, m[11] = m2.w;
                    slack = overlap_slack(bmax, ia.near[inst].y);  // (g, Xw): no division by g, the test stays in world space
                    node = (int)f2u(w3.y), sp = 0, in_blas = true;
                    continue;
                }
                if (w.done) break;
                w = overlap_top_step(tl, lds_off, glx, gly, glz, ghx, ghy, ghz, w);
            }
        }
        // (a query that was not traversed: the list as init left it, k empty slots in both pages, and count 0)
        if (a.counts) a.counts[j] = count;
        write_pair_pages(L, a.k, skip, page, ipage);
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

void launch_overlap_instances(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapInstArgs& a, const TlasDev& tl, const RayFilter& f, uint32_t depth)
{
    // (depth: of the deepest bottom-level tree)
    with_stack_class(depth, [&](auto S) {
        with_k_bucket(a.a.k, [&](auto K) {
            with_flag(f.tri_mask != nullptr, [&](auto FILTER) {
                launch_points<k_overlap_inst<decltype(S)::value, decltype(K)::value, decltype(FILTER)::value>>(cfg, a.a.n, bvh, a, tl, f);
            });
        });
    });
}
void launch_overlap_triangles_instances(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapTriInstArgs& a, const TlasDev& tl, const RayFilter& f,
                                        uint32_t depth)
{
    // (depth: of the deepest bottom-level tree)
    with_stack_class(depth, [&](auto S) {
        with_k_bucket(a.a.k, [&](auto K) {
            with_flag(f.tri_mask != nullptr, [&](auto FILTER) {
                launch_points<k_overlap_tri_inst<decltype(S)::value, decltype(K)::value, decltype(FILTER)::value>>(cfg, a.a.n, bvh, a, tl, f);
            });
        });
    });
}
void launch_overlap_triangles(const LaunchCfg& cfg, const BvhDev& bvh, const OverlapTriArgs& a, const RayFilter* f, uint32_t depth)
{
    BvhDev b   = bvh;
    b.wide8_ok = 0;
    const RayFilter rf = f ? *f : RayFilter{};
    with_stack_class(depth, [&](auto S) {
        with_k_bucket(a.k, [&](auto K) {
            with_flag(f && f->tri_mask, [&](auto FILTER) {
                launch_points<k_overlap_triangles<decltype(S)::value, decltype(K)::value, decltype(FILTER)::value>>(cfg, a.n, b, a, rf);
            });
        });
    });
}
}  // namespace cap
